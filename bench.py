#!/usr/bin/env python3
"""bench.py -- the hot path on BASELINE.json's headline workload.

Metric: effective GF/s (2:4 spmma vs dense gemm) on the ResNet-50 layer shapes, fp16, b = 32.
A "step" is one pass of the hot path over this rank's units of the table(s): for each layer the 2:4 prune + compress
of the per-batch activation operand A and the sparse x dense matmul -- as ONE fused kernel (sm_spmma_fused_f16) on the
layers where that wins (--path auto) and as sm_compress24_f16 + sm_spmma_f16 on the rest; both give the same C bit for
bit.  (This is compress(STRIP)+spmma on the UNPRUNED A, bit-identical to the reference's spmma() call sequence only for
an A that is already 2:4; the API-faithful sequence -- TILE prune in place, check, compress, multiply, spmma.hxx:82-113
-- is timed beside it as stages.api_spmma_ms.)  value = dense-equivalent flops (2*m*n*k per batch index, summed over
the units of every rank) / time.  Inputs are generated on the device, per (layer, global batch index), and are
resident in HBM before the timed region starts.  A step's launches, spread over 4 HIP streams, are captured once into a
hipGraph and replayed (the launches are 7-100 us each; without the graph the Python/ctypes call cost would be on the
clock).

Multi-GPU (--scaling): one process per GPU, no data-path collective, one tiny all-reduce (RCCL) of sum(flops) and
max(time).  weak (default): every rank runs every layer on its own b batch indices (rank r = global indices
[r*b, (r+1)*b)).  strong: every layer's batch is split [g*b/G, (g+1)*b/G), B replicated.  lpt: whole
layers, longest-processing-time assignment -- the config-4 sweep: --tables resnet50,resnet101,resnet152 --scaling lpt.

Besides the contract line's fields the JSON carries `stages` (matmul only, compress only, the API-faithful sequence and
the dense GEMMs that are the metric's denominator), `roofline` for the dominant kernel of the timed step and
`cpu_baseline` (the oracle's arithmetic timed on the host cores; rank 0, N = 1 only).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from benchlib.common import (F32_MATRIX_PEAK_TFS, GUIDE_COPY_GBS, HBM_PEAK_GBS, contract_line, file_tag, fused_variant, ge_mod, library_tag,  # noqa: E402,F401
                             read_shapes, table_path)
from benchlib.cpu import config1_cpu, cpu_baseline  # noqa: E402,F401
from benchlib.ranks import emulate_world, launch_ranks  # noqa: E402,F401
from benchlib.stages import bell_stage, config5_stage, conv_path_stage, conv_step_stage, extras  # noqa: E402,F401

DUMP_MAX_BYTES = 60 << 20   # --dump-outputs: what all ranks together write, at most


def dump_sample_index(numel, cap, unit):
    """Which elements of a unit's C --dump-outputs writes: all of them when they fit in `cap`, else `cap` of them, drawn without
    replacement by a generator seeded with the unit (layer, batch begin, batch end) and sorted: the same for every build and run."""
    import numpy as np
    if numel <= cap:
        return None
    return np.sort(np.random.default_rng([0x5EED, *unit]).choice(numel, cap, replace=False))


def dump_outputs(out_dir, layers, world):
    """C of every unit of this rank, as float32, one DIR/C_layer<i>_b<lo>-<hi>.npy per unit; each unit gets an equal share of
    DUMP_MAX_BYTES / world.  Returns what was written."""
    import numpy as np
    import torch
    units = {}
    for L in layers:
        units.setdefault(L["unit"], L["C_unit"])
    cap = DUMP_MAX_BYTES // 4 // (len(units) * world)
    os.makedirs(out_dir, exist_ok=True)
    nbytes, sampled = 0, 0
    for unit, C in sorted(units.items()):
        idx = dump_sample_index(C.numel(), cap, unit)
        x = C if idx is None else C[torch.from_numpy(idx).to(C.device)]
        a = x.float().cpu().numpy()
        np.save(os.path.join(out_dir, "C_layer%03d_b%d-%d.npy" % unit), a)
        nbytes += a.nbytes
        sampled += idx is not None
    return {"dir": out_dir, "arrays": len(units), "sampled": sampled, "elements_per_sampled_array": cap, "bytes": nbytes, "dtype": "float32"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--plan-costs", choices=["measure", "table"], default="measure",
                    help="per-shape costs of the hybrid plan: measured in setup on this box (one grouped launch per unique shape, outside "
                         "the timed region; rank 0's figures are broadcast) or the library's fallback table (sparsify.me_amd/multigpu.py)")
    ap.add_argument("--costs-file", default=None,
                    help="--emulate-world plumbing: the N = 1 child writes the costs it measured here, the rank children read them (so that "
                         "every emulated rank plans with the same numbers, as the broadcast does in a real N-GPU run)")
    ap.add_argument("--config4-stage", choices=["auto", "on", "off"], default="auto",
                    help="also time the config-4 sweep (resnet50 + 101 + 152, 300 layers, lpt) in the same run and report it as "
                         "stages.config4_sweep; auto = when N > 1 (north_star's >= 7x at 8 GPUs is stated on that sweep)")
    ap.add_argument("--streamk", choices=["on", "off"], default="off",
                    help="on: give the grouped fused launches a workspace (sm_spmma_fused_*_grouped_ws): the library then runs the stream-K form "
                         "on the shapes its rule names (round 5).  Default off: the form shortens a launch that runs ALONE (196 x 512 x 4608 x 3: "
                         "123 -> 106 us) but inside the 8-stream step, where other kernels fill a few-tile launch's idle CUs, its extra partial-sum "
                         "traffic costs more than its balance returns (1.600 / 1.608 ms against 1.591 / 1.588, profiles/bench_streamk_ab_r05f.txt)")
    ap.add_argument("--settle-ms", type=float, default=300.0,
                    help="setup, before the W warm-up steps: untimed replays of the step for this long (clock ramp after an idle "
                         "GPU, first-use state of a fresh graph); 0 = none.  Stated in config.launch")
    ap.add_argument("--tables", default=None,
                    help="comma-separated shape tables (names under datasets/ or paths), concatenated into one work list; "
                         "default resnet50 (fp16 / bf16) or resnet18 (f32: BASELINE config 2); "
                         "config 4 = resnet50,resnet101,resnet152")
    ap.add_argument("--table", default=None, help="one shape table (alias of --tables)")
    ap.add_argument("--scaling", choices=["weak", "strong", "lpt", "hybrid"], default=None,
                    help="multi-GPU partitioning of the (layer, batch) units: weak = every rank the whole table on its own "
                         "batch; strong = batch split b/G per layer; lpt = whole layers by longest-processing-time; hybrid = "
                         "batch split where a rank's share still fills the chip, whole layers (LPT) elsewhere.  Default: total "
                         "work fixed as N grows -- hybrid on one table, lpt on several (--tables); N = 1: all the same")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the per-stage / denominator passes")
    ap.add_argument("--eager", action="store_true", help="launch from Python instead of replaying a hipGraph")
    ap.add_argument("--path", choices=["auto", "staged"], default="auto",
                    help="auto: fused prune+compress+matmul kernel on the layers where it wins (n <= --fused-max-n), the "
                         "staged compress24 + spmma pair elsewhere; staged: the pair on every layer")
    ap.add_argument("--fused-max-n", type=int, default=512,
                    help="auto path: widest n served by sm_spmma_fused_f16 whatever k (one workgroup spans up to 256 columns: up to "
                         "there A is loaded and selected once, at 512 twice).  512 (default since round 3): inside the step, which is "
                         "bound by the bytes it moves, fusing the n = 512 long-K layers too is 3-4 %% faster than compress + spmma for "
                         "them (no blob written and re-read) although each such launch alone is slower; 256 = round 2's choice")
    ap.add_argument("--fused-max-k-wide", type=int, default=512,
                    help="auto path: wider layers (n > --fused-max-n) are still fused when k <= this (the A-stationary "
                         "kernel keeps the 2:4 image of a row panel in LDS across its column tiles); 0 = never")
    ap.add_argument("--batch-split", type=int, default=1,
                    help="run every layer's batch as this many independent problems of b / S entries (more, smaller work items "
                         "for the streams to interleave; same kernels, same results)")
    ap.add_argument("--dtype", choices=["f16", "bf16", "f32"], default="f16",
                    help="element type (BASELINE's metric is quoted on f16; bf16 runs the same kernels with the bfloat16 matrix "
                         "instructions; f32 is BASELINE config 2: sm_compress24_f32 + sm_spmma_f32 against the fp32 dense GEMMs, "
                         "default table resnet18)")
    ap.add_argument("--f32-planes", type=int, choices=[0, 2, 3], default=3,
                    help="--dtype f32: 3 (default since round 6) / 2 = the multiply on the sparse matrix instruction through exact bfloat16 "
                         "splits of both operands (sm_spmma_fused_f32_split: |error| <= 2^-21 / 2^-13 of sum|a||b|; north_star allows 1e-3, the "
                         "reference's library computes float operands in TF32) -- the default of sparsifyme::spmma<float> too "
                         "(spmma_options().f32_planes); 0 = the exact fp32 form (dense fp32 MFMA work on the selected operand)")
    ap.add_argument("--streams", type=int, default=8,
                    help="HIP streams the independent layers of a step are spread over (fork/join inside the step)")
    ap.add_argument("--graphs", choices=["single", "per-stream"], default="single",
                    help="hipGraph form of a step: one graph holding every chain (default) or one linear graph per stream")
    ap.add_argument("--sched", choices=["rr", "split", "lpt"], default="rr",
                    help="layer -> stream assignment: round-robin, or chip-filling layers (>= 784 row tiles) on the first half "
                         "of the streams and the under-filling ones on the second half")
    ap.add_argument("--group", choices=["on", "off"], default="on",
                    help="on (default): the fused layers of one (m, n, k, b) shape run as ONE grouped launch per 8 instances "
                         "(sm_spmma_fused_*_grouped: same kernels, same C bit for bit; the instances share the chip instead of each "
                         "paying its own last partial round of workgroups); off: one launch per layer")
    ap.add_argument("--no-span", action="store_true", help="auto path: k %% 64 != 0 layers on sm_compress24 + sm_spmma instead of the span-form fused kernel")
    ap.add_argument("--cost", choices=["bytes", "model"], default="bytes", help="what the longest-first spreading of work items balances")
    ap.add_argument("--item-order", choices=["big-first", "small-first"], default="big-first", help="order of a stream's items")
    ap.add_argument("--big-streams", type=int, default=2, help="--sched split: streams reserved for the chip-filling items")
    ap.add_argument("--emulate-world", type=int, default=0,
                    help="predict an N-GPU run on ONE GPU: the data path has no collective, so rank r's time is measurable alone. "
                         "For r = 0..N-1 a fresh child process (started before this process touches a GPU; it never does) runs rank "
                         "r's units of the --scaling plan; the parent reports max_r t_r, sum(flops) / max t and the spread, labelled "
                         "'predicted, single-GPU emulation' (no RCCL, no contention between ranks, one box's clock)")
    ap.add_argument("--emu-rank", type=int, default=None, help=argparse.SUPPRESS)  # child of --emulate-world: whose units to run
    ap.add_argument("--rank-bias-file", default=None, help=argparse.SUPPRESS)     # child of --emulate-world: the per-rank bias (us) of a re-planning round
    ap.add_argument("--rebalance", type=int, default=0,
                    help="N > 1, hybrid plan: rounds of closed-loop balancing in SETUP (before the W warm-up steps): every rank times its own step, "
                         "the times are all-gathered, the difference to the cost model becomes a per-rank bias and every rank re-plans with it; the "
                         "best plan measured is kept.  Default 0 = plan once from the per-shape costs measured on the box: in the 8-rank emulation the "
                         "loop did not pay (max rank time 0.2574 -> 0.2700 -> 0.2562 ms over two rounds, profiles/rebalance_r06h.txt: a rank's excess "
                         "over its modelled sum moves with the layers it holds, it is not a per-rank constant)")
    ap.add_argument("--detail", default=None,
                    help="where the full detail object (stages, families, yardstick, verified_layers, per-shape tables) is written; "
                         "default gpurun_out/bench_detail[_<dtype>].json.  stdout carries the compact contract line only")
    ap.add_argument("--full-line", action="store_true", help="print the full detail object on stdout instead of the compact contract line")
    ap.add_argument("--rehearse-gloo", action="store_true",
                    help="multi-rank rehearsal on a ONE-GPU box: gloo backend, every rank on cuda:0 (control flow only; "
                         "the ranks share the device, so the numbers mean nothing)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step computed -- the C of every (layer, batch range) unit of "
                         "this rank -- as float32 to DIR/C_layer<i>_b<lo>-<hi>.npy, at most 60 MiB in all: a C larger than its share is "
                         "written as a fixed, seeded sample of its elements (dump_sample_index).  The inputs are seeded, so two builds "
                         "run with the same arguments can be compared output for output")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("bench: --gpus must be >= 1")
    if args.steps < 1:
        raise SystemExit("bench: --steps must be >= 1")
    if args.dump_outputs and args.emulate_world:
        raise SystemExit("bench: --dump-outputs is not supported with --emulate-world")
    if args.emulate_world and args.emu_rank is None:
        raise SystemExit(emulate_world(args))
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: this process becomes the launcher of N ranks.  It has not imported torch and
        # never touches a GPU; the ranks are child processes (no exec), rank 0's JSON line and the exit code are relayed.
        raise SystemExit(launch_ranks(args))

    import torch
    import torch.distributed as dist
    import __graft_entry__ as ge

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:  # a launcher that realised another rank count than asked for must not pass as an N-GPU run
        raise SystemExit(f"bench: --gpus {args.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {args.gpus} "
                         f"(or run `python bench.py --gpus {args.gpus}`, which starts its own ranks)")
    if world > 1 and not args.rehearse_gloo and torch.cuda.device_count() < world:
        raise SystemExit(f"bench: {world} ranks asked for, {torch.cuda.device_count()} GPU(s) visible "
                         "(--rehearse-gloo rehearses the control flow on one GPU)")
    plan_world, plan_rank = (args.emulate_world, args.emu_rank) if args.emu_rank is not None else (world, rank)
    if args.scaling is None:
        ntab = len((args.tables or args.table or "x").split(","))
        args.scaling = "weak" if plan_world == 1 else ("lpt" if ntab > 1 else "hybrid")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.rehearse_gloo:
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", torch.cuda.current_device())

    sm = ge.load_package()
    mg = ge.load_package_module("multigpu")
    sm.device_check()  # raises when the HIP library or a gfx950 device is missing: no fallback

    f32 = args.dtype == "f32"
    tables = (args.tables or args.table or ("resnet18" if f32 else "resnet50")).split(",")
    tables = [table_path(t) for t in tables]
    shapes = [s_ for t in tables for s_ in read_shapes(t)]
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[args.dtype]
    # Costs the hybrid plan balances with (round 5): measured HERE, in setup, on the box that runs -- not a table from another box.
    # Every rank must plan with the same numbers: rank 0 measures and broadcasts (setup, not the data path); emulated ranks are
    # separate processes on one GPU and read what the N = 1 child measured (--costs-file).
    plan_costs = {"source": "fallback table (sparsify.me_amd/multigpu.py)"}
    if args.scaling == "hybrid" and plan_world > 1 and args.plan_costs == "measure" and not f32:
        costs = None
        if args.costs_file and os.path.exists(args.costs_file):
            costs = {tuple(int(x) for x in k_.split("x")): tuple(v) for k_, v in json.load(open(args.costs_file)).items()}
            plan_costs = {"source": "measured by the N = 1 child of this emulation (--costs-file)"}
        elif world > 1:
            box = [mg.measure_costs(sm, torch, shapes, tdt, world=world) if rank == 0 else None]
            dist.broadcast_object_list(box, src=0)
            costs = box[0]
            plan_costs = {"source": "measured in setup by rank 0 on this node (one grouped launch per unique shape), broadcast to all ranks"}
        if costs:
            mg.set_measured_costs(costs)
            plan_costs["us_per_instance"] = {"x".join(map(str, k_)): [round(x, 2) for x in v] for k_, v in costs.items()}
    elif args.costs_file and plan_world == 1 and not f32:   # the N = 1 child of an emulation: measure for the rank children
        costs = mg.measure_costs(sm, torch, shapes, tdt, world=(2, 4, 8))
        json.dump({"x".join(map(str, k_)): list(v) for k_, v in costs.items()}, open(args.costs_file, "w"))
    elif plan_world == 1 and world == 1 and not f32 and args.plan_costs == "measure" and not args.no_extras and args.emu_rank is None:
        # (round 6) a plain N = 1 run measures the plan costs on THIS box too -- at the full batch and at a rank's share for
        # 2 / 4 / 8 ranks -- and records them with the hybrid plan's predicted imbalance (max / mean modelled rank time), so that the line
        # of the first box of a node says what the N > 1 runs on that node will plan with.  Setup, outside the timed region.
        costs = mg.measure_costs(sm, torch, shapes, tdt, world=(2, 4, 8))
        mg.set_measured_costs(costs)
        plan_costs = {"source": "measured in setup on this box (one grouped launch per unique shape, at b and at b / 2, b / 4, b / 8 for the shapes "
                                "the hybrid plan splits by batch index)",
                      "us_per_instance": {"x".join(map(str, k_)): [round(x, 2) for x in v] for k_, v in costs.items()},
                      "hybrid_plan_predicted": {str(w_): {"max_over_mean": round(max(l_) / (sum(l_) / w_), 4), "max_rank_us": round(max(l_), 1),
                                                          "speedup_vs_n1_modelled": round(sum(mg.plan_loads(shapes, 1, "hybrid")) / max(l_), 3)}
                                                for w_ in (2, 4, 8) for l_ in [mg.plan_loads(shapes, w_, "hybrid")]}}
    rank_bias = json.load(open(args.rank_bias_file)) if (args.rank_bias_file and args.scaling == "hybrid") else None
    units = mg.plan_units(shapes, plan_world, plan_rank, args.scaling, rank_bias)
    es = 4 if f32 else 2

    def build_layers(shapes_, units_):
        """device operands of the units (layer, batch_begin, batch_end): A, B, blob, C per unit, seeded per (layer, global batch index)"""
        layers = []
        for (li, lo, hi) in units_:
            m, n, k, _ = shapes_[li]
            b = hi - lo
            A = torch.empty(b * m * k, dtype=tdt, device=dev)
            B = torch.empty(k * n, dtype=tdt, device=dev)
            for bi in range(lo, hi):  # operand of (layer, global batch index): the same matrix whatever the sharding
                sm.fill_uniform(A[(bi - lo) * m * k:(bi - lo + 1) * m * k], mg.unit_seed(0x5EED0000, li, bi), 0.0, 1.0)
            sm.fill_uniform(B, mg.unit_seed(0xB0000000, li, -1), 0.0, 1.0)
            blob = torch.empty(sm.compress24_size(m, k, es, b), dtype=torch.uint8, device=dev)
            C = torch.empty(b * m * n, dtype=tdt, device=dev)
            S = args.batch_split if args.batch_split > 1 and b % args.batch_split == 0 else 1
            if S == 1:
                layers.append(dict(li=li, m=m, n=n, k=k, b=b, A=A, B=B, blob=blob, C=C, unit=(li, lo, hi), C_unit=C))
            else:
                # --batch-split S: the layer's batch as S independent problems of b / S batch entries (views of the same operands; own
                # blobs): more, smaller work items for the streams to interleave -- same kernels, same C
                bs = b // S
                for s_ in range(S):
                    layers.append(dict(li=li, m=m, n=n, k=k, b=bs, A=A[s_ * bs * m * k:(s_ + 1) * bs * m * k], B=B,
                                       blob=torch.empty(sm.compress24_size(m, k, es, bs), dtype=torch.uint8, device=dev),
                                       C=C[s_ * bs * m * n:(s_ + 1) * bs * m * n], unit=(li, lo, hi), C_unit=C))
        return layers
    layers = build_layers(shapes, units)
    flops = mg.unit_flops(shapes, units)
    if f32 and args.f32_planes:
        # the split form's workspace (B's bfloat16 planes, written by every call) per layer, and -- asked once, in setup -- whether the form
        # takes the layer (k % 64 == 0 or the span form, n % 8 == 0); the others run the exact kernels
        for L in layers:
            L["ws"] = torch.empty(max(16, sm.spmma_fused_f32_split_workspace(L["n"], L["k"], planes=args.f32_planes)), dtype=torch.uint8, device=dev)
            L["split"] = sm.spmma_fused_f32_split(L["A"], L["B"], L["C"], L["m"], L["n"], L["k"], L["ws"], batch=L["b"], planes=args.f32_planes, check=False) == 0
        torch.cuda.synchronize()

    # The layers of a step are independent problems (the reference's sweep runs them as separate
    # processes, examples/profiling.py:6-17), so a step forks them over a few HIP streams and joins:
    # one layer's ramp-up and tail overlap another layer's streaming phase.  compress -> spmma of one
    # layer stay ordered on one stream.
    side = [torch.cuda.Stream() for _ in range(max(0, args.streams - 1))]
    nstreams = len(side) + 1
    def make_chains(layers_):
        """stream w runs chains[w] in order (the ungrouped step; the grouped step spreads work ITEMS instead: spread())"""
        chains_ = [[] for _ in range(nstreams)]
        cnt = [0, 0]
        for i, L in enumerate(layers_):
            w = i % nstreams
            if args.sched == "split" and nstreams >= 2:
                big = 0 if L["m"] * L["b"] >= 784 * 128 else 1
                half = [nstreams // 2, nstreams - nstreams // 2]
                w = (0 if big == 0 else half[0]) + cnt[big] % half[big]
                cnt[big] += 1
            chains_[w].append(L)
        if args.sched == "lpt":  # longest chain first by the layers' bytes (A + B + C: what the kernels stream), largest layers first
            def cost(L):
                return L["b"] * (L["m"] * L["k"] + L["m"] * L["n"]) + L["k"] * L["n"]
            chains_ = [[] for _ in range(nstreams)]
            load = [0] * nstreams
            for L in sorted(layers_, key=cost, reverse=True):
                w = load.index(min(load))
                chains_[w].append(L)
                load[w] += cost(L)
        return chains_
    chains = make_chains(layers)

    class Forked:
        """A step whose layers are spread over the streams: fork, one chain of layers per stream, join."""

        def __init__(self, per_layer, only=None):
            self.per_layer = per_layer
            self.only = only  # optional predicate: the layers this pass runs

        def fork_join(self, run_chain):
            main_s = torch.cuda.current_stream()
            for s_ in side:
                s_.wait_stream(main_s)
            run_chain(0)
            for w, s_ in enumerate(side, start=1):
                with torch.cuda.stream(s_):
                    run_chain(w)
            for s_ in side:
                main_s.wait_stream(s_)

        def chain(self, w):
            for L in chains[w]:
                if self.only is None or self.only(L):
                    self.per_layer(L)

        def __call__(self):  # launched kernel by kernel
            self.fork_join(self.chain)

    def layer_staged(L):
        sm.compress24(L["A"], L["m"], L["k"], L["k"], L["b"], L["m"] * L["k"], L["blob"])
        sm.spmma(L["blob"], L["B"], L["C"], L["m"], L["n"], L["k"], L["b"], 0)

    def use_fused(L):
        if f32:  # sm_spmma_fused_f32: the STRIP rule in the registers of the dense fp32 MFMA kernel (no blob, no compress pass)
            return args.path == "auto" and L["k"] % 32 == 0 and L["n"] % 4 == 0
        if L["n"] < 8 and L["k"] <= 64:  # the thin form (round 5): depthwise layers as im2col products, on the vector ALUs
            return args.path == "auto" and (L["b"] * L["m"] * L["k"] * 2) % 16 == 0
        if L["k"] % 64 != 0:  # the span form of sm_spmma_fused_*: ragged k (the stem layer, k = 147), n <= 128, span + B within the LDS
            return (args.path == "auto" and not args.no_span and L["n"] % 8 == 0 and L["n"] <= 128 and (L["b"] * L["m"] * L["k"] * 2) % 16 == 0 and
                    128 * L["k"] * 2 + 1152 + (L["k"] + 63) // 64 * 64 * (64 if L["n"] <= 64 else 128) * 2 <= 160 * 1024)
        return args.path == "auto" and (L["n"] <= args.fused_max_n or L["k"] <= args.fused_max_k_wide)

    # (f-1) the fused kernel computes the same C bit for bit straight from the dense A (the 2:4 selection
    # and compaction happen in registers / LDS; no blob goes to HBM)
    def layer_path(L):
        if L.get("split"):
            sm.spmma_fused_f32_split(L["A"], L["B"], L["C"], L["m"], L["n"], L["k"], L["ws"], batch=L["b"], planes=args.f32_planes)
        elif use_fused(L):
            sm.spmma_fused(L["A"], L["B"], L["C"], L["m"], L["n"], L["k"], batch=L["b"])
        else:
            layer_staged(L)

    # Work items of the timed step: with --group on the fused layers of one shape are one item (a grouped launch per 8
    # instances), every other layer is its own item; items are spread over the streams longest-first by their bytes.
    def layer_bytes(L):
        return L["b"] * (L["m"] * L["k"] + L["m"] * L["n"]) + L["k"] * L["n"]

    def fused_groups(Ls):
        """[(shape key, [layers])] of the fused layers in Ls, in table order of first appearance"""
        g = {}
        for L in Ls:
            g.setdefault((L["m"], L["n"], L["k"], L["b"]), []).append(L)
        return list(g.items())

    sk_ws = {}   # shape -> the stream-K workspace of that shape's grouped launches (one per work item: items run concurrently)

    def sk_takes(L0, cnt):
        """does the library run the stream-K form on a grouped launch of `cnt` instances of L0's shape? (its own rule, asked through
        sm_spmma_fused_streamk_plan -- nothing is mirrored here)"""
        if f32 or args.streamk != "on" or L0["k"] % 64 != 0 or L0["n"] <= 128:
            return False
        return sm.spmma_fused_streamk_plan(L0["m"] * L0["b"], L0["n"], L0["k"], cnt)[0]

    def run_group(Ls):
        L0 = Ls[0]
        key = (L0["m"], L0["n"], L0["k"], L0["b"])
        if key not in sk_ws:   # decided once per shape, at the first (untimed) call
            chunks = {min(8, len(Ls) - i) for i in range(0, len(Ls), 8)}
            sk_ws[key] = sm.spmma_fused_workspace() if any(sk_takes(L0, c) for c in chunks) else None
        sm.spmma_fused_grouped([L["A"] for L in Ls], [L["B"] for L in Ls], [L["C"] for L in Ls], L0["m"], L0["n"], L0["k"], batch=L0["b"],
                               workspace=sk_ws[key])

    grouped = args.group == "on" and not f32

    def item_cost(it):
        """what a work item costs a stream: its bytes (--cost bytes) or those bytes over the rate its kernel family reaches
        alone (--cost model: direct 4.9, span 2.9, wide 3.0, A-stationary 3.1 TB/s, profiles/bench_r03k.json)"""
        by = sum(layer_bytes(L) for L in it[1])
        if args.cost == "bytes" or f32:
            return by
        L0 = it[1][0]
        rate = {"direct": 4.9, "span": 2.9, "wide": 3.0, "astat": 3.1, "big": 3.2, "thin": 3.0}[fused_variant(L0["n"], L0["k"])] if use_fused(L0) else 3.0
        return by / rate

    def spread(items):
        """items [(kind, [layers])] -> per-stream chains, longest-first onto the least-loaded stream."""
        items = sorted(items, key=lambda it: -item_cost(it))
        ch, load = [[] for _ in range(nstreams)], [0] * nstreams
        nbig = min(max(1, args.big_streams), nstreams - 1) if (args.sched == "split" and nstreams >= 2) else 0
        for it in items:
            # --sched split: the chip-filling items (>= 784 row tiles per instance: they stream at the HBM rate whatever runs
            # beside them) go to the first `--big-streams` streams, the few-tile items (bound by per-tile latency, they
            # leave CUs idle) to the others, so that a few-tile kernel always has a streaming kernel beside it
            if nbig:
                big = it[1][0]["m"] * it[1][0]["b"] >= 784 * 128
                cand = range(0, nbig) if big else range(nbig, nstreams)
            else:
                cand = range(nstreams)
            w = min(cand, key=lambda c: load[c])
            ch[w].append(it)
            load[w] += item_cost(it)
        if args.item_order == "small-first":  # a stream ends on its chip-filling items: the step's tail is not left to few-tile kernels
            ch = [list(reversed(c)) for c in ch]
        return ch

    class ForkedItems(Forked):
        """A step of work items (a group of same-shape layers launched as one grid, or a single layer) spread over the streams."""

        def __init__(self, ch, run_group_fn, run_single_fn):
            Forked.__init__(self, run_single_fn)
            self.ch, self.run_group_fn = ch, run_group_fn

        def chain(self, w):
            for kind, Ls in self.ch[w]:
                if kind == "group":
                    self.run_group_fn(Ls)
                else:
                    self.per_layer(Ls[0])

    def assemble(layers_):
        """the timed step of these layers: (callable, number of grouped launches)"""
        if grouped:
            items = [("group", Ls) for _, Ls in fused_groups([L for L in layers_ if use_fused(L)])]
            items += [("single", [L]) for L in layers_ if not use_fused(L)]
            return ForkedItems(spread(items), run_group, layer_path), sum((len(Ls) + 7) // 8 for kind, Ls in items if kind == "group")
        return Forked(layer_path), 0
    step_full, n_launch_groups = assemble(layers)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def make_runner(fn):
        """fn replayed from a hipGraph (one graph = one call of fn), or fn itself with --eager.  --graphs per-stream
        turns a Forked step into one linear graph per stream, replayed into its own stream between the fork and the
        join (measured the same as the single graph, profiles/ktrace_r01l.txt)."""
        fn()  # first call outside capture: lazy module loads, function attributes
        torch.cuda.synchronize()
        if args.eager:
            return fn
        try:
            if isinstance(fn, Forked) and args.graphs == "per-stream":
                graphs = []
                for w in range(nstreams):
                    gw = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gw, stream=torch.cuda.Stream()):
                        fn.chain(w)
                    graphs.append(gw)
                return lambda: fn.fork_join(lambda w: graphs[w].replay())
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=torch.cuda.Stream()):
                fn()
            return g.replay
        except Exception as e:  # capture unsupported: fall back to eager launches, and say so
            sys.stderr.write(f"bench: hipGraph capture failed ({e}); launching eagerly\n")
            return fn

    def timed(run, steps, warmup, collective=True):
        """Wall time of `steps` calls.  collective=False: rank-local timing (the per-stage / per-family passes only rank
        0 runs: a distributed barrier there would pair with the other ranks' final barrier and hang the job)."""
        sync = barrier if collective else torch.cuda.synchronize
        for _ in range(warmup):
            run()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        sync()
        return wall

    def event_seconds(run, reps, warmup=2):
        """Device time per call by a HIP event pair on the stream the work is launched on (torch's current stream: the
        graph replays and the eager launches both go there)."""
        for _ in range(warmup):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    run_full = make_runner(step_full)
    # Closed-loop balancing of the hybrid plan (round 6; N > 1 only, SETUP -- before the settle and warm-up steps): a rank's step of ~10
    # launches over 8 streams is not the sum of its launches alone, so the plan built from per-shape costs leaves 12-17 % between the
    # slowest rank and the mean at 8 ranks.  Every rank times its own step, the times are all-gathered (the same list on every rank), the
    # difference to the cost model becomes a per-rank bias (multigpu.rebalance_bias) and every rank re-plans with it and rebuilds its
    # operands; the best plan measured is kept.  No matrix data crosses ranks: the operand of (layer, global batch index) is seeded.
    rebalance_log = []
    if world > 1 and args.scaling == "hybrid" and args.rebalance > 0 and args.emu_rank is None and not f32:
        def gather_us():
            box = [None] * world
            dist.all_gather_object(box, event_seconds(run_full, 5) * 1e6)
            return [float(x) for x in box]

        times = gather_us()
        rebalance_log.append({"round": 0, "rank_us": [round(t, 1) for t in times], "max_over_mean": round(max(times) / (sum(times) / world), 4)})
        best_t, best_bias, cur_bias = max(times), None, None
        for it in range(args.rebalance + 1):
            last = it == args.rebalance
            if last and cur_bias is best_bias:
                break          # the plan in place is the best one measured
            if last:
                nxt = best_bias  # one more re-plan: back to the best plan measured
            else:
                nxt = mg.rebalance_bias(times, mg.plan_loads(shapes, world, "hybrid", rank_bias=cur_bias))
            run_full = step_full = layers = chains = None   # release the operands and the graph of the plan being replaced
            torch.cuda.empty_cache()
            units = mg.plan_units(shapes, world, rank, "hybrid", nxt)
            layers = build_layers(shapes, units)
            flops = mg.unit_flops(shapes, units)
            chains = make_chains(layers)
            step_full, n_launch_groups = assemble(layers)
            run_full = make_runner(step_full)
            cur_bias = nxt
            if last:
                rebalance_log.append({"round": "kept", "bias_us": None if nxt is None else [round(x, 1) for x in nxt]})
                break
            times = gather_us()
            rebalance_log.append({"round": it + 1, "bias_us": [round(x, 1) for x in nxt], "rank_us": [round(t, 1) for t in times],
                                  "max_over_mean": round(max(times) / (sum(times) / world), 4)})
            if max(times) < best_t:
                best_t, best_bias = max(times), nxt
    if args.settle_ms > 0:  # part of the setup, like the buffer fills and the graph capture: not one of the K timed steps
        t_end = time.perf_counter() + args.settle_ms * 1e-3
        while time.perf_counter() < t_end:
            for _ in range(8):
                run_full()
            torch.cuda.synchronize()
    wall = timed(run_full, args.steps, args.warmup)
    tot_flops, wall_max = mg.rollup(flops * args.steps, wall, None if args.rehearse_gloo else dev)
    ms_per_step = wall_max / args.steps * 1e3
    value = tot_flops / wall_max / 1e9
    # --dump-outputs: the C buffers as the last timed step left them, before any later pass (verification, stages) touches them
    dumped = dump_outputs(args.dump_outputs, layers, world) if args.dump_outputs else None

    # BASELINE config 4 in the same run (every rank takes part: the timed loop is bracketed by collectives): the three ResNet tables
    # as 300 whole layers placed by LPT, launched like the step (grouped, over the streams).  north_star's ">= 7x aggregate at 8 GPUs"
    # is stated on this sweep; with it in every N > 1 line the first real SCALE run reports it beside the one-table headline.
    config4 = None
    want_c4 = args.config4_stage == "on" or (args.config4_stage == "auto" and world > 1)
    if want_c4 and grouped and not f32 and args.emu_rank is None:
        shapes4 = [s_ for t in ("resnet50", "resnet101", "resnet152") for s_ in read_shapes(table_path(t))]
        units4 = mg.plan_units(shapes4, world, rank, "lpt")
        layers4 = build_layers(shapes4, units4)
        items4 = [("group", Ls) for _, Ls in fused_groups([L for L in layers4 if use_fused(L)])] + [("single", [L]) for L in layers4 if not use_fused(L)]
        run4 = make_runner(ForkedItems(spread(items4), run_group, layer_path))
        steps4 = max(3, args.steps // 4)
        wall4 = timed(run4, steps4, 2)
        f4, w4 = mg.rollup(mg.unit_flops(shapes4, units4) * steps4, wall4, None if args.rehearse_gloo else dev)
        config4 = {"workload": "datasets/resnet50.csv + resnet101.csv + resnet152.csv: %d layer instances at b = %d, whole layers by LPT over %d rank(s)" % (len(shapes4), shapes4[0][3], world),
                   "partition_mode": "lpt", "layers_this_rank": len(layers4), "steps": steps4, "ms_per_step": w4 / steps4 * 1e3, "value": f4 / w4 / 1e9, "unit": "GF/s",
                   "n_gpus": world, "dense_equiv_gflop_per_step": f4 / steps4 / 1e9,
                   "how": "same process, same ranks, after the headline loop; max over ranks of the wall time, one all-reduce of {flops, seconds}"}
        del layers4, items4, run4

    names = ",".join(os.path.basename(t) for t in tables)
    nfused = sum(use_fused(L) for L in layers)
    sfx = args.dtype
    if f32:
        nsplit = sum(1 for L in layers if L.get("split"))
        path_desc = ("auto: sm_spmma_fused_f32 on %d layers (k %% 32 == 0), sm_compress24_f32 + sm_spmma_f32 on %d" % (nfused, len(layers) - nfused)
                     if args.path == "auto" else "staged: sm_compress24_f32 + sm_spmma_f32 on every layer")
        if nsplit:
            path_desc = ("sm_spmma_fused_f32_split (planes = %d: v_smfmac_f32_16x16x64_bf16 on exact bfloat16 pieces, B split per call) on %d layers; on the other %d: "
                         % (args.f32_planes, nsplit, len(layers) - nsplit)) + path_desc
    elif args.path == "auto":
        path_desc = ("auto: sm_spmma_fused_%s on %d layers (n <= %d or k <= %d), sm_compress24_%s + sm_spmma_%s on %d"
                     % (sfx, nfused, args.fused_max_n, args.fused_max_k_wide, sfx, sfx, len(layers) - nfused))
    else:
        path_desc = "staged: sm_compress24_%s + sm_spmma_%s on every layer" % (sfx, sfx)
    split = {"weak": f"every rank runs all {len(shapes)} layers on its own batch (rank r = global batch indices [r*b, (r+1)*b))",
             "strong": f"batch split: rank g runs batch indices [g*b/{world}, (g+1)*b/{world}) of every layer, B replicated",
             "lpt": f"whole layers by longest-processing-time over {len(shapes)} layer instances",
             "hybrid": f"batch split [g*b/{world}, (g+1)*b/{world}) of the layers whose per-rank share keeps >= {mg.HYBRID_FILL_ROWS} rows, "
                       f"the other layers whole, longest modelled time first (this rank: {len(layers)} units)"}[args.scaling]
    if grouped:
        path_desc += ("; the fused layers run as %d grouped launches (sm_spmma_fused_%s_grouped: one grid per <= 8 same-shape instances, "
                      "same kernels, same C)" % (n_launch_groups, sfx))
    out = {
        "metric": "effective GF/s (2:4 spmma vs dense gemm) on ResNet-50 layer shapes" if "resnet50" in names and not f32 else
                  "effective GF/s (2:4 spmma vs dense gemm) on the layer shapes of " + names.replace(".csv", ""),
        "value": value, "unit": "GF/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak" if args.scaling == "weak" else "strong",
        "partition_mode": args.scaling,  # the real mode name (`scaling` keeps the contract's two values: hybrid / lpt fix the total work = strong)
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": "datasets/%s: %d conv layers as im2col GEMMs (m,n,k) at b=%d, %s; step = per layer "
                               "2:4 prune(STRIP)+compress+matmul of the unpruned A"
                               % (names, len(shapes), shapes[0][3], {"f16": "fp16", "bf16": "bfloat16", "f32": "fp32"}[args.dtype]),
                   "path": path_desc,
                   "layers": len(shapes), "layers_this_rank": len(layers), "batch": shapes[0][3],
                   "dense_equiv_gflop_per_step": tot_flops / args.steps / 1e9,
                   "launch": ("eager" if args.eager else ("hipGraph replay, one linear graph per stream" if args.graphs == "per-stream" else "hipGraph replay of one step"))
                             + (f"; setup runs {args.settle_ms:.0f} ms of untimed replays before the W warm-up steps" if args.settle_ms > 0 else ""),
                   "streams": args.streams, "sched": args.sched, "partition": args.scaling,
                   "library": library_tag(sm),
                   "parallelism": f"{args.scaling} x{world}: {split}; no data-path collective, one all-reduce of "
                                  "{sum flops, max seconds}"},
    }

    # What was timed, checked (not timed): C of one layer per kernel family, as the last timed step left it, against
    # sm_compress24 + sm_spmma on the same operands, bit for bit (the fused kernels' contract; tests/test_gpu_parity.py holds
    # the full matrix of cases).  A mismatch fails the run: a fast step with different results is not a measurement.
    #  a stream-K fix-up that timed out leaves a dirty flag page and an invalid C: every workspace the timed step used is
    # inspected here, after the loop (a 4 KiB read-back each; never inside the timed region)
    for key_, ws_ in sk_ws.items():
        if ws_ is not None and sm.spmma_fused_workspace_state(ws_) != 0:
            sys.stderr.write("bench: stream-K workspace of shape %s is not clean after the timed loop (a fix-up timed out)\n" % (key_,))
            raise SystemExit(4)
    if not f32 and args.path == "auto":
        checked, ok = [], True
        seen = set()
        for L in layers:
            if not use_fused(L):
                continue
            cnt_ = min(8, sum(1 for X in layers if (X["m"], X["n"], X["k"], X["b"]) == (L["m"], L["n"], L["k"], L["b"]))) if args.group == "on" else 1
            fam = fused_variant(L["n"], L["k"], L["m"], L["b"], cnt_)
            if grouped and sk_ws.get((L["m"], L["n"], L["k"], L["b"])) is not None and sk_takes(L, cnt_):
                fam = "sk"
            if fam in seen:
                continue
            seen.add(fam)
            Cref = torch.empty_like(L["C"])
            sm.compress24(L["A"], L["m"], L["k"], L["k"], L["b"], L["m"] * L["k"], L["blob"])
            sm.spmma(L["blob"], L["B"], Cref, L["m"], L["n"], L["k"], L["b"], 0)
            if fam == "thin":
                # the thin form (vector ALUs): the staged pair's products in another order of fp32 additions -- within one rounding of it
                af, bf_ = Cref.float(), L["C"].float()
                rel = float(((af - bf_).abs() / torch.maximum(af.abs(), bf_.abs()).clamp_min(2.0 ** -14)).max().item())
                same = rel <= 2.0 ** -9
                checked.append({"family": fam, "m": L["m"], "n": L["n"], "k": L["k"], "b": L["b"], "max_relative_difference_vs_compress_plus_spmma": rel,
                                "within_one_fp16_rounding": same})
            elif fam == "sk":
                # the stream-K form: the tiles its plan cuts are sums of fp32 partials in a fixed order -- equal to compress + spmma to
                # one fp16 rounding of the result (+ the few fp32 re-associations); every row panel the plan leaves whole: bit for bit
                _, plan = sm.spmma_fused_streamk_plan(L["m"] * L["b"], L["n"], L["k"], cnt_)
                M_, nkt_ = L["m"] * L["b"], L["k"] // 64
                tm_ = (M_ + 255) // 256
                inst = [X for X in layers if (X["m"], X["n"], X["k"], X["b"]) == (L["m"], L["n"], L["k"], L["b"])].index(L) % 8
                whole = [t - inst * tm_ for t in sm.streamk_whole_panels(plan, cnt_ * tm_, nkt_) if inst * tm_ <= t < (inst + 1) * tm_]
                a_, b_ = Cref.view(M_, L["n"]), L["C"].view(M_, L["n"])
                same_whole = all(bool(torch.equal(a_[t * 256:(t + 1) * 256].view(torch.int16), b_[t * 256:(t + 1) * 256].view(torch.int16))) for t in whole)
                af, bf_ = a_.float(), b_.float()
                rel = float(((af - bf_).abs() / torch.maximum(af.abs(), bf_.abs()).clamp_min(2.0 ** -14)).max().item())
                same = same_whole and rel <= 2.0 ** -9   # two neighbouring fp16 values of the larger magnitude differ by at most 2^-10 of it
                checked.append({"family": fam, "m": L["m"], "n": L["n"], "k": L["k"], "b": L["b"], "whole_row_panels": len(whole),
                                "whole_panels_bit_identical_to_compress_plus_spmma": same_whole,
                                "cut_tiles_max_relative_difference": rel, "within_one_fp16_rounding": rel <= 2.0 ** -9})
            else:
                same = bool(torch.equal(Cref.view(torch.int16), L["C"].view(torch.int16)))
                checked.append({"family": fam, "m": L["m"], "n": L["n"], "k": L["k"], "b": L["b"], "bit_identical_to_compress_plus_spmma": same})
            ok = ok and same
            del Cref
        out["verified"] = ok
        out["verified_layers"] = checked
        if not ok:
            sys.stderr.write("bench: the timed step's C differs from compress + spmma: " + json.dumps(checked) + "\n")
            raise SystemExit(4)
    if rebalance_log:
        plan_costs["rebalance_rounds"] = rebalance_log
    out["config"]["plan_costs"] = plan_costs
    if config4 is not None:
        out.setdefault("stages", {})["config4_sweep"] = config4
    if args.emu_rank is not None:
        out["emulated"] = {"world": plan_world, "rank": plan_rank, "units": len(units), "dense_equiv_gflop_per_step": flops / 1e9}
    if dumped is not None:
        out["dump_outputs"] = dumped
    if rank == 0 and not args.no_extras:
        extras(args, sm, torch, dev, layers, flops, wall / args.steps, Forked, make_runner, timed, event_seconds, use_fused, out,
               (fused_groups, run_group, spread, ForkedItems, sk_takes) if grouped else None, step_full)

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(ge, shapes)

    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # Round 6: stdout carries ONE compact contract line (< 4 KB: benchlib.common.contract_line); the whole detail object --
        # `stages` in full, `families`, `yardstick`, `verified_layers`, the per-shape tables: 20 KB in round 5, which the driver
        # could not parse -- goes to a FILE.  --full-line prints the detail object instead (the A/B tools that read it from stdout).
        detail = args.detail or os.path.join(ROOT, "gpurun_out", "bench_detail%s.json" % ("" if args.dtype == "f16" else "_" + args.dtype))
        try:
            os.makedirs(os.path.dirname(os.path.abspath(detail)), exist_ok=True)
            with open(detail, "w") as fh:
                json.dump(out, fh)
            out["detail_file"] = os.path.relpath(detail, ROOT) if os.path.abspath(detail).startswith(ROOT) else detail
        except OSError as e:
            sys.stderr.write(f"bench: detail file not written ({e})\n")
        print(json.dumps(out) if args.full_line else contract_line(out), flush=True)


if __name__ == "__main__":
    main()
