#!/usr/bin/env python3
"""tools/attn_decode_table.py -- sm_attn_decode_bf16 against the framework route it replaces: us per call over
datasets/attn_shapes.csv at contexts 1024, 4096, 16384 and 32768 and batches 1, 8 and 64 (cells whose cache exceeds half the device memory
are skipped); bf16; every sequence holds the full context, pages scattered by a random permutation.

  call    one sm_attn_decode_bf16 call (one launch in the direct form, two in the split form).
  torch   the route a caller has today: index_select of the table's pages into a contiguous K / V, then scaled_dot_product_attention with the
          group expanded (sdpa) or matmul / softmax / matmul on the grouped shape (mm); the faster of the two is the route's time.
  sdpa0   scaled_dot_product_attention alone on an already contiguous, already expanded cache: the route's floor.
  copy    a torch copy that moves the call's algorithmic bytes -- the live K and V rows once -- in the same process: the call is reported as
          a multiple of it and as a fraction of 8 TB/s.
The graph and the eager clock of tools/tablelib.py, median of five; N is 20, fewer where a call moves more than 256 MB.
Expectation, stated before the run: no cell is behind the torch route, and at batch >= 8 and context >= 4096 the call is within a small factor
of the copy.  Nothing is required of the numbers: the table is the finding.

--part chunk: the run SM_ATTN_DECODE_CHUNK is chosen from -- the attn_decode translation unit alone built at 128, 256 and 512
(tools/probes/attn_decode_forced.hip), the batch-1 and batch-64 columns, graph clock.

  python tools/attn_decode_table.py > profiles/attn_decode_table.txt
"""
import argparse
import ctypes
import os
import sys

from tablelib import CALLS, REPEATS, REPLAYS, attn_shapes as shapes, clocks, medians, paged_cache, probe_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTEXTS = [1024, 4096, 16384, 32768]
BATCHES = [1, 8, 64]
CHUNKS = [128, 256, 512]


def forced_lib(chunk):
    """tools/probes/libattn_decode_c<chunk>.so: attn_decode.hip alone with the chunk forced; built when it is not there"""
    L = probe_lib(f"attn_decode_c{chunk}", "attn_decode_forced.hip", f"ATTN_DECODE_CHUNK={chunk}")
    L.sm_attn_decode_bf16.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_size_t] * 13 + [ctypes.c_float, ctypes.c_void_p]
    L.sm_attn_decode_bf16.restype = ctypes.c_int
    L.sm_attn_decode_workspace_size.argtypes = [ctypes.c_size_t] * 5 + [ctypes.POINTER(ctypes.c_size_t)]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["table", "chunk", "all"], default="all")
    ap.add_argument("--build-only", action="store_true", help="build the forced-chunk libraries and leave (no device needed)")
    args = ap.parse_args()
    if args.build_only:
        for c in CHUNKS:
            forced_lib(c)
        return
    import torch
    import torch.nn.functional as F
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = "cuda:0"
    half_mem = torch.cuda.get_device_properties(0).total_memory // 2

    def operands(batch, ctx, qh, kvh, hd, ps):
        gen = torch.Generator(device=dev).manual_seed(batch * 131 + ctx)
        max_pages = ctx // ps
        q = torch.randn((batch, qh, hd), generator=gen, device=dev, dtype=torch.bfloat16)
        K, V, bt = paged_cache(gen, dev, batch, max_pages, ps, kvh, hd, normal=True)
        o = dict(q=q, K=K, V=V, bt=bt, sl=torch.full((batch,), ctx, dtype=torch.int32, device=dev), out=torch.empty((batch, qh, hd), device=dev, dtype=torch.bfloat16))
        need = pkg.attn_decode_workspace_size(batch, qh, hd, ps, max_pages)
        o["ws"] = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        return o

    def one_cell(cell, moved, batch, ctx, qh, kvh, hd, ps, G, behind):
        calls = CALLS if moved <= (256 << 20) else max(2, int(CALLS * (256 << 20) / moved))
        o = operands(batch, ctx, qh, kvh, hd, ps)
        scale = hd ** -0.5
        idx = o["bt"].flatten().long()
        call = lambda: pkg.attn_decode(o["q"], o["K"], o["V"], o["bt"], o["sl"], out=o["out"], workspace=o["ws"])
        def gather():
            Kc = o["K"].index_select(0, idx).view(batch, ctx, kvh, hd).transpose(1, 2)          # [batch][kvh][ctx][hd]
            Vc = o["V"].index_select(0, idx).view(batch, ctx, kvh, hd).transpose(1, 2)
            return Kc, Vc
        def expand(x):
            return x if G == 1 else x[:, :, None].expand(batch, kvh, G, ctx, hd).reshape(batch, qh, ctx, hd)
        def route_sdpa():
            Kc, Vc = gather()
            return F.scaled_dot_product_attention(o["q"][:, :, None, :], expand(Kc), expand(Vc))
        def route_mm():
            Kc, Vc = gather()
            s = torch.matmul(o["q"].view(batch, kvh, G, hd), Kc.transpose(-1, -2)) * scale
            return torch.matmul(torch.softmax(s.float(), dim=-1).to(torch.bfloat16), Vc)
        Ke, Ve = (expand(x).contiguous() for x in gather())
        floor = lambda: F.scaled_dot_product_attention(o["q"][:, :, None, :], Ke, Ve)
        src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        cols = {}
        cols["call graph"], cols["call eager"] = clocks(call, calls)
        cols["sdpa graph"], cols["sdpa eager"] = clocks(route_sdpa, calls)
        cols["mm graph"], cols["mm eager"] = clocks(route_mm, calls)
        cols["sdpa0 graph"], _ = clocks(floor, calls)
        cols["copy graph"], _ = clocks(lambda: dst.copy_(src), calls)
        med, runs = medians(cols)
        text = "  ".join(f"{k} {med[k]:.1f} [{min(runs[k]):.1f} .. {max(runs[k]):.1f}]" for k in cols)
        tg, te = min(med["sdpa graph"], med["mm graph"]), min(med["sdpa eager"], med["mm eager"])
        rg, re_ = tg / med["call graph"], te / med["call eager"]
        form = pkg.attn_decode_form(batch, qh, kvh, hd, ps, ctx // ps)
        print(f"{cell} [{form}, N {calls}]: {text}  torch/call graph {rg:.2f} eager {re_:.2f}  call/copy {med['call graph'] / med['copy graph']:.2f} "
              f"({moved / med['call graph'] / 1e6:.2f} TB/s of algorithmic bytes, {moved / med['call graph'] / 8e6:.3f} of 8 TB/s)", flush=True)
        for clock, r in (("graph", rg), ("eager", re_)):
            if r < 1.0:
                behind.append(f"{cell} {clock} {r:.2f}")

    if args.part in ("table", "all"):
        print(f"# {pkg.version()}; bf16; us per call, median of {REPEATS} alternated repeats (graph: N calls x {REPLAYS} replays; eager: N calls, launch gaps "
              f"included; N = {CALLS}, fewer above 256 MB per call); SM_ATTN_DECODE_CHUNK {pkg.ATTN_DECODE_CHUNK}")
        behind = []
        for qh, kvh, hd, ps in shapes():
            G = qh // kvh
            for ctx in CONTEXTS:
                for batch in BATCHES:
                    moved = 2 * batch * ctx * kvh * hd * 2                 # the live K and V rows once
                    cell = f"q_heads {qh} kv_heads {kvh} head_dim {hd} page {ps} context {ctx} batch {batch}"
                    if moved > half_mem:
                        print(f"{cell}: skipped, the cache ({moved / 2 ** 30:.1f} GiB) exceeds half the device memory", flush=True)
                        continue
                    try:
                        one_cell(cell, moved, batch, ctx, qh, kvh, hd, ps, G, behind)
                    except torch.OutOfMemoryError:
                        print(f"{cell}: skipped, the torch route ran out of device memory", flush=True)
                    torch.cuda.empty_cache()
        print("# cells where the call is behind the torch route: " + ("none" if not behind else ""))
        for b in behind:
            print("behind: " + b)

    if args.part in ("chunk", "all"):
        print(f"# SM_ATTN_DECODE_CHUNK: the translation unit alone at {CHUNKS} on the batch-1 and batch-64 columns (graph clock, us per call, median of {REPEATS})")
        libs = {c: forced_lib(c) for c in CHUNKS}
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        for qh, kvh, hd, ps in shapes():
            for ctx in CONTEXTS:
                for batch in (1, 64):
                    moved = 2 * batch * ctx * kvh * hd * 2
                    if moved > half_mem:
                        continue
                    calls = CALLS if moved <= (256 << 20) else max(2, int(CALLS * (256 << 20) / moved))
                    o = operands(batch, ctx, qh, kvh, hd, ps)
                    max_pages = ctx // ps
                    ws = torch.empty(batch * qh * (ctx // min(CHUNKS)) * (hd + 2) * 4 + 16, dtype=torch.uint8, device=dev)     # enough for every chunk

                    def forced(L):
                        def fn():
                            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                            rc = L.sm_attn_decode_bf16(ptr(o["q"]), ptr(o["K"]), ptr(o["V"]), ptr(o["bt"]), ptr(o["sl"]), ptr(o["out"]), None, ptr(ws), ws.numel(),
                                                       batch, qh, kvh, hd, batch * max_pages, ps, max_pages, qh * hd, kvh * hd, ps * kvh * hd, max_pages, qh * hd,
                                                       hd ** -0.5, st)
                            assert rc == 0, rc
                        return fn
                    cols = {f"chunk {c}": clocks(forced(L), calls)[0] for c, L in libs.items()}
                    med, runs = medians(cols)
                    text = "  ".join(f"{k} {med[k]:.1f} [{min(runs[k]):.1f} .. {max(runs[k]):.1f}]" for k in cols)
                    best = min(med, key=med.get)
                    print(f"forced q_heads {qh} kv_heads {kvh} head_dim {hd} context {ctx} batch {batch}: {text}  best {best}", flush=True)
                    del o, ws
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
