#!/usr/bin/env python3
"""tools/rmsnorm_table.py -- sm_rmsnorm_bf16 against the framework ops it replaces: us per call at 16, 128, 1024 and 8192
tokens; hidden 128 with tokens * 32 rows (the per-head norm), 4096 and 8192; bf16; three variants.

  norm          n = rmsnorm(H) * gamma -> N
  add+norm      h = H + D -> res_out, n -> N
  add+norm+e4m3 h -> res_out, n quantised per row -> Q, row_scale (no 16-bit N: what the W8A8 layers read)
  call    one sm_rmsnorm_bf16 launch.
  torch   the torch spelling: add, fp32 pow / mean / rsqrt / mul / mul, cast; for the third variant sm_quantize_rows_fp8_bf16 on top.
  copy    a torch copy that moves the call's algorithmic bytes (reads + writes), in the same process: the call is reported as a multiple
          of it, not against a fixed TB/s.
The graph and the eager clock of tools/tablelib.py per side, 20 calls each, median of five.
Expectation, stated before the run: one launch against five to eight is ahead in every cell, and at 8192 tokens the call sits within a
small factor of the copy of its own bytes.  Nothing is required of the numbers: the table is the finding.

Behind the cells, the run SM_RMSNORM_LANES_MAX_HIDDEN is chosen from: both forms forced on the same shapes, hidden 256 .. 4608, from two
builds of the rmsnorm translation unit alone (tools/probes/rmsnorm_forced.hip, the threshold at 4608 and at 8), graph clock.

  python tools/rmsnorm_table.py > profiles/rmsnorm_table.txt
"""
import ctypes
import os
import sys

from tablelib import CALLS, REPEATS, REPLAYS, clocks, medians, probe_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKENS = [16, 128, 1024, 8192]
HIDDENS = [128, 4096, 8192]
VARIANTS = ["norm", "add+norm", "add+norm+e4m3"]
FORCED_HIDDENS = [256, 512, 768, 1024, 1536, 2048, 2560, 3072, 4096, 4608]
FORCED_TOKENS = [16, 1024, 8192]
EPS = 1e-6


def forced_lib(name, lanes_max):
    """tools/probes/librmsnorm_<name>.so: rmsnorm.hip alone with the threshold forced; built when it is not there"""
    L = probe_lib(f"rmsnorm_{name}", "rmsnorm_forced.hip", f"RMSNORM_LANES_MAX={lanes_max}")
    L.sm_rmsnorm_bf16.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_size_t] * 6 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    L.sm_rmsnorm_bf16.restype = ctypes.c_int
    return L


def main():
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = "cuda:0"
    f8 = torch.float8_e4m3fn

    def operands(rows, hidden):
        gen = torch.Generator().manual_seed(rows * 131 + hidden)
        mk = lambda *shape: torch.randn(*shape, generator=gen).to(torch.bfloat16).to(dev)
        o = dict(H=mk(rows, hidden), D=mk(rows, hidden), g=(1.0 + 0.3 * torch.randn(hidden, generator=gen)).to(torch.bfloat16).to(dev))
        o["res"], o["N"] = torch.empty_like(o["H"]), torch.empty_like(o["H"])
        o["Q"] = torch.empty((rows, hidden), dtype=torch.uint8, device=dev).view(f8)
        o["rs"] = torch.empty(rows, dtype=torch.float32, device=dev)
        return o

    def torch_norm(h, g):
        x = h.float()
        return (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS) * g.float()).to(torch.bfloat16)

    print(f"# {pkg.version()}; bf16; us per call, median of {REPEATS} alternated repeats (graph: {CALLS} calls x {REPLAYS} replays; eager: {CALLS} calls, "
          f"launch gaps included); SM_RMSNORM_LANES_MAX_HIDDEN {pkg.RMSNORM_LANES_MAX_HIDDEN}")
    behind = []
    for hidden in HIDDENS:
        for tokens in TOKENS:
            rows = tokens * 32 if hidden == 128 else tokens
            o = operands(rows, hidden)
            for variant in VARIANTS:
                if variant == "norm":
                    call = lambda: pkg.rmsnorm(o["H"], gamma=o["g"], eps=EPS, out=o["N"])
                    ops = lambda: torch_norm(o["H"], o["g"])
                    moved = 2 * rows * hidden * 2
                elif variant == "add+norm":
                    call = lambda: pkg.rmsnorm(o["H"], delta=o["D"], gamma=o["g"], eps=EPS, out=o["N"], res_out=o["res"])
                    ops = lambda: torch_norm(o["H"] + o["D"], o["g"])
                    moved = 4 * rows * hidden * 2
                else:
                    call = lambda: pkg.rmsnorm(o["H"], delta=o["D"], gamma=o["g"], eps=EPS, res_out=o["res"], fp8=(o["Q"], o["rs"]))

                    def ops():
                        n = torch_norm(o["H"] + o["D"], o["g"])
                        pkg.quantize_rows_fp8(n, o["Q"], o["rs"], rows, hidden)
                    moved = 3 * rows * hidden * 2 + rows * hidden + rows * 4
                src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                cols = {}
                cols["call graph"], cols["call eager"] = clocks(call)
                cols["torch graph"], cols["torch eager"] = clocks(ops)
                cols["copy graph"], _ = clocks(lambda: dst.copy_(src))
                med, runs = medians(cols)
                cell = f"hidden {hidden} rows {rows} (tokens {tokens}) {variant} [{pkg.rmsnorm_form(hidden)}]"
                text = "  ".join(f"{k} {med[k]:.1f} [{min(runs[k]):.1f} .. {max(runs[k]):.1f}]" for k in cols)
                rg, re_ = med["torch graph"] / med["call graph"], med["torch eager"] / med["call eager"]
                print(f"{cell}: {text}  torch/call graph {rg:.2f} eager {re_:.2f}  call/copy {med['call graph'] / med['copy graph']:.2f} "
                      f"({moved / med['call graph'] / 1e6:.2f} TB/s of algorithmic bytes)", flush=True)
                for clock, r in (("graph", rg), ("eager", re_)):
                    if r < 1.0:
                        behind.append(f"{cell} {clock} {r:.2f}")
                del src, dst
            del o
            torch.cuda.empty_cache()
    print("# cells where the call is behind the torch ops: " + ("none" if not behind else ""))
    for b in behind:
        print("behind: " + b)

    print(f"# LANES against BLOCK forced on the same shapes (graph clock, us per call, median of {REPEATS}): what SM_RMSNORM_LANES_MAX_HIDDEN is chosen from")
    forms = {"lanes": forced_lib("lanes", 4608), "block": forced_lib("block", 8)}
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    for hidden in FORCED_HIDDENS:
        for tokens in FORCED_TOKENS:
            o = operands(tokens, hidden)
            for variant in ("add+norm", "add+norm+e4m3"):
                quant = variant.endswith("e4m3")

                def forced(L):
                    def fn():
                        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                        rc = L.sm_rmsnorm_bf16(ptr(o["H"]), ptr(o["D"]), ptr(o["g"]), ptr(o["res"]), None if quant else ptr(o["N"]), ptr(o["Q"]) if quant else None,
                                               ptr(o["rs"]) if quant else None, tokens, hidden, hidden, hidden, hidden, hidden, EPS, pkg.FP8_E4M3, st)
                        assert rc == 0, rc
                    return fn
                cols = {name: clocks(forced(L))[0] for name, L in forms.items()}
                med, runs = medians(cols)
                text = "  ".join(f"{k} {med[k]:.1f} [{min(runs[k]):.1f} .. {max(runs[k]):.1f}]" for k in cols)
                print(f"forced hidden {hidden} tokens {tokens} {variant}: {text}  block/lanes {med['block'] / med['lanes']:.2f}", flush=True)
            del o


if __name__ == "__main__":
    main()
