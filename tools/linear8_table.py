#!/usr/bin/env python3
"""tools/linear8_table.py -- the measurement of sm_linear24_fp8: the layers of datasets/linear_shapes.csv at
tokens in {1, 8, 16, 32, 64, 128, 512, 2048, 8192}, e4m3 x e4m3, bf16 out, both scales given; ms per call by hipGraph replay
(graph_time_ms: 20 calls per graph, 3 replays), five interleaved repeats, median [min .. max] per column.

  t_linear8   sm_linear24_fp8 of this build
  t_route     what a caller ran before for the same fp8 X -> token-major Y: sm_spmma_fp8 (C[out][tokens] bf16, row_scale = w_scale) +
              sm_transpose of the output, on the library given by --lib (a build of the parent commit; default: this build, whose
              two kernels are the same objects); the per-token scale has nowhere to go in the route and is left out of it
  t_linear16  sm_linear24_bf16 on the same shape (bf16 blob of the same weight, bf16 tokens), --lib build
  t_dense8    the dense denominator: sm_gemm_rowmajor_fp8(A = X, B = W as [out][in]: Y[tokens][out] directly), --lib build
  t_tile / t_decode  (tokens <= 64, with --tile / --decode) sm_linear24_fp8 of two other builds whose dispatch constants were edited
              to take the tile form always / the decode form up to 64 tokens (the form table, profiles/linear8_forms.txt)
  bytes = 0.625 * out * in + tokens * in + 2 * tokens * out over t_linear8 as a share of 8 TB/s; 16/8 = t_linear16 / t_linear8 beside
  the 1.8 x byte ceiling of the weight stream (1.125 / 0.625).

The buffers of a cell are reused by every replay, so a layer whose operands fit the 256 MB Infinity Cache is timed warm, in all
columns alike.

  python tools/linear8_table.py [--lib LIB] [--tile LIB --decode LIB] [--tokens 1,8,16] > profiles/linear8_table.txt

Kernel stats (profiles/linear8_kernel_stats.csv) come from a run of their own, the table under the profiler with one repeat:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/linear8_table.py --repeats 1 [--lib LIB]
"""
import argparse
import csv
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKENS = [1, 8, 16, 32, 64, 128, 512, 2048, 8192]
REPEATS = 5
E4M3, OUT_BF16 = 0, 2


def load(pkg, path, names):
    L = ctypes.CDLL(os.path.abspath(path))
    for n in names:
        fn = getattr(L, n)
        fn.argtypes, fn.restype = pkg._SIGS[n], ctypes.c_int
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the libsparsifyme.so that runs t_route, t_linear16 and t_dense8 (default: the in-tree build)")
    ap.add_argument("--tile", help="a build that always takes the tile form (extra column t_tile)")
    ap.add_argument("--decode", help="a build that takes the decode form up to 64 tokens (extra column t_decode)")
    ap.add_argument("--tokens", default=",".join(map(str, TOKENS)))
    ap.add_argument("--repeats", type=int, default=REPEATS, help="interleaved repeats per cell (1 for the kernel-stats run)")
    ap.add_argument("--shapes", default=os.path.join(ROOT, "datasets", "linear_shapes.csv"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = torch.device("cuda:0")
    P = load(pkg, a.lib or pkg.LIB_PATH, ["sm_transpose", "sm_spmma_fp8", "sm_linear24_bf16", "sm_gemm_rowmajor_fp8"])
    forced = {k: load(pkg, p, ["sm_linear24_fp8"]) for k, p in (("t_tile", a.tile), ("t_decode", a.decode)) if p}
    lines = open(a.shapes).read().splitlines()
    shapes = [(int(r["out"]), int(r["in"])) for r in csv.DictReader(l for l in lines if not l.startswith("#"))]
    tokens_list = [int(t) for t in a.tokens.split(",")]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    f8 = torch.float8_e4m3fn

    def ok(rc):
        assert rc == 0, rc

    print(f"# {pkg.version()}; ms per call, median [min .. max] of {a.repeats} interleaved repeats (graph replay, 20 calls x 3 replays)")
    sums = {}
    for out, inf in shapes:
        g = torch.Generator(device=dev).manual_seed(out + inf)
        W = (torch.rand(out, inf, generator=g, device=dev) - 0.5).bfloat16()
        blob8 = torch.empty(pkg.compress24_size(out, inf, 1, 1), dtype=torch.uint8, device=dev)
        ws = torch.empty(out, dtype=torch.float32, device=dev)
        pkg.quantize_compress24_fp8(W, blob8, ws, out, inf, f8)
        W8 = torch.empty(out, inf, dtype=f8, device=dev)       # the dense fp8 weight of the dense denominator: the pruned, quantised W
        pkg.decompress24_fp8(blob8, out, inf, inf, 1, out * inf, W8)
        pkg.prune24(W, W, out, inf, inf, pkg.PRUNE_STRIP)
        blob16 = torch.empty(pkg.compress24_size(out, inf, 2, 1), dtype=torch.uint8, device=dev)
        pkg.compress24(W, out, inf, inf, 1, out * inf, blob16)
        for tokens in tokens_list:
            X = (torch.rand(tokens, inf, generator=g, device=dev) - 0.5).bfloat16()
            Q = torch.empty(tokens, inf, dtype=f8, device=dev)
            xs = torch.empty(tokens, dtype=torch.float32, device=dev)
            pkg.quantize_rows_fp8(X, Q, xs, tokens, inf)
            Y = torch.empty(tokens, out, dtype=torch.bfloat16, device=dev)
            C = torch.empty(out, tokens, dtype=torch.bfloat16, device=dev)
            Yr = torch.empty(tokens, out, dtype=torch.bfloat16, device=dev)
            Y16 = torch.empty(tokens, out, dtype=torch.bfloat16, device=dev)
            Yd = torch.empty(tokens, out, dtype=torch.bfloat16, device=dev)
            st = pkg._stream

            def route():
                ok(P.sm_spmma_fp8(ptr(blob8), ptr(Q), ptr(C), out, tokens, inf, 1, 0, out * tokens, E4M3, E4M3, OUT_BF16, 1.0, 0.0, ptr(ws), st()))
                ok(P.sm_transpose(ptr(C), ptr(Yr), out, tokens, tokens, out, 2, 1, 0, 0, st()))

            cols = {
                "t_linear8": lambda: pkg.linear24_fp8(blob8, Q, Y, tokens, out, inf, w_scale=ws, x_scale=xs),
                "t_route": route,
                "t_linear16": lambda: ok(P.sm_linear24_bf16(ptr(blob16), ptr(X), ptr(Y16), tokens, out, inf, inf, out, 1.0, 0.0, None, st())),
                "t_dense8": lambda: ok(P.sm_gemm_rowmajor_fp8(ptr(Q), ptr(W8), ptr(Yd), tokens, out, inf, inf, 1, tokens * inf, 0, tokens * out,
                                                              E4M3, E4M3, OUT_BF16, 1.0, 0.0, None, st())),
            }
            if tokens <= 64:
                for k, L in forced.items():
                    cols[k] = (lambda L: lambda: ok(L.sm_linear24_fp8(ptr(blob8), ptr(Q), ptr(Y), tokens, out, inf, inf, out, E4M3, E4M3, OUT_BF16, 1.0, 0.0,
                                                                      ptr(ws), ptr(xs), None, st())))(L)
            t = {k: [] for k in cols}
            for _ in range(a.repeats):
                for k, fn in cols.items():
                    t[k].append(pkg.graph_time_ms(fn))
            torch.cuda.synchronize()
            med = {k: statistics.median(v) for k, v in t.items()}
            cell = "  ".join(f"{k} {med[k]:.4f} [{min(v):.4f} .. {max(v):.4f}]" for k, v in t.items())
            byts = 0.625 * out * inf + tokens * inf + 2 * tokens * out
            extra = f"  bytes/8TBs {byts / (med['t_linear8'] * 1e-3) / 8e12:.3f}  16/8 {med['t_linear16'] / med['t_linear8']:.3f} (ceiling 1.8)"
            a_ = "met" if med["t_linear8"] <= med["t_route"] else ("tie" if med["t_linear8"] <= max(t["t_route"]) else "MISSED")
            b_ = "" if tokens > 16 else ("  (b) met" if med["t_linear8"] <= med["t_linear16"] else "  (b) MISSED")
            print(f"{out}x{inf} tokens {tokens} [{pkg.linear24_fp8_form(tokens, out, inf)}]: {cell}{extra}  dense8/linear8 {med['t_dense8'] / med['t_linear8']:.3f}"
                  f"  (a) {a_}{b_}", flush=True)
            s = sums.setdefault(tokens, {})
            for k in med:
                s[k] = s.get(k, 0.0) + med[k]
            del X, Q, Y, C, Yr, Y16, Yd
        del W, W8, blob8, blob16
    print("# summed over the table, per tokens")
    for tokens, s in sums.items():
        print(f"sum tokens {tokens}: " + "  ".join(f"{k} {v:.4f}" for k, v in s.items())
              + f"  route/linear8 {s['t_route'] / s['t_linear8']:.3f}  linear16/linear8 {s['t_linear16'] / s['t_linear8']:.3f}"
              + f"  dense8/linear8 {s['t_dense8'] / s['t_linear8']:.3f}", flush=True)


if __name__ == "__main__":
    main()
