#!/usr/bin/env python3
"""tools/linear_table.py -- the measurement of sm_linear24_f16: the layers of datasets/linear_shapes.csv at
tokens in {1, 8, 16, 32, 64, 128, 512, 2048, 8192}, fp16, ms per call by hipGraph replay (graph_time_ms: 20 calls per graph, 3
replays), five interleaved repeats, median [min .. max] per column.

  t_linear  sm_linear24_f16 of this build
  t_route   what a caller ran before for the same X -> Y: sm_transpose + sm_spmma_f16 + sm_transpose, on the library given by
            --lib (a build of the commit before sm_linear24 existed; default: this build, whose three kernels are the same
            code); same process, interleaved
  t_dense   the library's own dense denominator: sm_gemm_rowmajor_f16(A = X, B = W^T stored [in][out] once), --lib build
  t_vendor  torch.nn.functional.linear on the dense pruned W (a yardstick, reported only)
  t_tile / t_decode  (tokens <= 64, with --tile / --decode) sm_linear24_f16 of two other builds of the library: for the form
            threshold of DESIGN.md 4.13 these were builds whose dispatch constants were edited to take the tile form always / the
            decode form up to 64 tokens (the latter with the decode kernel also instantiated for 32 and 64 tokens)
  bytes = 0.5625 * 2 * out * in + 2 * tokens * (in + out) over t_linear as a share of 8 TB/s; flops = 2 * tokens * out * in over
  t_linear as a share of 5 PF/s (the dense fp16 rate the 2:4 instruction doubles), printed for tokens >= 512.

The buffers of a cell are reused by every replay, so a layer whose operands fit the 256 MB Infinity Cache is timed warm, in all
columns alike.

  python tools/linear_table.py [--lib LIB] [--tile LIB --decode LIB] [--tokens 1,8,16] > profiles/linear_table.txt
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


def load(pkg, path, names):
    L = ctypes.CDLL(os.path.abspath(path))
    for n in names:
        fn = getattr(L, n)
        fn.argtypes, fn.restype = pkg._SIGS[n], ctypes.c_int
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the libsparsifyme.so that runs t_route and t_dense (default: the in-tree build)")
    ap.add_argument("--tile", help="a build that always takes the tile form (extra column t_tile)")
    ap.add_argument("--decode", help="a build that takes the decode form up to 64 tokens (extra column t_decode)")
    ap.add_argument("--tokens", default=",".join(map(str, TOKENS)))
    ap.add_argument("--shapes", default=os.path.join(ROOT, "datasets", "linear_shapes.csv"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = torch.device("cuda:0")
    P = load(pkg, a.lib or pkg.LIB_PATH, ["sm_transpose", "sm_spmma_f16", "sm_gemm_rowmajor_f16"])
    forced = {k: load(pkg, p, ["sm_linear24_f16"]) for k, p in (("t_tile", a.tile), ("t_decode", a.decode)) if p}
    lines = open(a.shapes).read().splitlines()
    shapes = [(int(r["out"]), int(r["in"])) for r in csv.DictReader(l for l in lines if not l.startswith("#"))]
    tokens_list = [int(t) for t in a.tokens.split(",")]
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())

    def ok(rc):
        assert rc == 0, rc

    print(f"# {pkg.version()}; ms per call, median [min .. max] of {REPEATS} interleaved repeats (graph replay, 20 calls x 3 replays)")
    sums = {}
    for out, inf in shapes:
        g = torch.Generator(device=dev).manual_seed(out + inf)
        W = (torch.rand(out, inf, generator=g, device=dev) - 0.5).half()
        pkg.prune24(W, W, out, inf, inf, pkg.PRUNE_STRIP)
        blob = torch.empty(pkg.compress24_size(out, inf, 2, 1), dtype=torch.uint8, device=dev)
        pkg.compress24(W, out, inf, inf, 1, out * inf, blob)
        Wt = W.t().contiguous()
        for tokens in tokens_list:
            X = (torch.rand(tokens, inf, generator=g, device=dev) - 0.5).half()
            Y = torch.empty(tokens, out, dtype=torch.float16, device=dev)
            Xt = torch.empty(inf, tokens, dtype=torch.float16, device=dev)
            C = torch.empty(out, tokens, dtype=torch.float16, device=dev)
            Yr = torch.empty(tokens, out, dtype=torch.float16, device=dev)
            Yd = torch.empty(tokens, out, dtype=torch.float16, device=dev)
            st = pkg._stream

            def route():
                ok(P.sm_transpose(ptr(X), ptr(Xt), tokens, inf, inf, tokens, 2, 1, 0, 0, st()))
                ok(P.sm_spmma_f16(ptr(blob), ptr(Xt), ptr(C), out, tokens, inf, 1, 0, out * tokens, 1.0, 0.0, st()))
                ok(P.sm_transpose(ptr(C), ptr(Yr), out, tokens, tokens, out, 2, 1, 0, 0, st()))

            cols = {
                "t_linear": lambda: pkg.linear24(blob, X, Y, tokens, out, inf),
                "t_route": route,
                "t_dense": lambda: ok(P.sm_gemm_rowmajor_f16(ptr(X), ptr(Wt), ptr(Yd), tokens, out, inf, inf, 1, tokens * inf, 0, tokens * out, 1.0, 0.0, st())),
                "t_vendor": lambda: torch.nn.functional.linear(X, W),
            }
            if tokens <= 64:
                for k, L in forced.items():
                    cols[k] = (lambda L: lambda: ok(L.sm_linear24_f16(ptr(blob), ptr(X), ptr(Y), tokens, out, inf, inf, out, 1.0, 0.0, None, st())))(L)
            t = {k: [] for k in cols}
            for _ in range(REPEATS):
                for k, fn in cols.items():
                    t[k].append(pkg.graph_time_ms(fn))
            # the same seeded inputs give the route's result (bit for bit in the tile form)
            torch.cuda.synchronize()
            same = torch.equal(Y.view(torch.int16), Yr.view(torch.int16)) if "t_tile" not in cols and tokens > 16 else None
            med = {k: statistics.median(v) for k, v in t.items()}
            cell = "  ".join(f"{k} {med[k]:.4f} [{min(v):.4f} .. {max(v):.4f}]" for k, v in t.items())
            byts = 0.5625 * 2 * out * inf + 2 * tokens * (inf + out)
            extra = f"  bytes/8TBs {byts / (med['t_linear'] * 1e-3) / 8e12:.3f}"
            if tokens >= 512:
                extra += f"  flops/5PFs {2.0 * tokens * out * inf / (med['t_linear'] * 1e-3) / 5e15:.3f}"
            line1 = "met" if med["t_linear"] <= min(t["t_route"]) else ("within spread" if med["t_linear"] <= max(t["t_route"]) else "MISSED")
            print(f"{out}x{inf} tokens {tokens}: {cell}{extra}  dense/linear {med['t_dense'] / med['t_linear']:.3f}  line1 {line1}"
                  + ("" if same is None else f"  ==route {'yes' if same else 'NO'}"), flush=True)
            s = sums.setdefault(tokens, {})
            for k in med:
                s[k] = s.get(k, 0.0) + med[k]
            del X, Y, Xt, C, Yr, Yd
        del W, Wt, blob
    print("# summed over the table, per tokens")
    for tokens, s in sums.items():
        print(f"sum tokens {tokens}: " + "  ".join(f"{k} {v:.4f}" for k, v in s.items())
              + f"  dense/linear {s['t_dense'] / s['t_linear']:.3f}  route/linear {s['t_route'] / s['t_linear']:.3f}", flush=True)


if __name__ == "__main__":
    main()
