#!/usr/bin/env python3
"""tools/linear_glu_table.py -- the measurement of the gated layers sm_linear24_glu_* (DESIGN.md 4.15): the two gate/up rows of
datasets/linear_shapes.csv (hidden 14336 and 11008, in 4096) at tokens in {1, 8, 16, 32, 64, 128, 512, 2048, 8192}, in bf16 and in
fp8 (e4m3 x e4m3, bf16 out, both scales given); ms per call by hipGraph replay (graph_time_ms: 20 calls per graph, 3 replays), five
interleaved repeats, median [min .. max] per column, all columns in one run on warm buffers (a cell's buffers are reused by every
replay, so operands that fit the 256 MB Infinity Cache are timed warm, in all columns alike).

  t_glu     sm_linear24_glu_* : Y[tokens][hidden] = silu(gate) * up in one launch
  t_linear  the plain sm_linear24_* on the same blob, out = 2 * hidden: Y[tokens][2 hidden] -- the parent's code and the yardstick: the
            gated call does the same products and stores half the bytes, so t_glu <= t_linear is expected on every cell.  A cell whose
            t_glu median lies above t_linear's max is reported NOT MET.
  t_route   t_linear plus what a caller ran after it: torch.nn.functional.silu(y[:, :h]) * y[:, h:]

  python tools/linear_glu_table.py [--tokens 1,8,16] > profiles/linear_glu_table.txt

Kernel stats (profiles/linear_glu_kernel_stats.csv) come from a run of their own, the table under the profiler with one repeat:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/linear_glu_table.py --repeats 1
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKENS = [1, 8, 16, 32, 64, 128, 512, 2048, 8192]
HIDDEN = [(14336, 4096), (11008, 4096)]   # the fused gate/up rows 28672 x 4096 and 22016 x 4096 of datasets/linear_shapes.csv
REPEATS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default=",".join(map(str, TOKENS)))
    ap.add_argument("--repeats", type=int, default=REPEATS, help="interleaved repeats per cell (1 for the kernel-stats run)")
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = torch.device("cuda:0")
    tokens_list = [int(t) for t in a.tokens.split(",")]
    f8 = torch.float8_e4m3fn
    table = open(os.path.join(ROOT, "datasets", "linear_shapes.csv")).read()
    for hidden, inf in HIDDEN:
        assert f"{2 * hidden},{inf}" in table.replace(" ", ""), "the gate/up rows are those of datasets/linear_shapes.csv"

    print(f"# {pkg.version()}; ms per call, median [min .. max] of {a.repeats} interleaved repeats (graph replay, 20 calls x 3 replays)")
    sums, missed = {}, []
    for hidden, inf in HIDDEN:
        out = 2 * hidden
        g = torch.Generator(device=dev).manual_seed(out + inf)
        W = (torch.rand(out, inf, generator=g, device=dev) - 0.5).bfloat16()
        blob8 = torch.empty(pkg.compress24_size(out, inf, 1, 1), dtype=torch.uint8, device=dev)
        ws = torch.empty(out, dtype=torch.float32, device=dev)
        pkg.quantize_compress24_fp8(W, blob8, ws, out, inf, f8)
        pkg.prune24(W, W, out, inf, inf, pkg.PRUNE_STRIP)
        blob16 = torch.empty(pkg.compress24_size(out, inf, 2, 1), dtype=torch.uint8, device=dev)
        pkg.compress24(W, out, inf, inf, 1, out * inf, blob16)
        for tokens in tokens_list:
            X = (torch.rand(tokens, inf, generator=g, device=dev) - 0.5).bfloat16()
            Q = torch.empty(tokens, inf, dtype=f8, device=dev)
            xs = torch.empty(tokens, dtype=torch.float32, device=dev)
            pkg.quantize_rows_fp8(X, Q, xs, tokens, inf)
            Yg = torch.empty(tokens, hidden, dtype=torch.bfloat16, device=dev)
            Yw = torch.empty(tokens, out, dtype=torch.bfloat16, device=dev)
            Yr = torch.empty(tokens, hidden, dtype=torch.bfloat16, device=dev)
            silu = torch.nn.functional.silu

            def route(linear):
                def fn():
                    linear()
                    torch.mul(silu(Yw[:, :hidden]), Yw[:, hidden:], out=Yr)
                return fn

            lin16 = lambda: pkg.linear24(blob16, X, Yw, tokens, out, inf)
            lin8 = lambda: pkg.linear24_fp8(blob8, Q, Yw, tokens, out, inf, w_scale=ws, x_scale=xs)
            for name, cols, form in (
                    ("bf16", {"t_glu": lambda: pkg.linear24_glu(blob16, X, Yg, tokens, hidden, inf), "t_linear": lin16, "t_route": route(lin16)},
                     pkg.linear24_glu_form(tokens, hidden, inf, cus=256)),
                    ("fp8", {"t_glu": lambda: pkg.linear24_glu_fp8(blob8, Q, Yg, tokens, hidden, inf, w_scale=ws, x_scale=xs), "t_linear": lin8,
                             "t_route": route(lin8)}, pkg.linear24_glu_form(tokens, hidden, inf))):
                t = {k: [] for k in cols}
                for _ in range(a.repeats):
                    for k, fn in cols.items():
                        t[k].append(pkg.graph_time_ms(fn))
                torch.cuda.synchronize()
                med = {k: statistics.median(v) for k, v in t.items()}
                cell = "  ".join(f"{k} {med[k]:.4f} [{min(v):.4f} .. {max(v):.4f}]" for k, v in t.items())
                verdict = "met" if med["t_glu"] <= med["t_linear"] else ("tie" if med["t_glu"] <= max(t["t_linear"]) else "NOT MET")
                label = f"{name} hidden {hidden} in {inf} tokens {tokens} [{form}]"
                if verdict == "NOT MET":
                    missed.append(label)
                print(f"{label}: {cell}  linear/glu {med['t_linear'] / med['t_glu']:.3f}  route/glu {med['t_route'] / med['t_glu']:.3f}  t_glu <= t_linear: {verdict}",
                      flush=True)
                s = sums.setdefault((name, tokens), {})
                for k in med:
                    s[k] = s.get(k, 0.0) + med[k]
            del X, Q, Yg, Yw, Yr
        del W, blob8, blob16
    print("# summed over the two layers, per type and tokens")
    for (name, tokens), s in sums.items():
        print(f"sum {name} tokens {tokens}: " + "  ".join(f"{k} {v:.4f}" for k, v in s.items())
              + f"  linear/glu {s['t_linear'] / s['t_glu']:.3f}  route/glu {s['t_route'] / s['t_glu']:.3f}", flush=True)
    print("# cells not met (t_glu median above t_linear's max): " + ("; ".join(missed) if missed else "none"))


if __name__ == "__main__":
    main()
