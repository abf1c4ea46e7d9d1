#!/usr/bin/env python3
"""tools/linear_grouped_table.py -- the measurement of the grouped layers sm_linear24_grouped_* (DESIGN.md 4.16): both rows of
datasets/moe_shapes.csv (8 experts: gate/up 28672 x 4096 gated, down 4096 x 14336) in bf16 and in fp8 (e4m3 x e4m3, bf16 out, both
scales given) at 16, 128, 1024 and 8192 routed tokens (rows of X, sorted by expert), under a balanced routing and a skewed one (half
the tokens on expert 0, two experts empty); ms per call by hipGraph replay (graph_time_ms: 20 calls per graph, 3 replays), five
interleaved repeats, median [min .. max] per column, all columns of a cell alternated in one process on warm buffers.

  t_grouped  sm_linear24_grouped_* : one launch, the offsets read from device memory
  t_loop     the parent's code and the comparator: one sm_linear24_* / sm_linear24_glu_* call per NON-EMPTY expert on that expert's
             own blob (the same kept values and metadata, compressed alone) and its slice of X and Y.  The counts are known to the
             host here -- a gift to the loop: a real caller would first copy them from the device and synchronise.
  t_loop2    the same loop again, a column of its own: |t_loop - t_loop2| is the run-to-run spread the requirement is read with.

Requirement: summed over all cells of a token count, at 1024 and 8192 tokens t_grouped <= t_loop + spread.  At 16 and 128 tokens the
loop runs the decode form for every expert with at most 16 tokens, which the grouped call does not have: reported as they come out.

  python tools/linear_grouped_table.py [--tokens 16,128] > profiles/linear_grouped_table.txt

Kernel stats (profiles/linear_grouped_kernel_stats.csv) come from a run of their own, the table under the profiler with one repeat:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/linear_grouped_table.py --repeats 1
(the committed file keeps the rows of this library's kernels, `sm::`; the set-up's torch and runtime helper kernels are dropped)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKENS = [16, 128, 1024, 8192]
REPEATS = 5


def routings(tokens, groups):
    """name -> per-expert counts.  balanced: tokens / groups each, the remainder on the first experts; skewed: half the tokens on
    expert 0, experts 1 and groups - 1 empty, the rest spread over the others."""
    bal = [tokens // groups + (g < tokens % groups) for g in range(groups)]
    rest, others = tokens - tokens // 2, [g for g in range(2, groups - 1)]
    skew = [0] * groups
    skew[0] = tokens // 2
    for i, g in enumerate(others):
        skew[g] = rest // len(others) + (i < rest % len(others))
    assert sum(bal) == tokens == sum(skew) and skew[1] == 0 == skew[groups - 1]
    return {"balanced": bal, "skewed": skew}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default=",".join(map(str, TOKENS)))
    ap.add_argument("--repeats", type=int, default=REPEATS, help="interleaved repeats per cell (1 for the kernel-stats run)")
    ap.add_argument("--shapes", default=os.path.join(ROOT, "datasets", "moe_shapes.csv"))
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = torch.device("cuda:0")
    tokens_list = [int(t) for t in a.tokens.split(",")]
    f8, bf = torch.float8_e4m3fn, torch.bfloat16
    rows = [l.split(",") for l in open(a.shapes).read().splitlines() if l and not l.startswith("#")][1:]
    shapes = [(int(g), int(o), int(i), bool(int(gated))) for g, o, i, gated, _ in rows]

    print(f"# {pkg.version()}; ms per call, median [min .. max] of {a.repeats} interleaved repeats (graph replay, 20 calls x 3 replays)")
    sums, behind = {}, []
    for G, R, inf, gated in shapes:            # R: blob rows of one expert
        width = R // 2 if gated else R         # of Y
        gen = torch.Generator(device=dev).manual_seed(R + inf)
        W = torch.empty(G * R, inf, dtype=bf, device=dev)
        for g in range(G):
            W[g * R:(g + 1) * R] = (torch.rand(R, inf, generator=gen, device=dev) - 0.5).to(bf)
        blob8 = torch.empty(pkg.compress24_size(G * R, inf, 1, 1), dtype=torch.uint8, device=dev)
        ws = torch.empty(G * R, dtype=torch.float32, device=dev)
        pkg.quantize_compress24_fp8(W, blob8, ws, G * R, inf, f8)
        own8 = []
        for g in range(G):
            b = torch.empty(pkg.compress24_size(R, inf, 1, 1), dtype=torch.uint8, device=dev)
            s = torch.empty(R, dtype=torch.float32, device=dev)
            pkg.quantize_compress24_fp8(W[g * R:(g + 1) * R], b, s, R, inf, f8)
            own8.append((b, s))
        pkg.prune24(W, W, G * R, inf, inf, pkg.PRUNE_STRIP)
        blob16 = torch.empty(pkg.compress24_size(G * R, inf, 2, 1), dtype=torch.uint8, device=dev)
        pkg.compress24(W, G * R, inf, inf, 1, G * R * inf, blob16)
        own16 = []
        for g in range(G):
            b = torch.empty(pkg.compress24_size(R, inf, 2, 1), dtype=torch.uint8, device=dev)
            pkg.compress24(W[g * R:(g + 1) * R], R, inf, inf, 1, R * inf, b)
            own16.append(b)
        del W
        for tokens in tokens_list:
            X = (torch.rand(tokens, inf, generator=gen, device=dev) - 0.5).to(bf)
            Q = torch.empty(tokens, inf, dtype=f8, device=dev)
            xs = torch.empty(tokens, dtype=torch.float32, device=dev)
            pkg.quantize_rows_fp8(X, Q, xs, tokens, inf)
            Yg = torch.empty(tokens, width, dtype=bf, device=dev)
            Yl = torch.empty(tokens, width, dtype=bf, device=dev)
            for rname, counts in routings(tokens, G).items():
                offs = [0]
                for c in counts:
                    offs.append(offs[-1] + c)
                off = torch.tensor(offs, dtype=torch.int32, device=dev)
                live = [(g, offs[g], counts[g]) for g in range(G) if counts[g]]

                def grouped16():
                    if gated:
                        pkg.linear24_grouped_glu(blob16, X, Yg, off, G, tokens, width, inf)
                    else:
                        pkg.linear24_grouped(blob16, X, Yg, off, G, tokens, width, inf)

                def loop16():
                    for g, lo, n in live:
                        if gated:
                            pkg.linear24_glu(own16[g], X[lo:lo + n], Yl[lo:lo + n], n, width, inf)
                        else:
                            pkg.linear24(own16[g], X[lo:lo + n], Yl[lo:lo + n], n, width, inf)

                def grouped8():
                    if gated:
                        pkg.linear24_grouped_glu_fp8(blob8, Q, Yg, off, G, tokens, width, inf, w_scale=ws, x_scale=xs)
                    else:
                        pkg.linear24_grouped_fp8(blob8, Q, Yg, off, G, tokens, width, inf, w_scale=ws, x_scale=xs)

                def loop8():
                    for g, lo, n in live:
                        b, s = own8[g]
                        if gated:
                            pkg.linear24_glu_fp8(b, Q[lo:lo + n], Yl[lo:lo + n], n, width, inf, w_scale=s, x_scale=xs[lo:lo + n])
                        else:
                            pkg.linear24_fp8(b, Q[lo:lo + n], Yl[lo:lo + n], n, width, inf, w_scale=s, x_scale=xs[lo:lo + n])

                def loop_forms(cus):
                    q = (lambda n: pkg.linear24_glu_form(n, width, inf, cus=cus)) if gated else (lambda n: pkg.linear24_fp8_form(n, R, inf, cus=cus))
                    return "/".join(sorted({q(n) for _, _, n in live}))

                for name, cols, form, lforms in (
                        ("bf16", {"t_grouped": grouped16, "t_loop": loop16, "t_loop2": loop16}, pkg.linear24_grouped_form(tokens, G, R, inf, cus=256), loop_forms(256)),
                        ("fp8", {"t_grouped": grouped8, "t_loop": loop8, "t_loop2": loop8}, pkg.linear24_grouped_form(tokens, G, R, inf), loop_forms(0))):
                    t = {k: [] for k in cols}
                    for _ in range(a.repeats):
                        for k, fn in cols.items():
                            t[k].append(pkg.graph_time_ms(fn))
                    torch.cuda.synchronize()
                    med = {k: statistics.median(v) for k, v in t.items()}
                    spread = abs(med["t_loop"] - med["t_loop2"])
                    loop = min(med["t_loop"], med["t_loop2"])
                    cell = "  ".join(f"{k} {med[k]:.4f} [{min(v):.4f} .. {max(v):.4f}]" for k, v in t.items())
                    verdict = "ahead" if med["t_grouped"] <= loop else ("tie" if med["t_grouped"] <= loop + spread else "BEHIND")
                    label = f"{name} {'gated ' if gated else ''}{R}x{inf} x{G} tokens {tokens} {rname} [{form}; loop {lforms}]"
                    if verdict == "BEHIND":
                        behind.append(f"{label} ({med['t_grouped'] / loop:.2f}x)")
                    print(f"{label}: {cell}  loop/grouped {loop / med['t_grouped']:.3f}  {verdict}", flush=True)
                    s = sums.setdefault(tokens, {"t_grouped": 0.0, "t_loop": 0.0, "t_loop2": 0.0})
                    for k in med:
                        s[k] += med[k]
            del X, Q, Yg, Yl
        del blob8, blob16, own8, own16
    print("# summed over all cells of a token count (both layers, both types, both routings)")
    for tokens, s in sums.items():
        spread = abs(s["t_loop"] - s["t_loop2"])
        loop = min(s["t_loop"], s["t_loop2"])
        ok = s["t_grouped"] <= loop + spread
        need = "  requirement (grouped <= loop + spread): " + ("met" if ok else "NOT MET") if tokens >= 1024 else "  (reported as it comes out: the loop has the decode form)"
        print(f"sum tokens {tokens}: " + "  ".join(f"{k} {v:.4f}" for k, v in s.items()) + f"  spread {spread:.4f}  loop/grouped {loop / s['t_grouped']:.3f}{need}",
              flush=True)
    print("# cells behind the loop by more than its spread: " + ("; ".join(behind) if behind else "none"))


if __name__ == "__main__":
    main()
