#!/usr/bin/env python3
"""From a 16-bit A to the fp8 2:4 blob, per layer of a shape table (default: ResNet-50, b = 32, stacked as one tall A).

For every unique (m, n, k, b) of datasets/<table>.csv with k % 64 == 0 (the stem layer, k = 147, is outside the fp8 kernels'
constraints), one fp16 A of rows = b m, e4m3.  Device times of one call in ms, by hipGraph replay (graph_time_ms), one run:
  torch_route  amax, divide, multiply, cast in torch (fp32 arithmetic, the rule of sm_quantize_rows_fp8) + sm_compress24_fp8
  staged       sm_quantize_rows_fp8 + sm_compress24_fp8
  onepass      sm_quantize_compress24_fp8
  comp_fp8     sm_compress24_fp8 alone (fp8 in, blob out: 1.625 B per element)
  copy         sm_copy_bytes moving 2.625 B per element in all (read + write), the in-run bandwidth yardstick
comp_fp8 and onepass are timed alternately --reps times each; their columns are medians, and `spread` is (max - min) / median
of the comp_fp8 sums of the repetitions.  onepass_roof: 2.625 B per element / 8 TB/s over the time.  For context the whole route
from the 16-bit A to C, onepass + sm_spmma_fp8 (bf16 C, row_scale), next to sm_spmma_fused_f16 on the same A (fp16 C).
Sums are weighted by the number of table rows of each shape."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12
ONEPASS_B, COMP_B = 2.625, 1.625


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default="resnet50")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sm = ge.load_package()
    sm.device_check()
    dev = torch.device("cuda", 0)
    e4 = torch.float8_e4m3fn
    path = args.table if args.table.endswith(".csv") else os.path.join(ROOT, "datasets", args.table + ".csv")
    rows_ = [tuple(int(x) for x in r[:4]) for r in list(csv.reader(open(path)))[1:] if r]
    uniq = []
    for r in rows_:
        if r not in [u for u, _ in uniq]:
            uniq.append((r, rows_.count(r)))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    kinds = ("torch_route", "staged", "onepass", "comp_fp8", "copy", "onepass_spmma_fp8", "spmma_fused_f16")
    emit("m,n,k,b,cnt," + ",".join(f"{x}_ms" for x in kinds) + ",onepass_roof,onepass_over_copy,onepass_over_comp")
    tot = {x: 0.0 for x in kinds}
    rep_comp = [0.0] * args.reps
    rep_one = [0.0] * args.reps
    slower_than_torch = []
    for (m, n, k, b), cnt in uniq:
        if k % 64 != 0:
            emit(f"# {m},{n},{k},{b}: skipped (k % 64 != 0)")
            continue
        rows = b * m
        A = torch.empty(rows * k, dtype=torch.float16, device=dev)
        sm.fill_uniform(A, 5, -1.0, 1.0)
        Q = torch.empty(rows * k, dtype=e4, device=dev)
        rs = torch.empty(rows, dtype=torch.float32, device=dev)
        blob = torch.empty(sm.compress24_size(rows, k, 1, 1), dtype=torch.uint8, device=dev)
        A2 = A.view(rows, k)

        def torch_route():
            x = A2.float()
            amax = x.abs().amax(dim=1, keepdim=True).clamp_min(2.0 ** -100)
            rs.copy_((amax / 448.0).view(-1))
            q = (x * (448.0 / amax)).to(e4)
            sm.compress24_fp8(q, rows, k, k, 1, rows * k, blob)

        def staged():
            sm.quantize_rows_fp8(A, Q, rs, rows, k)
            sm.compress24_fp8(Q, rows, k, k, 1, rows * k, blob)

        def onepass():
            sm.quantize_compress24_fp8(A, blob, rs, rows, k, e4)

        def comp():
            sm.compress24_fp8(Q, rows, k, k, 1, rows * k, blob)

        t = {}
        t["torch_route"] = sm.graph_time_ms(torch_route, iters=args.iters)
        t["staged"] = sm.graph_time_ms(staged, iters=args.iters)
        tc, to = [], []
        for _ in range(args.reps):
            tc.append(sm.graph_time_ms(comp, iters=args.iters))
            to.append(sm.graph_time_ms(onepass, iters=args.iters))
        for i in range(args.reps):
            rep_comp[i] += cnt * tc[i]
            rep_one[i] += cnt * to[i]
        t["comp_fp8"], t["onepass"] = statistics.median(tc), statistics.median(to)
        nb = int(ONEPASS_B / 2 * rows * k) // 16 * 16
        src = torch.empty(nb, dtype=torch.uint8, device=dev)
        dst = torch.empty(nb, dtype=torch.uint8, device=dev)
        t["copy"] = sm.graph_time_ms(lambda: sm.copy_bytes(src, dst), iters=args.iters)
        del src, dst, Q
        # context: the whole route from the 16-bit A to C
        B = torch.empty(k * n, dtype=torch.float16, device=dev)
        sm.fill_uniform(B, 6, -1.0, 1.0)
        Bt = torch.empty(n * k, dtype=e4, device=dev)
        sm.quantize_transpose_fp8(B, Bt, k, n, 448.0)
        C = torch.empty(rows * n, dtype=torch.bfloat16, device=dev)

        def route8():
            sm.quantize_compress24_fp8(A, blob, rs, rows, k, e4)
            sm.spmma_fp8(blob, Bt, C, rows, n, k, 1, 0, alpha=1.0 / 448.0, row_scale=rs)

        t["onepass_spmma_fp8"] = sm.graph_time_ms(route8, iters=args.iters)
        del C
        C16 = torch.empty(rows * n, dtype=torch.float16, device=dev)
        t["spmma_fused_f16"] = sm.graph_time_ms(lambda: sm.spmma_fused(A, B, C16, m, n, k, batch=b), iters=args.iters)
        del C16, A, A2, B, Bt, blob
        for x in kinds:
            tot[x] += cnt * t[x]
        if t["onepass"] >= t["torch_route"]:
            slower_than_torch.append((m, n, k, b))
        emit("%d,%d,%d,%d,%d," % (m, n, k, b, cnt) + ",".join("%.4f" % t[x] for x in kinds) +
             ",%.2f,%.2f,%.2f" % (ONEPASS_B * rows * k / HBM / (t["onepass"] * 1e-3), t["onepass"] / t["copy"], t["onepass"] / t["comp_fp8"]))
    emit("# sums (ms, weighted by table rows, stem layer excluded): " + "  ".join("%s %.3f" % (x, tot[x]) for x in kinds))
    spread = (max(rep_comp) - min(rep_comp)) / statistics.median(rep_comp)
    emit("# comp_fp8 sums of the repetitions: " + " ".join("%.3f" % x for x in rep_comp) + "; onepass: " + " ".join("%.3f" % x for x in rep_one) +
         "; spread %.3f" % spread)
    emit("# sum onepass / sum torch_route = %.2f; shapes where onepass is not faster than torch_route: %s" %
         (tot["onepass"] / tot["torch_route"], slower_than_torch or "none"))
    emit("# sum onepass / sum comp_fp8 = %.3f against the byte ratio %.3f x (1 + spread) = %.3f" %
         (tot["onepass"] / tot["comp_fp8"], ONEPASS_B / COMP_B, ONEPASS_B / COMP_B * (1 + spread)))
    emit("# sum onepass / sum copy = %.2f; sum (onepass + spmma_fp8) / sum spmma_fused_f16 = %.2f" %
         (tot["onepass"] / tot["copy"], tot["onepass_spmma_fp8"] / tot["spmma_fused_f16"]))
    # the re-reading form (rows beyond what a lane holds): no target, reported
    rows, k = 4096, 16448
    A = torch.empty(rows * k, dtype=torch.float16, device=dev)
    sm.fill_uniform(A, 7, -1.0, 1.0)
    rs = torch.empty(rows, dtype=torch.float32, device=dev)
    blob = torch.empty(sm.compress24_size(rows, k, 1, 1), dtype=torch.uint8, device=dev)
    tl = sm.graph_time_ms(lambda: sm.quantize_compress24_fp8(A, blob, rs, rows, k, e4), iters=args.iters)
    emit("# long-row form, %d x %d: %.4f ms, %.2f TB/s of the 2.625 B per element" % (rows, k, tl, ONEPASS_B * rows * k / (tl * 1e-3) / 1e12))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
