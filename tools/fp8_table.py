#!/usr/bin/env python3
"""The fp8 2:4 path against the fp16 one, per layer of a shape table (default: ResNet-50, b = 32).

For every unique (m, n, k, b) of datasets/<table>.csv with k % 64 == 0 (the 7 x 7 x 3 stem layer, k = 147, is outside the
fp8 kernels' constraints, as for int8), one e4m3 A of b matrices, one shared e4m3 B ([n][k]) and a bf16 C.  Device times
of one call in ms, by hipGraph replay (graph_time_ms), all in one run:
  spmma_fp8   sm_spmma_fp8 on the compressed A, bf16 out
  fused_fp8   sm_spmma_fused_fp8 from the dense A (STRIP selection in registers), bf16 out
  comp_fp8    sm_compress24_fp8
  spmma_f16   sm_spmma_f16 on the same shape (fp16 blob, row-major fp16 B, fp16 C)
Per kernel: effective TF/s (2 m n k b dense-equivalent flops over the time) and the byte-roofline fraction,
bytes / 8 TB/s over the time, with bytes = blob + B + C read or written once (fused: dense A instead of the blob;
compress: dense A + blob).  Sums are weighted by the number of table rows of each shape."""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default="resnet50")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    sm = ge.load_package()
    sm.device_check()
    dev = torch.device("cuda", 0)
    path = args.table if args.table.endswith(".csv") else os.path.join(ROOT, "datasets", args.table + ".csv")
    rows = [tuple(int(x) for x in r[:4]) for r in list(csv.reader(open(path)))[1:] if r]
    uniq = []
    for r in rows:
        if r not in [u for u, _ in uniq]:
            uniq.append((r, rows.count(r)))
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    kinds = ("spmma_fp8", "fused_fp8", "comp_fp8", "spmma_f16")
    emit("m,n,k,b,cnt," + ",".join(f"{x}_ms" for x in kinds) + "," + ",".join(f"{x}_tfs" for x in kinds) + "," +
         ",".join(f"{x}_roof" for x in kinds) + ",fp8_over_f16")
    tot = {x: 0.0 for x in kinds}
    g = torch.Generator(device=dev).manual_seed(3)
    for (m, n, k, b), cnt in uniq:
        if k % 64 != 0:
            emit(f"# {m},{n},{k},{b}: skipped (k % 64 != 0)")
            continue
        A = (torch.rand(b * m * k, generator=g, device=dev) * 2 - 1).to(torch.float8_e4m3fn)
        Bt = (torch.rand(n * k, generator=g, device=dev) * 2 - 1).to(torch.float8_e4m3fn)
        C = torch.empty(b * m * n, dtype=torch.bfloat16, device=dev)
        blob = torch.empty(sm.compress24_size(m, k, 1, b), dtype=torch.uint8, device=dev)
        sm.compress24_fp8(A, m, k, k, b, m * k, blob)
        t = {}
        t["spmma_fp8"] = sm.graph_time_ms(lambda: sm.spmma_fp8(blob, Bt, C, m, n, k, b), iters=args.iters)
        t["fused_fp8"] = sm.graph_time_ms(lambda: sm.spmma_fused_fp8(A, Bt, C, m, n, k, batch=b), iters=args.iters)
        t["comp_fp8"] = sm.graph_time_ms(lambda: sm.compress24_fp8(A, m, k, k, b, m * k, blob), iters=args.iters)
        blob8 = blob.numel()
        del A, C, blob
        A16 = torch.empty(b * m * k, dtype=torch.float16, device=dev)
        sm.fill_uniform(A16, 5, -1.0, 1.0)
        B16 = torch.empty(k * n, dtype=torch.float16, device=dev)
        sm.fill_uniform(B16, 6, -1.0, 1.0)
        blob16 = torch.empty(sm.compress24_size(m, k, 2, b), dtype=torch.uint8, device=dev)
        sm.compress24(A16, m, k, k, b, m * k, blob16)
        blob16_n = blob16.numel()
        del A16
        C16 = torch.empty(b * m * n, dtype=torch.float16, device=dev)
        t["spmma_f16"] = sm.graph_time_ms(lambda: sm.spmma(blob16, B16, C16, m, n, k, b), iters=args.iters)
        del blob16, B16, C16, Bt
        fl = 2.0 * m * n * k * b
        by = {"spmma_fp8": blob8 + n * k + 2 * b * m * n, "fused_fp8": b * m * k + n * k + 2 * b * m * n, "comp_fp8": b * m * k + blob8,
              "spmma_f16": blob16_n + 2 * n * k + 2 * b * m * n}
        for x in kinds:
            tot[x] += cnt * t[x]
        emit("%d,%d,%d,%d,%d," % (m, n, k, b, cnt) + ",".join("%.4f" % t[x] for x in kinds) + "," +
             ",".join("%.0f" % (fl / (t[x] * 1e-3) / 1e12) for x in kinds) + "," +
             ",".join("%.2f" % (by[x] / HBM / (t[x] * 1e-3)) for x in kinds) + ",%.2f" % (t["spmma_fp8"] / t["spmma_f16"]))
    emit("# sums (ms, weighted by table rows, stem layer excluded): " + "  ".join("%s %.3f" % (x, tot[x]) for x in kinds))
    emit("# sum spmma_fp8 / sum spmma_f16 = %.2f" % (tot["spmma_fp8"] / tot["spmma_f16"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
