#!/usr/bin/env python3
"""What the bias / activation / residual epilogue of the fused 16-bit 2:4 matmul costs, per unique layer shape of a table
(default: ResNet-50, b = 32), fp16.

Device times of one call in ms by hipGraph replay (graph_time_ms), the variants interleaved `--repeats` times in one process so
that they share the clock state; median (min / max for the plain call: its run-to-run spread):
  t_plain      sm_spmma_fused_f16, beta = 0 (the existing kernels: the yardstick)
  t_pass       ONE elementwise pass with the traffic of D = relu(C + bias + R): torch.add(C, R, out=D) -- reads C and R, writes D; a
               lower bound of what a caller pays today, who needs three torch kernels for the expression (t_pass3)
  t_pass3      torch.add(C, R, out=D); D += bias; relu_(D)
  t_bias_relu  sm_spmma_fused_f16_ex with bias + ReLU, no residual
  t_res        sm_spmma_fused_f16_ex with bias + residual (beta = 1, R != D) + ReLU
  t_beta_old   sm_spmma_fused_f16 with beta = 1 (the per-element store of the plain kernels)
Checks printed at the end (the acceptance of the feature): t_res < t_plain + t_pass on every shape; t_res <= t_beta_old on every
shape with n % 8 == 0; t_bias_relu / t_plain per shape next to the spread of t_plain.
--plain-only: only the t_plain column (to confirm on another build of the library that the yardstick is the same kernel)."""
import argparse
import csv
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default="resnet50")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--footer", default=None, help="a text file appended to the table (register counts of the instantiations)")
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

    kinds = ("t_plain",) if args.plain_only else ("t_plain", "t_pass", "t_pass3", "t_bias_relu", "t_res", "t_beta_old")
    emit("m,n,k,b,cnt," + ",".join(kinds) + ",plain_min,plain_max" + ("" if args.plain_only else ",bias_relu/plain,res/(plain+pass),res/beta_old"))
    fails = []
    for (m, n, k, b), cnt in uniq:
        A = torch.empty(b * m * k, dtype=torch.float16, device=dev)
        sm.fill_uniform(A, 5, -1.0, 1.0)
        B = torch.empty(k * n, dtype=torch.float16, device=dev)
        sm.fill_uniform(B, 6, -1.0, 1.0)
        C = torch.empty(b * m * n, dtype=torch.float16, device=dev)
        D = torch.empty_like(C)
        R = torch.empty_like(C)
        sm.fill_uniform(R, 7, -1.0, 1.0)
        bias = torch.rand(n, device=dev) * 2 - 1
        bias16 = bias.half()
        C2, D2, R2 = C.view(-1, n), D.view(-1, n), R.view(-1, n)
        ep_br = sm.Epilogue(bias=bias, act="relu")
        ep_res = sm.Epilogue(bias=bias, act="relu", residual=R)

        def pass3():
            torch.add(C2, R2, out=D2)
            D2.add_(bias16)
            D2.relu_()

        fns = {"t_plain": lambda: sm.spmma_fused(A, B, C, m, n, k, batch=b),
               "t_pass": lambda: torch.add(C, R, out=D),
               "t_pass3": pass3,
               "t_bias_relu": lambda: sm.spmma_fused(A, B, D, m, n, k, batch=b, epilogue=ep_br),
               "t_res": lambda: sm.spmma_fused(A, B, D, m, n, k, batch=b, beta=1.0, epilogue=ep_res),
               "t_beta_old": lambda: sm.spmma_fused(A, B, C, m, n, k, batch=b, beta=1.0)}
        t = {x: [] for x in kinds}
        for _ in range(args.repeats):
            for x in kinds:
                t[x].append(sm.graph_time_ms(fns[x], iters=args.iters))
        med = {x: statistics.median(t[x]) for x in kinds}
        line = "%d,%d,%d,%d,%d," % (m, n, k, b, cnt) + ",".join("%.4f" % med[x] for x in kinds) + ",%.4f,%.4f" % (min(t["t_plain"]), max(t["t_plain"]))
        if not args.plain_only:
            line += ",%.3f,%.3f,%.3f" % (med["t_bias_relu"] / med["t_plain"], med["t_res"] / (med["t_plain"] + med["t_pass"]), med["t_res"] / med["t_beta_old"])
            if not med["t_res"] < med["t_plain"] + med["t_pass"]:
                fails.append(f"{m}x{n}x{k}: t_res {med['t_res']:.4f} >= t_plain + t_pass {med['t_plain'] + med['t_pass']:.4f}")
            if n % 8 == 0 and not med["t_res"] <= med["t_beta_old"]:
                fails.append(f"{m}x{n}x{k}: t_res {med['t_res']:.4f} > t_beta_old {med['t_beta_old']:.4f}")
        emit(line)
        del A, B, C, D, R
    if not args.plain_only:
        emit("# acceptance (t_res < t_plain + t_pass everywhere; t_res <= t_beta_old where n % 8 == 0): " + ("holds on every shape" if not fails else "MISSED"))
        for f in fails:
            emit("#   " + f)
    if args.footer and os.path.exists(args.footer):
        for ln in open(args.footer).read().splitlines():
            emit("# " + ln)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
