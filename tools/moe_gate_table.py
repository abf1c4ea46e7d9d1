#!/usr/bin/env python3
"""tools/moe_gate_table.py -- sm_moe_gate_* against the framework ops it replaces: us per gate at 16, 128, 1024 and 8192
tokens; 8 experts top-2, 64 experts top-8, 256 experts top-8; bf16 and fp32 logits; both scorings.

  gate    one sm_moe_gate_* launch: softmax renormalised over the top_k; sigmoid with a selection bias, renormalised, scale 2.5.
  torch   softmax: softmax(x.float()) -> topk -> w / w.sum -> ids.to(int32);
          sigmoid: sigmoid(x.float()) -> + bias -> topk -> gather -> w / w.sum -> * 2.5 -> ids.to(int32).
The graph and the eager clock of tools/tablelib.py per side, 20 calls each, median of five.
Behind the cells: the gate at 8 experts top-2 as a share of the bf16 balanced block of profiles/moe_block_table.txt (t_block, graph replay)
at the same token count.  Nothing is required of the numbers: the table is the finding.

  python tools/moe_gate_table.py > profiles/moe_gate_table.txt
"""
import os
import re
import sys

from tablelib import CALLS, REPEATS, REPLAYS, clocks, medians

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKENS = [16, 128, 1024, 8192]
ROUTERS = [(8, 2), (64, 8), (256, 8)]


def block_times():
    """tokens -> t_block (ms) of the bf16 balanced cell of profiles/moe_block_table.txt; empty when the file is not there"""
    out = {}
    path = os.path.join(ROOT, "profiles", "moe_block_table.txt")
    if os.path.exists(path):
        for line in open(path):
            m = re.match(r"bf16 8 experts top-2 .* tokens (\d+) balanced .*?: t_block ([0-9.]+)", line)
            if m:
                out[int(m.group(1))] = float(m.group(2))
    return out


def main():
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = "cuda:0"

    blocks = block_times()
    print(f"# {pkg.version()}; us per gate, median of {REPEATS} alternated repeats (graph: {CALLS} calls x {REPLAYS} replays; eager: {CALLS} calls, "
          "launch gaps included)")
    behind, share = [], []
    for experts, top_k in ROUTERS:
        for ty in (torch.bfloat16, torch.float32):
            for scoring in ("softmax", "sigmoid"):
                for tokens in TOKENS:
                    gen = torch.Generator().manual_seed(experts * 100003 + tokens)
                    x = (3.0 * torch.randn(tokens, experts, generator=gen)).to(ty).to(dev)
                    bias = (torch.rand(experts, generator=gen) - 0.5).to(dev) if scoring == "sigmoid" else None
                    scale = 2.5 if scoring == "sigmoid" else 1.0
                    ids = torch.empty(tokens * top_k, dtype=torch.int32, device=dev)
                    w = torch.empty(tokens * top_k, dtype=torch.float32, device=dev)

                    def gate():
                        pkg.moe_gate(x, ids, w, tokens, experts, top_k, scoring=scoring, renormalize=True, scale=scale, select_bias=bias)

                    def ops():
                        if scoring == "softmax":
                            tw, ti = torch.topk(torch.softmax(x.float(), dim=-1), top_k, dim=-1)
                        else:
                            q = torch.sigmoid(x.float())
                            ti = torch.topk(q + bias, top_k, dim=-1).indices
                            tw = torch.gather(q, 1, ti)
                        tw = tw / tw.sum(dim=-1, keepdim=True)
                        if scale != 1.0:
                            tw = tw * scale
                        return tw, ti.to(torch.int32)

                    cols = {}
                    cols["gate graph"], cols["gate eager"] = clocks(gate)
                    cols["torch graph"], cols["torch eager"] = clocks(ops)
                    med, runs = medians(cols)
                    name = {torch.bfloat16: "bf16", torch.float32: "fp32"}[ty]
                    cell = f"{name} {experts} experts top-{top_k} {scoring} tokens {tokens} [{pkg.moe_gate_form(tokens, experts, top_k)}]"
                    text = "  ".join(f"{k} {med[k]:.1f} [{min(runs[k]):.1f} .. {max(runs[k]):.1f}]" for k in cols)
                    rg, re_ = med["torch graph"] / med["gate graph"], med["torch eager"] / med["gate eager"]
                    print(f"{cell}: {text}  torch/gate graph {rg:.2f} eager {re_:.2f}", flush=True)
                    for clock, r in (("graph", rg), ("eager", re_)):
                        if r < 1.0:
                            behind.append(f"{cell} {clock} {r:.2f}")
                    if experts == 8 and name == "bf16" and tokens in blocks:
                        share.append(f"share of the block, {scoring}, tokens {tokens}: gate {med['gate graph']:.1f} us of t_block {blocks[tokens] * 1000:.1f} us = "
                                     f"{med['gate graph'] / (blocks[tokens] * 10):.2f} %  (torch ops: {med['torch graph'] / (blocks[tokens] * 10):.2f} %)")
    print("# the gate (8 experts top-2, bf16, graph clock) against the bf16 balanced block of profiles/moe_block_table.txt")
    for s in share:
        print(s)
    print("# cells where the gate is behind the torch ops: " + ("none" if not behind else ""))
    for b in behind:
        print("behind: " + b)


if __name__ == "__main__":
    main()
