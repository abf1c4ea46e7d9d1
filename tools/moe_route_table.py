#!/usr/bin/env python3
"""tools/moe_route_table.py -- sm_moe_route alone: us per call by hipGraph replay (graph_time_ms, median of three)
at 8 experts top-2 and 256 experts top-8 (a seeded router, top_k distinct experts per token), from 32 to 65536 pairs -- both sides of
the SINGLE / MULTI threshold (4096 pairs).

  python tools/moe_route_table.py > profiles/moe_route_table.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = "cuda:0"
    print(f"# {pkg.version()}; us per sm_moe_route call, median of 3 (graph replay, 20 calls x 3 replays)")
    for G, top_k in ((8, 2), (256, 8)):
        for P in (32, 256, 1024, 2048, 4096, 4097, 8192, 16384, 65536):
            K = top_k if P % top_k == 0 else 1
            T = P // K
            rng = np.random.default_rng(P)
            ids = torch.from_numpy(np.argsort(rng.random((T, G)), axis=1)[:, :K].reshape(-1).astype(np.int32)).to(dev)
            i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
            off, st, sp, pp = i32(G + 1), i32(P), i32(P), i32(P)
            nb = pkg.moe_route_workspace_size(T, K, G)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev) if nb else None
            fn = lambda: pkg.moe_route(ids, T, K, G, off, st, sp, pp, workspace=ws)
            ms = sorted(pkg.graph_time_ms(fn) for _ in range(3))[1]
            print(f"groups {G} top_k {K} pairs {P} form {pkg.moe_route_form(T, K, G)}: {ms * 1000:.1f} us", flush=True)


if __name__ == "__main__":
    main()
