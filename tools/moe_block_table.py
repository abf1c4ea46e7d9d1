#!/usr/bin/env python3
"""tools/moe_block_table.py -- the measurement of the MoE block: both rows of datasets/moe_shapes.csv as ONE block
(8 experts, top-2: gate/up 28672 x 4096 gated, down 4096 x 14336) from the router's ids to the combined hidden states, in bf16 and in
fp8 (e4m3 x e4m3, bf16 out, both scales), at 16, 128, 1024 and 8192 tokens (P = 2 x tokens routed pairs), under a balanced routing and
a skewed one (every token's first choice is expert 0, two experts empty); ms per block by hipGraph replay where the column can be
captured (graph_time_ms: 20 calls per graph, 3 replays), else eagerly between two events (20 calls, launch gaps included), five
interleaved repeats, median [min .. max] per column, all columns of a cell alternated in one process on warm buffers.

  t_block   this library end to end: sm_moe_route, the gathered gated layer (X stays in token order), the grouped down projection,
            sm_moe_combine (weights, the residual add in place of a separate pass).  fp8: X is quantised per token once (outside the
            clock, as the previous layer's epilogue would), the gated layer's output per pair inside it (both columns pay it).
  t_block_eager  the same calls timed eagerly, as the glued route has to be: the like-for-like column a cell is judged on.
  t_glue    the parent's route: torch.sort (stable) + bincount / cumsum + index_select of X (fp8: and of its scales) + the existing
            grouped calls + index_select . weights summed over top_k + the residual, all framework ops around the same two launches.
            Eager: torch.bincount reads its output size back to the host, a synchronisation no capture takes.
  t_glue2   the same again, a column of its own: |t_glue - t_glue2| is the run-to-run spread a cell is judged with.

A cell is BEHIND when t_block_eager > min(t_glue, t_glue2) + spread.  Nothing is required of the numbers: the table is the finding.
Also printed per cell: the activation bytes each route moves through HBM around the two matmuls (the glue writes the [P][in] copy of X
and reads it back; the block reads X's rows in place).

  python tools/moe_block_table.py [--tokens 16,128] > profiles/moe_block_table.txt

Kernel stats (profiles/moe_block_kernel_stats.csv) come from a run of their own, the table under the profiler with one repeat:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 tools/moe_block_table.py --repeats 1
(the committed file keeps the rows of this library's kernels, `sm::`)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKENS = [16, 128, 1024, 8192]
REPEATS = 5


def router(tokens, top_k, groups, kind):
    """ids[tokens * top_k], top_k distinct experts per token.  balanced: pair (t, j) -> (top_k t + j) mod groups; skewed: every token's
    first choice is expert 0, experts 1 and groups - 1 stay empty, the other choices go round the rest."""
    ids = []
    others = list(range(2, groups - 1))
    for t in range(tokens):
        for j in range(top_k):
            if kind == "balanced":
                ids.append((top_k * t + j) % groups)
            else:
                ids.append(0 if j == 0 else others[(t * (top_k - 1) + j - 1) % len(others)])
    return ids


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
    f8, bf = torch.float8_e4m3fn, torch.bfloat16
    rows = [l.split(",") for l in open(a.shapes).read().splitlines() if l and not l.startswith("#")][1:]
    (G, R1, inf, g1, K), (G2, R2, mid, g2, K2) = [tuple(int(v) for v in r) for r in rows]
    assert g1 == 1 and g2 == 0 and G == G2 and K == K2 and R1 == 2 * mid and R2 == inf, "the two rows are one block: gate/up, then down"

    def weights(R, k, seed):
        gen = torch.Generator(device=dev).manual_seed(seed)
        W = torch.empty(G * R, k, dtype=bf, device=dev)
        for g in range(G):
            W[g * R:(g + 1) * R] = (torch.rand(R, k, generator=gen, device=dev) - 0.5).to(bf)
        b8 = torch.empty(pkg.compress24_size(G * R, k, 1, 1), dtype=torch.uint8, device=dev)
        ws = torch.empty(G * R, dtype=torch.float32, device=dev)
        pkg.quantize_compress24_fp8(W, b8, ws, G * R, k, f8)
        pkg.prune24(W, W, G * R, k, k, pkg.PRUNE_STRIP)
        b16 = torch.empty(pkg.compress24_size(G * R, k, 2, 1), dtype=torch.uint8, device=dev)
        pkg.compress24(W, G * R, k, k, 1, G * R * k, b16)
        return b16, b8, ws

    up16, up8, upws = weights(R1, inf, 1)
    dn16, dn8, dnws = weights(R2, mid, 2)
    torch.cuda.synchronize()

    def timed(fn, capture):
        if capture:
            return pkg.graph_time_ms(fn)
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / 20

    print(f"# {pkg.version()}; ms per block, median [min .. max] of {a.repeats} interleaved repeats (t_block: graph replay, 20 blocks x 3 replays; the other "
          f"columns: 20 eager calls between two events, launch gaps included)")
    behind, sums = [], {}
    for tokens in [int(t) for t in a.tokens.split(",")]:
        P = tokens * K
        gen = torch.Generator(device=dev).manual_seed(tokens)
        X = (torch.rand(tokens, inf, generator=gen, device=dev) - 0.5).to(bf)
        Q = torch.empty(tokens, inf, dtype=f8, device=dev)
        xs = torch.empty(tokens, dtype=torch.float32, device=dev)
        pkg.quantize_rows_fp8(X, Q, xs, tokens, inf)
        w = torch.rand(P, generator=gen, device=dev)
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        off, st, sp, pp = i32(G + 1), i32(P), i32(P), i32(P)
        nb = pkg.moe_route_workspace_size(tokens, K, G)
        wsp = torch.empty(max(nb, 4), dtype=torch.uint8, device=dev) if nb else None
        H = torch.empty(P, mid, dtype=bf, device=dev)
        H8 = torch.empty(P, mid, dtype=f8, device=dev)
        hs = torch.empty(P, dtype=torch.float32, device=dev)
        Yp = torch.empty(P, inf, dtype=bf, device=dev)
        out = torch.empty(tokens, inf, dtype=bf, device=dev)
        outg = torch.empty(tokens, inf, dtype=bf, device=dev)
        for rname in ("balanced", "skewed"):
            ids = torch.tensor(router(tokens, K, G, rname), dtype=torch.int32, device=dev)
            ids64 = ids.long()

            def block16():
                pkg.moe_route(ids, tokens, K, G, off, st, sp, pp, workspace=wsp)
                pkg.linear24_grouped_glu(up16, X, H, off, G, P, mid, inf, x_index=st, x_rows=tokens)
                pkg.linear24_grouped(dn16, H, Yp, off, G, P, inf, mid)
                pkg.moe_combine(Yp, pp, out, tokens, K, inf, P, weights=w, residual=X)

            def block8():
                pkg.moe_route(ids, tokens, K, G, off, st, sp, pp, workspace=wsp)
                pkg.linear24_grouped_glu_fp8(up8, Q, H, off, G, P, mid, inf, w_scale=upws, x_scale=xs, x_index=st, x_rows=tokens)
                pkg.quantize_rows_fp8(H, H8, hs, P, mid)
                pkg.linear24_grouped_fp8(dn8, H8, Yp, off, G, P, inf, mid, w_scale=dnws, x_scale=hs)
                pkg.moe_combine(Yp, pp, out, tokens, K, inf, P, weights=w, residual=X)

            def glue_route():
                order = torch.sort(ids64, stable=True).indices
                offs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(torch.bincount(ids64, minlength=G), 0)]).to(torch.int32)
                return order, offs, torch.div(order, K, rounding_mode="floor")

            def glue_combine(order):
                pos = torch.empty_like(order)
                pos[order] = torch.arange(P, device=dev)
                y = Yp.index_select(0, pos).view(tokens, K, inf).float() * w.view(tokens, K, 1)
                outg.copy_((X.float() + y.sum(1)).to(bf))

            def glue16():
                order, offs, tok = glue_route()
                Xs = X.index_select(0, tok)
                pkg.linear24_grouped_glu(up16, Xs, H, offs, G, P, mid, inf)
                pkg.linear24_grouped(dn16, H, Yp, offs, G, P, inf, mid)
                glue_combine(order)

            def glue8():
                order, offs, tok = glue_route()
                Qs, xss = Q.view(torch.uint8).index_select(0, tok).view(f8), xs.index_select(0, tok)
                pkg.linear24_grouped_glu_fp8(up8, Qs, H, offs, G, P, mid, inf, w_scale=upws, x_scale=xss)
                pkg.quantize_rows_fp8(H, H8, hs, P, mid)
                pkg.linear24_grouped_fp8(dn8, H8, Yp, offs, G, P, inf, mid, w_scale=dnws, x_scale=hs)
                glue_combine(order)

            for name, elt, cols in (("bf16", 2, {"t_block": (block16, True), "t_block_eager": (block16, False), "t_glue": (glue16, False), "t_glue2": (glue16, False)}),
                                    ("fp8", 1, {"t_block": (block8, True), "t_block_eager": (block8, False), "t_glue": (glue8, False), "t_glue2": (glue8, False)})):
                t = {k: [] for k in cols}
                for _ in range(a.repeats):
                    for k, (fn, capture) in cols.items():
                        t[k].append(timed(fn, capture))
                torch.cuda.synchronize()
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = abs(med["t_glue"] - med["t_glue2"])
                glue = min(med["t_glue"], med["t_glue2"])
                verdict = "ahead" if med["t_block_eager"] <= glue else ("tie" if med["t_block_eager"] <= glue + spread else "BEHIND")
                cell = "  ".join(f"{k} {med[k]:.4f} [{min(v):.4f} .. {max(v):.4f}]" for k, v in t.items())
                # activation bytes around the matmuls: ids, the route's arrays, X rows read by the gated layer, Yp read by the combine, out, the residual
                common = P * inf * elt + P * inf * 2 + 2 * tokens * inf * 2 + P * 4
                b_block = common + 4 * P + (G + 1 + 3 * P) * 4 + P * 4 + P * 4              # ids; offsets, sorted_token, sorted_pair, pair_pos; x_index, pair_pos read
                b_glue = common + 8 * P * 3 + 2 * P * inf * elt + 2 * P * inf * 4            # sort keys / order / pos (int64); the [P][in] copy written + its source read; the fp32 product written + read
                label = f"{name} {G} experts top-{K} {inf} -> {mid} -> {inf} tokens {tokens} {rname} [route {pkg.moe_route_form(tokens, K, G)}]"
                if verdict == "BEHIND":
                    behind.append(f"{label} ({med['t_block_eager'] / glue:.2f}x)")
                print(f"{label}: {cell}  glue/block_eager {glue / med['t_block_eager']:.3f}  glue/block {glue / med['t_block']:.3f}  {verdict}  bytes block {b_block / 1e6:.2f} MB glue {b_glue / 1e6:.2f} MB",
                      flush=True)
                s = sums.setdefault(tokens, {"t_block": 0.0, "t_block_eager": 0.0, "t_glue": 0.0, "t_glue2": 0.0})
                for k in med:
                    s[k] += med[k]
        del X, Q, H, H8, Yp, out, outg
    print("# summed over all cells of a token count (both types, both routings)")
    for tokens, s in sums.items():
        spread = abs(s["t_glue"] - s["t_glue2"])
        glue = min(s["t_glue"], s["t_glue2"])
        print(f"sum tokens {tokens}: " + "  ".join(f"{k} {v:.4f}" for k, v in s.items()) + f"  spread {spread:.4f}  glue/block_eager {glue / s['t_block_eager']:.3f}  glue/block {glue / s['t_block']:.3f}", flush=True)
    print("# cells behind the glued route by more than its spread: " + ("; ".join(behind) if behind else "none"))


if __name__ == "__main__":
    main()
