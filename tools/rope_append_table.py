#!/usr/bin/env python3
"""tools/rope_append_table.py -- sm_rope_append_bf16 against the framework route it replaces: us per call over the three
rows of datasets/attn_shapes.csv at 1, 8 and 64 tokens as a decode step (one token per sequence, position = the sequence's length - 1)
and at 1024 and 8192 tokens as the prefill of four sequences (tokens in sequence order); bf16, NEOX pairs over the whole head, Q, K and V
the column slices of one fused QKV buffer, Q rotated in place, pages scattered by a random permutation.

  call    one sm_rope_append_bf16 call (one launch).
  torch   the route a caller has today: cs[positions] gather, rotate-half in fp32 on Q and K (x cos + rotate_half(x) sin), cast, the slot
          block_table[seq, pos // P] * P + pos % P, two index_puts into the cache, Q written back in place.
  copy    a torch copy that moves the call's algorithmic bytes once -- Q, K and V read, Qo and the two cache rows written, the table row
          read: tokens * (2 q_heads + 4 kv_heads) * head_dim * 2 + tokens * head_dim * 4 bytes, half of them as the copy's source -- in
          the same process: the call is reported as a multiple of it and as a fraction of 8 TB/s.
The graph and the eager clock of tools/tablelib.py, median of five; N is 200 up to 64 tokens, 50 up to 2048, 20 above.
Expectation, stated before the run: no cell is behind the torch route (the route is eight to ten launches and several passes over the
tokens), and at 1024 tokens and above the call is within a small factor -- two to three times -- of the copy; below that the call is one
launch's latency, which the copy's launch shares.  Nothing is required of the numbers: the table is the finding.

--part forced: the run SM_ROPE_APPEND_BLOCK_MAX_TOKENS is chosen from -- the rope_append translation unit alone built with every count
forced to BLOCK and to WAVE (tools/probes/rope_append_forced.hip), token counts 1 .. 32768 as prefill, graph clock.

  python tools/rope_append_table.py > profiles/rope_append_table.txt
"""
import argparse
import ctypes
import os
import sys

from tablelib import REPEATS, REPLAYS, attn_shapes as shapes, clocks, medians, paged_cache, probe_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DECODE = [1, 8, 64]
PREFILL = [1024, 8192]
FORCED_TOKENS = [1, 64, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768]
FORCED = {"block": 2147483647, "wave": 0}
PREFILL_SEQS = 4


def calls_for(tokens):
    """calls per graph: enough that a window is milliseconds, not microseconds"""
    return 200 if tokens <= 64 else 50 if tokens <= 2048 else 20


def forced_lib(which):
    """tools/probes/librope_append_<which>.so: rope_append.hip alone with the threshold forced; built when it is not there"""
    L = probe_lib(f"rope_append_{which}", "rope_append_forced.hip", f"ROPE_APPEND_BLOCK_MAX={FORCED[which]}")
    L.sm_rope_append_bf16.argtypes = [ctypes.c_void_p] * 12 + [ctypes.c_size_t] * 19 + [ctypes.c_int, ctypes.c_void_p]
    L.sm_rope_append_bf16.restype = ctypes.c_int
    L.sm_rope_append_form.argtypes = [ctypes.c_size_t] * 5 + [ctypes.POINTER(ctypes.c_int)]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["table", "forced", "all"], default="all")
    ap.add_argument("--build-only", action="store_true", help="build the forced-threshold libraries and leave (no device needed)")
    args = ap.parse_args()
    if args.build_only:
        for w in FORCED:
            forced_lib(w)
        return
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = "cuda:0"

    def operands(tokens, decode, qh, kvh, hd, ps):
        """decode: `tokens` sequences of 1000 + 37 s tokens, the call appends the last; prefill: PREFILL_SEQS sequences share the tokens"""
        gen = torch.Generator(device=dev).manual_seed(tokens * 131 + qh)
        if decode:
            seqs = tokens
            lens = torch.arange(seqs, device=dev, dtype=torch.int32) * 37 % 512 + 1000
            pos, seq = (lens - 1).to(torch.int32), torch.arange(seqs, device=dev, dtype=torch.int32)
        else:
            seqs, per = PREFILL_SEQS, tokens // PREFILL_SEQS
            lens = torch.full((seqs,), per, device=dev, dtype=torch.int32)
            seq = torch.arange(seqs, device=dev, dtype=torch.int32).repeat_interleave(per)
            pos = torch.arange(per, device=dev, dtype=torch.int32).repeat(seqs)
        max_pages = (int(lens.max()) + ps - 1) // ps
        num_pages = seqs * max_pages
        W = (qh + 2 * kvh) * hd
        qkv = torch.randn((tokens, W), generator=gen, device=dev, dtype=torch.bfloat16)
        cut = lambda a, b: qkv[:, a * hd:b * hd].view(tokens, b - a, hd)
        K, V, bt = paged_cache(gen, dev, seqs, max_pages, ps, kvh, hd, normal=False)
        return dict(qkv=qkv, q=cut(0, qh), k=cut(qh, qh + kvh), v=cut(qh + kvh, qh + 2 * kvh), seqs=seqs, max_pages=max_pages, num_pages=num_pages,
                    K=K, V=V, bt=bt, sl=lens, pos=pos, seq=seq, cs=pkg.rope_table(max_pages * ps, hd, device=dev))

    def moved_bytes(tokens, qh, kvh, hd):
        return tokens * (2 * qh + 4 * kvh) * hd * 2 + tokens * hd * 4

    def one_cell(cell, tokens, decode, qh, kvh, hd, ps, behind):
        o = operands(tokens, decode, qh, kvh, hd, ps)
        half = hd // 2
        if decode:
            call = lambda: pkg.rope_append(o["q"], o["k"], o["v"], o["cs"], block_table=o["bt"], k_cache=o["K"], v_cache=o["V"], seq_lens=o["sl"])
        else:
            call = lambda: pkg.rope_append(o["q"], o["k"], o["v"], o["cs"], block_table=o["bt"], k_cache=o["K"], v_cache=o["V"], positions=o["pos"], token_seq=o["seq"])
        Kf, Vf = o["K"].view(-1, kvh, hd), o["V"].view(-1, kvh, hd)
        seq_l, pos_l = o["seq"].long(), o["pos"].long()

        def rot(x, cos, sin):
            xf = x.float()
            return (xf * cos + torch.cat([-xf[..., half:], xf[..., :half]], -1) * sin).to(torch.bfloat16)

        def route():
            row = o["cs"][pos_l]                                                # the gather
            cos, sin = torch.cat([row[:, :half]] * 2, -1)[:, None, :], torch.cat([row[:, half:]] * 2, -1)[:, None, :]
            o["q"].copy_(rot(o["q"], cos, sin))
            kr = rot(o["k"], cos, sin)
            slot = (o["bt"][seq_l, pos_l // ps].long() * ps + pos_l % ps,)
            Kf.index_put_(slot, kr)
            Vf.index_put_(slot, o["v"])
        moved = moved_bytes(tokens, qh, kvh, hd)
        src = torch.empty(max(moved // 2, 16), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        cols, N = {}, calls_for(tokens)
        cols["call graph"], cols["call eager"] = clocks(call, N)
        cols["torch graph"], cols["torch eager"] = clocks(route, N)
        cols["copy graph"], _ = clocks(lambda: dst.copy_(src), N)
        med, runs = medians(cols)
        text = "  ".join(f"{k} {med[k]:.1f} [{min(runs[k]):.1f} .. {max(runs[k]):.1f}]" for k in cols)
        rg, re_ = med["torch graph"] / med["call graph"], med["torch eager"] / med["call eager"]
        form = pkg.rope_append_form(tokens, qh, kvh, hd, hd)
        print(f"{cell} [{form}, N {N}]: {text}  torch/call graph {rg:.2f} eager {re_:.2f}  call/copy {med['call graph'] / med['copy graph']:.2f} "
              f"({moved / med['call graph'] / 1e6:.3f} TB/s of algorithmic bytes, {moved / med['call graph'] / 8e6:.3f} of 8 TB/s)", flush=True)
        for clock, r in (("graph", rg), ("eager", re_)):
            if r < 1.0:
                behind.append(f"{cell} {clock} {r:.2f}")

    if args.part in ("table", "all"):
        print(f"# {pkg.version()}; bf16; us per call, median of {REPEATS} alternated repeats (graph: N calls x {REPLAYS} replays; eager: N calls, launch gaps "
              f"included; N = 200 up to 64 tokens, 50 up to 2048, 20 above); SM_ROPE_APPEND_BLOCK_MAX_TOKENS {pkg.ROPE_APPEND_BLOCK_MAX_TOKENS}")
        behind = []
        for qh, kvh, hd, ps in shapes():
            for tokens, decode in [(t, True) for t in DECODE] + [(t, False) for t in PREFILL]:
                cell = f"q_heads {qh} kv_heads {kvh} head_dim {hd} page {ps} {'decode' if decode else 'prefill'} tokens {tokens}"
                one_cell(cell, tokens, decode, qh, kvh, hd, ps, behind)
                torch.cuda.empty_cache()
        print("# cells where the call is behind the torch route: " + ("none" if not behind else ""))
        for b in behind:
            print("behind: " + b)

    if args.part in ("forced", "all"):
        print(f"# SM_ROPE_APPEND_BLOCK_MAX_TOKENS: the translation unit alone with every count forced to BLOCK and to WAVE, prefill of {PREFILL_SEQS} sequences "
              f"(1 token: one sequence) (graph clock, us per call, median of {REPEATS})")
        libs = {w: forced_lib(w) for w in FORCED}
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())
        for qh, kvh, hd, ps in shapes():
            W = (qh + 2 * kvh) * hd
            for tokens in FORCED_TOKENS:
                o = operands(tokens, tokens < PREFILL_SEQS, qh, kvh, hd, ps)

                def forced(L, want):
                    f = ctypes.c_int(-1)
                    L.sm_rope_append_form(tokens, qh, kvh, hd, hd, ctypes.byref(f))
                    assert pkg.ROPE_APPEND_FORMS[f.value] == want, (f.value, want)

                    def fn():
                        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                        rc = L.sm_rope_append_bf16(ptr(o["q"]), ptr(o["k"]), ptr(o["v"]), ptr(o["q"]), None, ptr(o["K"]), ptr(o["V"]), ptr(o["cs"]), ptr(o["pos"]),
                                                   ptr(o["seq"]), ptr(o["sl"]), ptr(o["bt"]), tokens, o["seqs"], qh, kvh, hd, hd, o["cs"].shape[0], o["num_pages"], ps,
                                                   o["max_pages"], W, W, W, W, 0, kvh * hd, ps * kvh * hd, hd, o["max_pages"], 0, st)
                        assert rc == 0, rc
                    return fn
                cols = {w: clocks(forced(L, w), calls_for(tokens))[0] for w, L in libs.items()}
                med, runs = medians(cols)
                text = "  ".join(f"{k} {med[k]:.1f} [{min(runs[k]):.1f} .. {max(runs[k]):.1f}]" for k in cols)
                best = min(med, key=med.get)
                print(f"forced q_heads {qh} kv_heads {kvh} head_dim {hd} tokens {tokens}: {text}  best {best} (block/wave {med['block'] / med['wave']:.2f})", flush=True)
                del o
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
