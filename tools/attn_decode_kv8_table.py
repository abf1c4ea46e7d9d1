#!/usr/bin/env python3
"""tools/attn_decode_kv8_table.py -- the fp8 paged KV cache against the 16-bit one: us per call over datasets/attn_shapes.csv.

Part attention: contexts 1024, 4096, 16384 and 32768, batches 1, 8 and 64 (cells whose 16-bit cache exceeds half the device memory are
skipped); bf16 Q and O, an e4m3 cache; every sequence holds the full context, pages scattered by a random permutation.
  kv8     one sm_attn_decode_kv8_bf16 call on a cache quantised from N(0, 1) rows (quantize_rows_fp8 per head row).
  bf16    one sm_attn_decode_bf16 call on the same shape, the same table, the unquantised cache: the call this one is measured against.
  copy    a torch copy that moves the kv8 call's own live bytes -- K and V bytes and their scales once: 2 batch context kv_heads
          (head_dim + 4) -- in the same process: the call is reported as a multiple of it and in TB/s of those bytes.
Part append: sm_rope_append_kv8_bf16 against sm_rope_append_bf16 at 1, 8 and 64 tokens as a decode step and 1024 and 8192 tokens as the prefill
of four sequences, operands as tools/rope_append_table.py builds them.
The graph clock of tools/tablelib.py, median of five, the columns alternated; N is 20, fewer where a call moves more than 256 MB.
Expectation, stated before the run: the attention cells the 16-bit table shows at copy rate (batch >= 8, context >= 4096) get faster, up to
the ratio of the bytes, 2 head_dim / (head_dim + 4); cells bound by launch and reduction latency (batch 1, short contexts) do not.  The
append writes fewer bytes but adds a reduction over the head's lanes: no ratio is expected of it.  Nothing is required of the numbers: the
table is the finding.

  python tools/attn_decode_kv8_table.py > profiles/attn_decode_kv8_table.txt
"""
import argparse
import os
import sys

from tablelib import CALLS, REPEATS, REPLAYS, attn_shapes as shapes, clocks, medians, paged_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CONTEXTS = [1024, 4096, 16384, 32768]
BATCHES = [1, 8, 64]
DECODE = [1, 8, 64]
PREFILL = [1024, 8192]
PREFILL_SEQS = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["attention", "append", "all"], default="all")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    pkg.device_check()
    dev = "cuda:0"
    half_mem = torch.cuda.get_device_properties(0).total_memory // 2
    f8 = torch.float8_e4m3fn

    def quantised(X, kvh, hd):
        """[pages][ps][kvh][hd] bf16 -> the bytes in the same layout and the scales [pages][kvh][ps]"""
        pages, ps = X.shape[:2]
        rows = pages * ps * kvh
        Q8 = torch.empty((rows, hd), dtype=torch.uint8, device=dev).view(f8)
        rs = torch.empty(rows, dtype=torch.float32, device=dev)
        pkg.quantize_rows_fp8(X.view(rows, hd), Q8, rs, rows, hd)
        return Q8.view(pages, ps, kvh, hd), rs.view(pages, ps, kvh).transpose(1, 2).contiguous()

    if args.part in ("attention", "all"):
        print(f"# {pkg.version()}; bf16 Q and O, e4m3 cache; us per call, graph clock, median of {REPEATS} alternated repeats (N calls x {REPLAYS} replays; N = {CALLS}, "
              f"fewer above 256 MB per call); SM_ATTN_DECODE_CHUNK {pkg.ATTN_DECODE_CHUNK}")
        behind = []
        for qh, kvh, hd, ps in shapes():
            for ctx in CONTEXTS:
                for batch in BATCHES:
                    moved16 = 2 * batch * ctx * kvh * hd * 2
                    moved8 = 2 * batch * ctx * kvh * (hd + 4)
                    cell = f"q_heads {qh} kv_heads {kvh} head_dim {hd} page {ps} context {ctx} batch {batch}"
                    if moved16 > half_mem:
                        print(f"{cell}: skipped, the 16-bit cache ({moved16 / 2 ** 30:.1f} GiB) exceeds half the device memory", flush=True)
                        continue
                    calls = CALLS if moved16 <= (256 << 20) else max(2, int(CALLS * (256 << 20) / moved16))
                    gen = torch.Generator(device=dev).manual_seed(batch * 131 + ctx)
                    max_pages = ctx // ps
                    q = torch.randn((batch, qh, hd), generator=gen, device=dev, dtype=torch.bfloat16)
                    K, V, bt = paged_cache(gen, dev, batch, max_pages, ps, kvh, hd, normal=True)
                    (K8, Ks), (V8, Vs) = quantised(K, kvh, hd), quantised(V, kvh, hd)
                    sl = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
                    o8, o16 = (torch.empty((batch, qh, hd), device=dev, dtype=torch.bfloat16) for _ in range(2))
                    ws = torch.empty(max(pkg.attn_decode_workspace_size(batch, qh, hd, ps, max_pages), 16), dtype=torch.uint8, device=dev)
                    src = torch.empty(moved8 // 2, dtype=torch.uint8, device=dev)
                    dst = torch.empty_like(src)
                    cols = {"kv8": clocks(lambda: pkg.attn_decode_kv8(q, K8, V8, Ks, Vs, bt, sl, out=o8, workspace=ws), calls)[0],
                            "bf16": clocks(lambda: pkg.attn_decode(q, K, V, bt, sl, out=o16, workspace=ws), calls)[0],
                            "copy": clocks(lambda: dst.copy_(src), calls)[0]}
                    med, runs = medians(cols)
                    far = float((o8.float() - o16.float()).abs().max())
                    text = "  ".join(f"{k} {med[k]:.1f} [{min(runs[k]):.1f} .. {max(runs[k]):.1f}]" for k in cols)
                    r = med["bf16"] / med["kv8"]
                    print(f"{cell} [{pkg.attn_decode_form(batch, qh, kvh, hd, ps, max_pages)}, N {calls}]: {text}  bf16/kv8 {r:.2f}  kv8/copy {med['kv8'] / med['copy']:.2f} "
                          f"({moved8 / med['kv8'] / 1e6:.2f} TB/s of its live bytes; bf16 {moved16 / med['bf16'] / 1e6:.2f} TB/s of its own)  max |O_kv8 - O_bf16| {far:.3g}", flush=True)
                    if r < 1.0:
                        behind.append(f"{cell} {r:.2f}")
                    del K, V, K8, V8, Ks, Vs, src, dst, ws
                    torch.cuda.empty_cache()
        print("# cells where the kv8 call is behind the bf16 call: " + ("none" if not behind else ""))
        for b in behind:
            print("behind: " + b)

    if args.part in ("append", "all"):
        print(f"# append: sm_rope_append_kv8_bf16 (e4m3) against sm_rope_append_bf16; NEOX over the whole head, Q in place; us per call, graph clock, median of {REPEATS}")
        for qh, kvh, hd, ps in shapes():
            for tokens, decode in [(t, True) for t in DECODE] + [(t, False) for t in PREFILL]:
                gen = torch.Generator(device=dev).manual_seed(tokens * 131 + qh)
                if decode:
                    seqs = tokens
                    lens = torch.arange(seqs, device=dev, dtype=torch.int32) * 37 % 512 + 1000
                    kw = dict(seq_lens=lens)
                else:
                    seqs, per = PREFILL_SEQS, tokens // PREFILL_SEQS
                    lens = torch.full((seqs,), per, device=dev, dtype=torch.int32)
                    kw = dict(positions=torch.arange(per, device=dev, dtype=torch.int32).repeat(seqs),
                              token_seq=torch.arange(seqs, device=dev, dtype=torch.int32).repeat_interleave(per))
                max_pages = (int(lens.max()) + ps - 1) // ps
                W = (qh + 2 * kvh) * hd
                qkv = torch.randn((tokens, W), generator=gen, device=dev, dtype=torch.bfloat16)
                cut = lambda a, b: qkv[:, a * hd:b * hd].view(tokens, b - a, hd)
                q, k, v = cut(0, qh), cut(qh, qh + kvh), cut(qh + kvh, qh + 2 * kvh)
                K, V, bt = paged_cache(gen, dev, seqs, max_pages, ps, kvh, hd, normal=False)
                K8, V8 = (torch.zeros(K.shape, dtype=torch.uint8, device=dev).view(f8) for _ in range(2))
                Ks, Vs = (torch.zeros((K.shape[0], kvh, ps), dtype=torch.float32, device=dev) for _ in range(2))
                cs = pkg.rope_table(max_pages * ps, hd, device=dev)
                calls = 200 if tokens <= 64 else 50 if tokens <= 2048 else 20
                cols = {"kv8": clocks(lambda: pkg.rope_append_kv8(q, k, v, cs, bt, K8, V8, Ks, Vs, **kw), calls)[0],
                        "bf16": clocks(lambda: pkg.rope_append(q, k, v, cs, block_table=bt, k_cache=K, v_cache=V, **kw), calls)[0]}
                med, runs = medians(cols)
                text = "  ".join(f"{c} {med[c]:.1f} [{min(runs[c]):.1f} .. {max(runs[c]):.1f}]" for c in cols)
                print(f"append q_heads {qh} kv_heads {kvh} head_dim {hd} page {ps} tokens {tokens} {'decode' if decode else 'prefill'} "
                      f"[{pkg.rope_append_form(tokens, qh, kvh, hd, hd)}, N {calls}]: {text}  bf16/kv8 {med['bf16'] / med['kv8']:.2f}", flush=True)


if __name__ == "__main__":
    main()
