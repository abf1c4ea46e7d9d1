"""sm_rope_append_kv8_{f16,bf16} on the device (-m gpu): RoPE on every Q and K head and the quantising append of K and V to the fp8 paged
cache, in one launch.

Every case (tests/kv8_testlib.py: append_cases) reads Q, K and V as rope_append_testlib lays them out (column slices of one fused buffer at a
moved base, NaN in all padding and in the rows of padding tokens); Qo, Ko, BOTH byte caches and BOTH scale arrays hold a sentinel everywhere,
a guard page in front of page 0 and behind the last page of each included -- the places an unclamped kernel would address from the ids -1
and num_pages the tables hold.  Each case asserts its form through sm_rope_append_form, runs twice (same bits) and compares EVERY buffer whole
with what the restatement leaves there: Qo and Ko bit for bit what sm_rope_append_* writes (NaN by class), the bytes and the scales bit for
bit b8_testlib.ref_quant_rows of the rotated, rounded K head and of the V head, and bit for bit the uploaded contents everywhere else -- so a
refused append and a padding token write neither bytes nor scales.  The definition fixes every rounding: there is no tolerance.

Which failure each shape is the smallest to catch -- head_dim 64 / rot_dim 32 and 128 / 64 under NEOX: 6 and 12 item lanes a head, where a
power-of-two exchange ladder reads another head's lanes; rot_dim 16: 7 and 15; rot_dim 0 and head_dim: 8 / 16 and 4 / 8 lanes, copied and
rotated rows; heads (5, 5), (3, 1), (32, 8): head steps that do not fill a wave and K / V heads in different waves of a BLOCK workgroup;
BLOCK_MAX + 1, + 2 tokens: the WAVE form; a page edge (slots 15, 16, 17), padding by position, by sequence id and by a zero length; the
append refused beyond the capacity, at an absent page and at a sequence id out of range while Qo is still written; both decode spellings;
in place, out of place, without Ko; rows that are all +0, all -0, hold a NaN, hold +-inf, or whose amax is subnormal in the 16-bit type.

The file is ONE test item: test_quantising_append_on_the_device walks the classes below over their case tables (kv8_testlib.each) and reports
the failed cases together, each under its id."""
import numpy as np
import pytest
import torch

import attn_decode_testlib as al
import b8_testlib as b8
import kv8_testlib as kl
import rope_append_testlib as rl

pytestmark = pytest.mark.gpu


def every_buffer_bit_for_bit_against_the_restatement(gpu, cf):
    case, fmt = cf
    pr, (Q, K, V, cs) = kl.make_append(case)
    kl.AppendLayout(pr, Q, K, V, cs, fmt, torch).twice(gpu, rl.form_of(gpu, pr))


def wave_form_past_the_threshold_and_the_same_bits_on_both_sides(gpu, extra, fmt):
    """BLOCK_MAX + extra tokens run WAVE (extra 1: head_dim 64, rot_dim 32, NEOX -- six lanes a head); the same operands cut to BLOCK_MAX
    tokens run BLOCK: both equal the restatement, and the common tokens' bytes and scales are compared directly as well"""
    B = gpu.ROPE_APPEND_BLOCK_MAX_TOKENS
    case = rl.wave_twin(B, extra)
    pr, (Q, K, V, cs) = kl.make_append(case)
    assert pr.tokens == B + extra
    lay = kl.AppendLayout(pr, Q, K, V, cs, fmt, torch)
    wave = lay.run(gpu, "wave")
    cut = rl.Problem.__new__(rl.Problem)
    cut.__dict__.update(pr.__dict__)
    cut.tokens = B
    cut.token_seq, cut.positions, cut.s, cut.pos, cut.live, cut.slot = pr.token_seq[:B], pr.positions[:B], pr.s[:B], pr.pos[:B], pr.live[:B], pr.slot[:B]
    lay2 = kl.AppendLayout(cut, Q[:B], K[:B], V[:B], cs, fmt, torch)
    block = lay2.run(gpu, "block")
    for name in ("Kc8", "Vc8", "Ksc", "Vsc"):
        w = lay2.written[name]
        assert w.any() and np.array_equal(wave[name][w], block[name][w]), name


def cache_bytes_equal_quantize_rows_fp8_on_ko(gpu, ty, fmt, hd, style):
    """the device's own quantiser on Ko viewed as [tokens * kv_heads][head_dim], and on V: the bytes and row_scales the append stored"""
    pkg, ps, kvh, qh, tokens = gpu, 16, 2, 4, 37
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
    rng = np.random.default_rng(kl.seed(kl.SALT, "quantiser", hd))
    t16 = lambda a: torch.from_numpy(al.bits_of(a, ty).view(np.int16)).cuda().view(dt)
    q, k, v = (t16(rng.normal(0, 1, (tokens, h, hd))) for h in (qh, kvh, kvh))
    max_pages = -(-tokens // ps)
    bt = torch.from_numpy(rng.permutation(max_pages + 2)[:max_pages].astype(np.int32).reshape(1, max_pages)).cuda()
    kc, vc = (torch.zeros((max_pages + 2, ps, kvh, hd), dtype=torch.uint8, device="cuda").view(b8.tdt(fmt)) for _ in range(2))
    ksc, vsc = (torch.zeros((max_pages + 2, kvh, ps), dtype=torch.float32, device="cuda") for _ in range(2))
    pos = torch.from_numpy(rng.permutation(tokens).astype(np.int32)).cuda()
    ko = torch.zeros_like(k)
    pkg.rope_append_kv8(q, k, v, pkg.rope_table(tokens, hd, device="cuda"), bt, kc, vc, ksc, vsc, positions=pos, token_seq=torch.zeros(tokens, dtype=torch.int32, device="cuda"),
                        style=style, q_out=torch.zeros_like(q), k_out=ko)
    for src, c8, sc in ((ko, kc, ksc), (v, vc, vsc)):
        Qb = torch.zeros((tokens * kvh, hd), dtype=torch.uint8, device="cuda").view(b8.tdt(fmt))
        rs = torch.zeros(tokens * kvh, dtype=torch.float32, device="cuda")
        pkg.quantize_rows_fp8(src.reshape(tokens * kvh, hd), Qb, rs, tokens * kvh, hd)
        torch.cuda.synchronize()
        pg, sl = bt[0, (pos // ps).long()].long(), (pos % ps).long()
        assert torch.equal(c8.view(torch.uint8)[pg, sl], Qb.view(torch.uint8).view(tokens, kvh, hd))
        assert torch.equal(sc[pg, :, sl].view(torch.int32), rs.view(tokens, kvh).view(torch.int32))


def hipgraph_replay_after_lengths_and_table_changed_on_the_device(gpu, ty, fmt, hd, group):
    """a decode-spelling rope_append_kv8 followed by attn_decode_kv8, captured once; between replays seq_lens grow past a page boundary and
    block_table rows are rewritten ON THE DEVICE; each replay equals the eager pair on the new state bit for bit"""
    pkg, ps, kvh, seqs = gpu, 16, 2, 3
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
    max_pages, qh = 6, group * kvh
    num_pages = seqs * max_pages
    rng = np.random.default_rng(kl.seed(kl.SALT, "graph", hd))
    t16 = lambda a: torch.from_numpy(al.bits_of(a, ty).view(np.int16)).cuda().view(dt)
    qkv = t16(rng.normal(0, 1, (seqs, (qh + 2 * kvh) * hd)))
    q0, k, v = (qkv[:, a * hd:b * hd].view(seqs, -1, hd) for a, b in ((0, qh), (qh, qh + kvh), (qh + kvh, qh + 2 * kvh)))
    c0 = [torch.from_numpy(b8.finite_bytes(rng, (num_pages, ps, kvh, hd), fmt)).cuda().view(b8.tdt(fmt)) for _ in range(2)]
    s0 = [torch.from_numpy(rng.uniform(0.002, 0.01, (num_pages, kvh, ps)).astype(np.float32)).cuda() for _ in range(2)]
    cs = pkg.rope_table(max_pages * ps, hd, device="cuda")
    tables = [torch.from_numpy(rng.permutation(num_pages).astype(np.int32).reshape(seqs, max_pages)).cuda() for _ in range(2)]
    states = [([ps - 1, 5, 1], 0), ([ps, ps + 1, 2 * ps + 3], 0), ([ps + 1, 3 * ps, 2 * ps + 4], 1), ([max_pages * ps, 1, ps], 1)]
    bt, sl = tables[0].clone(), torch.zeros(seqs, dtype=torch.int32, device="cuda")

    def pair(qo, kc, vc, ks, vs, out):
        pkg.rope_append_kv8(q0, k, v, cs, bt, kc, vc, ks, vs, seq_lens=sl, q_out=qo)
        pkg.attn_decode_kv8(qo, kc, vc, ks, vs, bt, sl, out=out)
    fresh = lambda: (torch.zeros_like(q0.contiguous()), c0[0].clone(), c0[1].clone(), s0[0].clone(), s0[1].clone(), torch.zeros((seqs, qh, hd), dtype=dt, device="cuda"))
    held = fresh()
    sl.copy_(torch.tensor(states[0][0], dtype=torch.int32))
    pair(*held)                                                       # (warm-up outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pair(*held)
    bits = lambda t: t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])
    for lens, which in states:
        sl.copy_(torch.tensor(lens, dtype=torch.int32).cuda())
        bt.copy_(tables[which])
        for h, f in zip(held, fresh()):
            h.copy_(f)
        held[0].fill_(7.0), held[5].fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        eager = fresh()
        pair(*eager)
        torch.cuda.synchronize()
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(held, eager)), (lens, which)
        assert not torch.equal(bits(held[1]), bits(c0[0])) and not torch.equal(bits(held[3]), bits(s0[0])) and bool(torch.isfinite(held[5].float()).all())


def test_quantising_append_on_the_device(gpu):
    """ONE test item walks every class above and reports the failed cases together, each under its id: the case table (every buffer whole
    against the restatement), the WAVE form past the threshold, the device quantiser on Ko, graph replay."""
    kl.each(kl.append_cases(), kl.append_case_id, lambda cf: every_buffer_bit_for_bit_against_the_restatement(gpu, cf))
    kl.each([(1, "e4m3"), (2, "e5m2")], lambda a: f"wave+{a[0]}-{a[1]}", lambda a: wave_form_past_the_threshold_and_the_same_bits_on_both_sides(gpu, *a))
    kl.each([("bf16", "e4m3", 128, "neox"), ("f16", "e5m2", 64, "interleaved")], lambda a: "quantiser-" + "-".join(map(str, a)),
            lambda a: cache_bytes_equal_quantize_rows_fp8_on_ko(gpu, *a))
    kl.each([("bf16", "e4m3", 128, 4), ("f16", "e5m2", 64, 8)], lambda a: "graph-" + "-".join(map(str, a)),
            lambda a: hipgraph_replay_after_lengths_and_table_changed_on_the_device(gpu, *a))
