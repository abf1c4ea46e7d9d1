"""sm_rope_append_{f16,bf16} on the device (-m gpu): RoPE on every Q and K head and the append of K and V to the paged cache, in one launch.

Every case (tests/rope_append_testlib.py: CASES) reads Q, K and V as column slices of one fused buffer at a moved base with every pitch above
its extent, the type's NaN in all input padding and in the rows of padding tokens; Qo, Ko and the WHOLE cache hold a sentinel, a guard page
in front of page 0 and behind the last page included -- the pages an unclamped kernel would address from the ids -1 and num_pages the tables
hold.  Each case asserts its form through the query, runs twice (same bits) and compares EVERY buffer whole with what the float32
restatement of the definition leaves there: Qo, Ko, Kc and Vc bit for bit where the definition writes (NaN by class: canon16), and bit for
bit the uploaded contents everywhere else -- so no input changed unless the call is in place, and nothing outside the logical outputs lost
its sentinel.  The definition fixes every rounding, so there is no tolerance.

Which failure each shape is the smallest to catch -- 1 token: a kernel that needs a full workgroup of tokens; 3, 4, 5 tokens (and BLOCK_MAX + 1
.. + 5 in the WAVE form): a partial, a full and a second four-token workgroup; heads (1, 1), (5, 5), (8, 2), (32, 8), (3, 1): head counts that
do not fill a wave's step and a last partial step; head_dim 64, 128, 256, 40, 96 with rot_dim 0, 16, head_dim / 2 and head_dim in both styles:
every split of a head into rotated pairs and copied pieces, lane counts per head that do not divide 64; positions 0, page_size - 1, page_size,
max_pos - 1: the slot arithmetic and the table's last row; shuffled and interleaved prefills: token order is not slot order; padding by
position, by sequence id and by a zero length: nothing written, the NaN rows never read into an output; the append refused beyond the
capacity, at an absent page and at a sequence id out of range while Q is still written; both decode spellings; in place, out of place at
distinct pitches, without Ko, without a cache; special values (NaN, inf, the zeros, subnormals that an fp32 flush would lose); operands at
which a contracted multiply-add rounds to another 16-bit value (the premise is asserted on the host)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import attn_decode_testlib as al
import rope_append_testlib as rl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", rl.CASES, ids=rl.case_id)
def test_every_buffer_bit_for_bit_against_the_restatement(gpu, case):
    pr, (Q, K, V, cs) = rl.make(case)
    rl.Layout(pr, Q, K, V, cs, torch).twice(gpu, rl.form_of(gpu, pr))


@pytest.mark.parametrize("extra", [1, 2, 3, 4, 5])
def test_wave_form_past_the_threshold_and_the_same_bits_on_both_sides(gpu, extra):
    """BLOCK_MAX + extra tokens run WAVE; the same operands cut to BLOCK_MAX tokens run BLOCK: both equal the restatement, hence each other --
    and the common tokens' Qo rows and cache slots are compared directly as well"""
    B = gpu.ROPE_APPEND_BLOCK_MAX_TOKENS
    case = rl.wave_twin(B, extra)
    pr, (Q, K, V, cs) = rl.make(case)
    assert pr.tokens == B + extra
    lay = rl.Layout(pr, Q, K, V, cs, torch)
    wave = lay.twice(gpu, "wave")
    # the first BLOCK_MAX tokens of the same problem
    cut = rl.Problem.__new__(rl.Problem)
    cut.__dict__.update(pr.__dict__)
    cut.tokens = B
    cut.token_seq, cut.positions, cut.s, cut.pos, cut.live, cut.slot = pr.token_seq[:B], pr.positions[:B], pr.s[:B], pr.pos[:B], pr.live[:B], pr.slot[:B]
    lay2 = rl.Layout(cut, Q[:B], K[:B], V[:B], cs, torch)
    block = lay2.twice(gpu, "block")
    out = "qkv" if lay.inplace else "Qo"
    qi = lambda L: (L.ix["q"] if L.inplace else L.iqo)[:B].reshape(-1)
    assert np.array_equal(wave[out][qi(lay)], block[out][qi(lay2)])
    written = lay2.written["Kc"]
    assert np.array_equal(wave["Kc"][written], block["Kc"][written]) and np.array_equal(wave["Vc"][written], block["Vc"][written])


@pytest.mark.parametrize("ty,hd,group,kvh,ps,ctx", [("bf16", 128, 4, 2, 16, 300), ("f16", 64, 8, 1, 32, 70)])
def test_prefill_then_decode_then_attention_equals_attention_on_a_host_filled_cache(gpu, ty, hd, group, kvh, ps, ctx):
    """prefill ctx - 1 tokens per sequence and one decode token through rope_append, then attn_decode: the output equals attn_decode on a
    cache filled on the host from the restatement, bit for bit (bf16 128/4/2/16 runs the SPLIT form, f16 64/8/1/32 DIRECT)"""
    pkg, seqs, qh = gpu, 2, group * kvh
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
    rng = np.random.default_rng(rl.seed(rl.SALT, "compose", hd))
    lens = [ctx, ctx - ps - 3]
    max_pages = -(-ctx // ps)
    assert pkg.attn_decode_form(seqs, qh, kvh, hd, ps, max_pages) == ("split" if max_pages * ps > pkg.ATTN_DECODE_CHUNK else "direct")
    c = rl.case("compose", ty, qh, kvh, hd, hd, rl.NEOX, toks="interleaved", lens=[str(L - 1) for L in lens], ps=ps, max_pages=str(max_pages), max_pos=str(ctx))
    pr = rl.Problem(c, rng)
    Q, K, V, cs = rl.general(pr, rng)
    dev16 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(dt)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    kc = torch.zeros((pr.num_pages, ps, kvh, hd), dtype=dt, device="cuda")
    vc = torch.zeros_like(kc)
    bt, csd = i32(pr.table), torch.from_numpy(cs).cuda()
    # the table of the prefill has bad ids beyond the prefilled pages: give the decode token's page where it starts a new one
    table = pr.table.copy()
    spare = iter(sorted(set(range(pr.num_pages)) - set(table[(table >= 0) & (table < pr.num_pages)].tolist())))
    for s in range(seqs):
        col = (lens[s] - 1) // ps
        if not 0 <= table[s, col] < pr.num_pages:
            table[s, col] = next(spare)
    bt.copy_(i32(table))
    pkg.rope_append(dev16(Q), dev16(K), dev16(V), csd, block_table=bt, k_cache=kc, v_cache=vc, positions=i32(pr.positions), token_seq=i32(pr.token_seq))
    # the decode step: seq_lens already count the new token
    dq, dk, dv = (al.bits_of(rng.normal(0, 1, (seqs, h, hd)), ty) for h in (qh, kvh, kvh))
    sl = i32(lens)
    q1 = dev16(dq)
    pkg.rope_append(q1, dev16(dk), dev16(dv), csd, block_table=bt, k_cache=kc, v_cache=vc, seq_lens=sl)
    out = pkg.attn_decode(q1, kc, vc, bt, sl)
    torch.cuda.synchronize()
    # the same on the host: the restatement fills a cache, attn_decode reads it
    hk, hv = np.zeros((pr.num_pages, ps, kvh, hd), dtype=np.uint16), np.zeros((pr.num_pages, ps, kvh, hd), dtype=np.uint16)
    ev = rl.evaluate(pr, Q, K, V, cs, np.float32)
    for i in range(pr.tokens):
        pg, slot = table[pr.s[i], pr.pos[i] // ps], pr.pos[i] % ps
        hk[pg, slot], hv[pg, slot] = ev["kbits"][i], V[i]
    dec = rl.Problem.__new__(rl.Problem)
    dec.__dict__.update(pr.__dict__)
    dec.tokens, dec.pos, dec.live = seqs, np.array(lens) - 1, np.ones(seqs, dtype=bool)
    ed = rl.evaluate(dec, dq, dk, dv, cs, np.float32)
    for s in range(seqs):
        hk[table[s, (lens[s] - 1) // ps], (lens[s] - 1) % ps], hv[table[s, (lens[s] - 1) // ps], (lens[s] - 1) % ps] = ed["kbits"][s], dv[s]
    assert np.array_equal(rl.canon16(q1.view(torch.int16).cpu().numpy().view(np.uint16), ty), rl.canon16(ed["qbits"], ty)), "the decode token's rotated Q"
    assert np.array_equal(kc.view(torch.int16).cpu().numpy().view(np.uint16), hk) and np.array_equal(vc.view(torch.int16).cpu().numpy().view(np.uint16), hv)
    want = pkg.attn_decode(dev16(ed["qbits"]), dev16(hk), dev16(hv), bt, sl)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert bool(torch.isfinite(out.float()).all()) and float(out.float().abs().max()) > 0


@pytest.mark.parametrize("ty,hd,group", [("bf16", 128, 4), ("f16", 64, 8)])
def test_hipgraph_replay_after_lengths_and_table_changed_on_the_device(gpu, ty, hd, group):
    """a decode-spelling rope_append followed by attn_decode, captured once; between replays seq_lens grow past a page boundary and block_table
    rows are rewritten ON THE DEVICE; each replay equals the eager pair on the new state bit for bit"""
    pkg, ps, kvh, seqs = gpu, 16, 2, 3
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
    max_pages, qh = 6, group * kvh
    num_pages = seqs * max_pages
    rng = np.random.default_rng(rl.seed(rl.SALT, "graph", hd))
    t16 = lambda a: torch.from_numpy(al.bits_of(a, ty).view(np.int16)).cuda().view(dt)
    qkv = t16(rng.normal(0, 1, (seqs, (qh + 2 * kvh) * hd)))
    q0, k, v = (qkv[:, a * hd:b * hd].view(seqs, -1, hd) for a, b in ((0, qh), (qh, qh + kvh), (qh + kvh, qh + 2 * kvh)))
    cache0 = [t16(rng.normal(0, 1, (num_pages, ps, kvh, hd))) for _ in range(2)]
    cs = pkg.rope_table(max_pages * ps, hd, device="cuda")
    tables = [torch.from_numpy(rng.permutation(num_pages).astype(np.int32).reshape(seqs, max_pages)).cuda() for _ in range(2)]
    states = [([ps - 1, 5, 1], 0), ([ps, ps + 1, 2 * ps + 3], 0), ([ps + 1, 3 * ps, 2 * ps + 4], 1), ([max_pages * ps, 1, ps], 1)]
    bt, sl = tables[0].clone(), torch.zeros(seqs, dtype=torch.int32, device="cuda")

    def pair(qo, kc, vc, out):
        pkg.rope_append(q0, k, v, cs, block_table=bt, k_cache=kc, v_cache=vc, seq_lens=sl, q_out=qo)
        pkg.attn_decode(qo, kc, vc, bt, sl, out=out)
    qo, kc, vc = torch.zeros_like(q0.contiguous()), cache0[0].clone(), cache0[1].clone()
    out = torch.zeros((seqs, qh, hd), dtype=dt, device="cuda")
    sl.copy_(torch.tensor(states[0][0], dtype=torch.int32))
    pair(qo, kc, vc, out)                                              # (warm-up outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        pair(qo, kc, vc, out)
    for lens, which in states:
        sl.copy_(torch.tensor(lens, dtype=torch.int32).cuda())
        bt.copy_(tables[which])
        kc.copy_(cache0[0]), vc.copy_(cache0[1]), qo.fill_(7.0), out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        eq, ekc, evc, eo = torch.zeros_like(qo), cache0[0].clone(), cache0[1].clone(), torch.zeros_like(out)
        pair(eq, ekc, evc, eo)
        torch.cuda.synchronize()
        same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))
        assert same(qo, eq) and same(kc, ekc) and same(vc, evc) and same(out, eo), (lens, which)
        assert not same(kc, cache0[0]) and bool(torch.isfinite(out.float()).all())


def test_cpp_header_mirror(gpu):
    """examples/bin/rope_append: sparsifyme::rope_append and sparsifyme::attn_decode over a permuted page table through the headers; the example
    checks Qo and the cache rows bit for bit against a host loop of the definition and the attention output against attn_decode on a
    host-filled cache, and exits non-zero on a miss."""
    exe = os.path.join(ROOT, "examples", "bin", "rope_append")
    assert os.path.exists(exe), "examples/bin/rope_append is missing: build() makes it"
    for argv in (["3", "8", "2", "128", "300"], ["2", "4", "4", "64", "70"]):
        res = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert res.stdout.count(": yes") == 3 and "NO" not in res.stdout, res.stdout
