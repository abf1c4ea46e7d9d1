"""sm_attn_decode_kv8_{f16,bf16} on the device (-m gpu): single-query attention over the fp8 paged KV cache.

The cases are attn_decode_testlib.CASES, the 16-bit test's own -- DIRECT and SPLIT, both group classes, both head dims, page sizes 16 / 32 /
128, absent pages inside the live range, every page absent, clamped and negative lengths, shared prefix pages, L = 0 -- on a host-filled
cache where the test chooses bytes and scales (tests/kv8_testlib.py: DecodeLayout): operands at moved bases with pitches above their
extents, NaN BYTES (0x7f) and NaN SCALES in every slot at or beyond L of a sequence's last page, in every page no table refers to and in a
guard page in front of page 0 and behind the last page of the bytes and of the scales: a kernel that loads a masked token's byte or scale
shows NaN, it does not fault.  O, lse and the workspace sit between sentinel words; each case asserts its form through sm_attn_decode_form,
runs twice (same bits) and checks that no input and nothing outside the outputs changed.

One-hot class (addressing and the widening, bit for bit): attn_decode_testlib.one_hot's Q and K (K entries 0 and 4 are exact bytes), ks a
power of two in 1 .. 4, V running over EVERY finite byte of the format, vs a power of two in 2^-2 .. 2^2: O = rne16(fp32(v8) vs) of the target
row and lse = 128 ks, exactly.  Uniform class (reduction and combine, bit for bit): Q = 0, V integers |v| <= 7, vs a per-token power of two:
every partial sum is exact in any order (7 * 4 * L < 2^24, asserted).  The K-side widening over every finite byte: L = 1 and q = one unit
vector, so lse = (fp32(k8) ks) scale exactly.  General data -- rows of N(0, 1) and N(0, sigma) as the quantiser leaves them -- against the
fp64 definition at the device's bytes and scales within attn_decode_testlib.bound with A over |vs v8| and two further 2^-24 terms
(kv8_testlib.bound); every case prints its worst error as a share of the bound before it asserts.  The pipeline case goes prefill ->
decode step -> attention through the fp8 cache, and RECORDS (no assertion, no tolerance) how far the result is from the 16-bit call on the
unquantised cache, in units of A times the format's relative step.

The file is TWO test items, which walk the classes below over their case tables (kv8_testlib.each) and report the failed cases together,
each under its id; the premise that the one-hot targets cover every finite byte is held without a device (tests/test_kv8_abi.py)."""
import numpy as np
import pytest
import torch

import attn_decode_testlib as al
import b8_testlib as b8
import guard_testlib as gl
import kv8_testlib as kl
import parity_testlib as pl
import rope_append_testlib as rl

pytestmark = pytest.mark.gpu

_margin_report = gl.margin_report_fixture("attn_decode_kv8: worst error / bound of {n} comparisons (O and lse of every general-data case and of the pipeline case; the "
                                          "lines marked RECORD are the distance to the 16-bit call in units of A R, not held to anything), worst first")
CF = [(c, f) for c in al.CASES for f in kl.FMTS]
ALT = [(c, kl.FMTS[n % 2]) for n, c in enumerate(al.CASES)]
cf_id = lambda cf: al.case_id(cf[0]) + "-" + cf[1]


def problem(pkg, case, what):
    rng = np.random.default_rng(kl.seed(kl.SALT, what, al.CASES.index(case)))
    return al.Problem(case, pkg.ATTN_DECODE_CHUNK, rng), rng


def one_hot_class_bit_for_bit(gpu, cf):
    case, fmt = cf
    pr, rng = problem(gpu, case, "exact")
    Q, K8, V8, Ks, Vs, targets, want, wl = kl.one_hot(pr, rng, fmt)
    ob, lse = kl.DecodeLayout(pr, Q, K8, V8, Ks, Vs, fmt, torch).twice(gpu, 1.0, al.form_of(pr))
    bad = np.argwhere(ob != want)
    assert bad.size == 0, f"O is not rne16(fp32(v8) vs) of the target row at (sequence, head, dim) {bad[:4].tolist()}; targets {[targets.get((b[0], b[1])) for b in bad[:4]]}"
    assert np.array_equal(lse, wl), "lse is not 128 ks (-inf for a sequence without a present token)"


def uniform_class_bit_for_bit(gpu, cf):
    case, fmt = cf
    pr, rng = problem(gpu, case, "uniform")
    Q, K8, V8, Ks, Vs, want, wl = kl.uniform(pr, rng, fmt)
    ob, lse = kl.DecodeLayout(pr, Q, K8, V8, Ks, Vs, fmt, torch).twice(gpu, pr.hd ** -0.5, al.form_of(pr))
    bad = np.argwhere(ob != want)
    assert bad.size == 0, f"O is not rne16(sum vs v / T) at (sequence, head, dim) {bad[:4].tolist()}: {ob[tuple(bad[0])]:#x} for {want[tuple(bad[0])]:#x}"
    fin = np.isfinite(wl)
    assert np.array_equal(np.isneginf(lse), ~fin), "lse = -inf exactly where no token is present"
    assert np.all(np.abs(lse[fin].astype(np.float64) - wl[fin]) <= 2 * np.spacing(np.abs(wl[fin]).astype(np.float32))), "lse is not logf(T) within 2 ulp"
    for s in range(pr.seqs):
        if pr.tokens(s)[0].size == 0:
            assert not ob[s].any(), "no present token: O = +0"


def widening_of_every_byte_on_both_sides(gpu, ty, fmt, hd):
    """16 sequences of one token, 2 kv heads, group 8: q of (s, h) is one unit vector at a dim of its own, K's byte there is one of the format's
    finite bytes -- all of them over the 256 (s, h) -- so lse = (fp32(k8) ks) scale exactly; V holds all 256 bytes, the non-finite ones included,
    and O = rne16(fp32(v8) vs) (NaN by class): the K-side widening to Q's type and the V-side widening to fp32 are exact"""
    seqs, kvh, group, ps = 16, 2, 8, 16
    pr = al.Problem(al.case(ty, hd, group, kvh, ps, ["1"] * seqs, "1"), gpu.ATTN_DECODE_CHUNK, np.random.default_rng(kl.seed(kl.SALT, "widen", hd)))
    rng = np.random.default_rng(kl.seed(kl.SALT, "widen-data", hd))
    fb = kl.finite_bytes(fmt)
    Q = np.zeros((seqs, kvh * group, hd), dtype=np.float32)
    K8 = b8.finite_bytes(rng, (pr.num_pages, ps, kvh, hd), fmt)
    V8 = rng.integers(0, 256, (pr.num_pages, ps, kvh, hd)).astype(np.uint8)
    Ks, Vs = kl.pow2_scales(pr, rng, -3, 3), kl.pow2_scales(pr, rng, -2, 2)
    want_l = np.zeros((seqs, kvh * group), dtype=np.float32)
    want_o = np.zeros((seqs, kvh * group, hd), dtype=np.uint16)
    scale = np.float32(0.5)
    for s in range(seqs):
        pg = int(pr.table[s, 0])
        V8[pg, 0, :, :] = np.roll(np.arange(256, dtype=np.uint8), 37 * s)[:kvh * hd].reshape(kvh, hd)
        for h in range(kvh * group):
            kv, d = h // group, (h * 17 + s * 5 + 3) % hd
            Q[s, h, d] = 1.0
            K8[pg, 0, kv, d] = fb[(s * kvh * group + h) % fb.size]
            want_l[s, h] = (kl.val32(K8[pg, 0, kv, d:d + 1], fmt)[0] * Ks[pg, kv, 0]) * scale + np.float32(0.0)      # (a -0 byte sums to +0)
            with np.errstate(all="ignore"):
                want_o[s, h] = kl.rne16((kl.val32(V8[pg, 0, kv], fmt) * Vs[pg, kv, 0]).astype(np.float32) + np.float32(0.0), ty)
    # (h * 17 + s * 5 + 3) % hd is distinct over the 8 heads of a group: a K row's designated bytes do not overwrite each other
    assert all(len({(h * 17 + s * 5 + 3) % hd for h in range(kv * group, (kv + 1) * group)}) == group for s in range(seqs) for kv in range(kvh))
    ob, lse = kl.DecodeLayout(pr, al.bits_of(Q, ty), K8, V8, Ks, Vs, fmt, torch).twice(gpu, float(scale), "direct")
    assert np.array_equal(lse.view(np.uint32), want_l.view(np.uint32)), "lse is not (fp32(k8) ks) scale: the K-side widening is not exact"
    assert np.array_equal(rl.canon16(ob, ty), rl.canon16(want_o, ty)), "O is not rne16(fp32(v8) vs): the V-side widening is not exact"
    assert rl.is_nan16(want_o, ty).any() and (fmt == "e4m3" or np.isinf(kl.f32_of(want_o, ty)).any())


def general_data_within_the_bound(gpu, cf):
    case, fmt = cf
    pr, rng = problem(gpu, case, "general")
    for sigma, mult in ((0.01, 1.0), (1.0, 1.0), (30.0, 1.0), (1.0, 8.0)):
        Q, K8, V8, Ks, Vs = kl.general(pr, rng, sigma, fmt)
        scale = mult * pr.hd ** -0.5
        ob, lse = kl.DecodeLayout(pr, Q, K8, V8, Ks, Vs, fmt, torch).twice(gpu, scale, al.form_of(pr))
        ro, rlr = kl.worst_ratios(pr, ob, lse, Q, K8, V8, Ks, Vs, scale, fmt)
        what = f"{cf_id(cf)} sigma {sigma:g} scale x{mult:g} {al.form_of(pr)}"
        print(f"margin attn_decode_kv8 {what}: O {ro:.3f}, lse {rlr:.3f} of the bound")
        pl.MARGINS.append((f"attn_decode_kv8 O {what}", ro))
        pl.MARGINS.append((f"attn_decode_kv8 lse {what}", rlr))
        assert ro <= 1.0, f"O: error {ro:.3f} of the bound"
        assert rlr <= 1.0, f"lse: error {rlr:.3f} of the bound"


def a_sequence_alone_equals_the_sequence_among_five(gpu, ty, fmt, hd, group, kvh, ps):
    """the same table row at batch position 3 of 5 and alone: the same bits (the chunk does not depend on seqs)"""
    five = al.case(ty, hd, group, kvh, ps, ["17", "C+1", "P-1", "2*C+3", "C"], "2*C//P+1")
    rng = np.random.default_rng(kl.seed(kl.SALT, "alone", hd, group, ps))
    pr5 = al.Problem(five, gpu.ATTN_DECODE_CHUNK, rng)
    Q, K8, V8, Ks, Vs = kl.general(pr5, rng, 1.0, fmt)
    o5, l5 = kl.DecodeLayout(pr5, Q, K8, V8, Ks, Vs, fmt, torch).twice(gpu, hd ** -0.5, "split")
    for s in (3, 1, 0):
        one = al.Problem(al.case(ty, hd, group, kvh, ps, [five["lens"][s]], five["max_pages"]), gpu.ATTN_DECODE_CHUNK, np.random.default_rng(1))
        one.num_pages, one.table = pr5.num_pages, pr5.table[s:s + 1].copy()
        o1, l1 = kl.DecodeLayout(one, Q[s:s + 1], K8, V8, Ks, Vs, fmt, torch).run(gpu, hd ** -0.5, "split")
        assert np.array_equal(o1[0], o5[s]) and np.array_equal(l1[0].view(np.uint32), l5[s].view(np.uint32)), f"sequence {s} depends on the sequences that ride along"


def prefill_then_decode_then_attention_through_the_fp8_cache(gpu, ty, fmt, hd, group, kvh, ps, ctx):
    """prefill ctx - 1 tokens per sequence and one decode token through rope_append_kv8, then attn_decode_kv8: the bytes and scales the device
    wrote equal the restatement bit for bit, and the attention output is within the bound of the fp64 definition evaluated ON those bytes and
    scales.  Recorded beside it, held to nothing: how far that output is from attn_decode on the unquantised 16-bit cache."""
    pkg, seqs, qh = gpu, 2, group * kvh
    dt = {"f16": torch.float16, "bf16": torch.bfloat16}[ty]
    rng = np.random.default_rng(kl.seed(kl.SALT, "compose", hd))
    lens = [ctx, ctx - ps - 3]
    max_pages = -(-ctx // ps)
    form = "split" if max_pages * ps > pkg.ATTN_DECODE_CHUNK else "direct"
    assert pkg.attn_decode_form(seqs, qh, kvh, hd, ps, max_pages) == form
    c = rl.case("compose", ty, qh, kvh, hd, hd, rl.NEOX, toks="interleaved", lens=[str(L - 1) for L in lens], ps=ps, max_pages=str(max_pages), max_pos=str(ctx))
    pr = rl.Problem(c, rng)
    Q, K, V, cs = rl.general(pr, rng)
    dev16 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(dt)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()
    shape = (pr.num_pages, ps, kvh, hd)
    kc8, vc8 = (torch.zeros(shape, dtype=torch.uint8, device="cuda").view(b8.tdt(fmt)) for _ in range(2))
    ksc, vsc = (torch.zeros((pr.num_pages, kvh, ps), dtype=torch.float32, device="cuda") for _ in range(2))
    kc16, vc16 = (torch.zeros(shape, dtype=dt, device="cuda") for _ in range(2))
    csd = torch.from_numpy(cs).cuda()
    # the table of the prefill has bad ids beyond the prefilled pages: give the decode token's page where it starts a new one
    table = pr.table.copy()
    spare = iter(sorted(set(range(pr.num_pages)) - set(table[(table >= 0) & (table < pr.num_pages)].tolist())))
    for s in range(seqs):
        col = (lens[s] - 1) // ps
        if not 0 <= table[s, col] < pr.num_pages:
            table[s, col] = next(spare)
    bt = i32(table)
    pos, ts = i32(pr.positions), i32(pr.token_seq)
    pkg.rope_append_kv8(dev16(Q), dev16(K), dev16(V), csd, bt, kc8, vc8, ksc, vsc, positions=pos, token_seq=ts)
    pkg.rope_append(dev16(Q), dev16(K), dev16(V), csd, block_table=bt, k_cache=kc16, v_cache=vc16, positions=pos, token_seq=ts)
    # the decode step: seq_lens already count the new token
    dq, dk, dv = (al.bits_of(rng.normal(0, 1, (seqs, h, hd)), ty) for h in (qh, kvh, kvh))
    sl = i32(lens)
    q8, q16 = dev16(dq), dev16(dq)
    pkg.rope_append_kv8(q8, dev16(dk), dev16(dv), csd, bt, kc8, vc8, ksc, vsc, seq_lens=sl)
    pkg.rope_append(q16, dev16(dk), dev16(dv), csd, block_table=bt, k_cache=kc16, v_cache=vc16, seq_lens=sl)
    lse = torch.zeros((seqs, qh), dtype=torch.float32, device="cuda")
    out8 = pkg.attn_decode_kv8(q8, kc8, vc8, ksc, vsc, bt, sl, lse=lse)
    out16 = pkg.attn_decode(q16, kc16, vc16, bt, sl)
    torch.cuda.synchronize()
    # the same cache on the host, from the restatement
    hk, hv = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)
    hks, hvs = np.zeros((pr.num_pages, kvh, ps), dtype=np.float32), np.zeros((pr.num_pages, kvh, ps), dtype=np.float32)
    _, kq, ks, vq, vs = kl.append_restated(pr, K, V, cs, fmt)
    dec = rl.Problem.__new__(rl.Problem)
    dec.__dict__.update(pr.__dict__)
    dec.tokens, dec.pos, dec.live = seqs, np.array(lens) - 1, np.ones(seqs, dtype=bool)
    dqbits = rl.evaluate(dec, dq, dk, dv, cs, np.float32)["qbits"]
    _, dkq, dks, dvq, dvs = kl.append_restated(dec, dk, dv, cs, fmt)
    rows = [(table[pr.s[i], pr.pos[i] // ps], pr.pos[i] % ps, kq[i], ks[i], vq[i], vs[i]) for i in range(pr.tokens)]
    rows += [(table[s, (lens[s] - 1) // ps], (lens[s] - 1) % ps, dkq[s], dks[s], dvq[s], dvs[s]) for s in range(seqs)]
    for pg, slot, a, b, c_, d in rows:
        hk[pg, slot], hks[pg, :, slot], hv[pg, slot], hvs[pg, :, slot] = a, b, c_, d
    u8 = lambda t: t.view(torch.uint8).cpu().numpy()
    assert np.array_equal(rl.canon16(q8.view(torch.int16).cpu().numpy().view(np.uint16), ty), rl.canon16(dqbits, ty)), "the decode token's rotated Q"
    assert torch.equal(q8.view(torch.int16), q16.view(torch.int16)), "Qo differs from sm_rope_append_*'s"
    assert np.array_equal(u8(kc8), hk) and np.array_equal(u8(vc8), hv), "cache bytes"
    assert np.array_equal(ksc.cpu().numpy().view(np.uint32), hks.view(np.uint32)) and np.array_equal(vsc.cpu().numpy().view(np.uint32), hvs.view(np.uint32)), "cache scales"
    # against the fp64 definition on the bytes and scales the device wrote
    apr = al.Problem(al.case(ty, hd, group, kvh, ps, [str(L) for L in lens], str(max_pages)), pkg.ATTN_DECODE_CHUNK, np.random.default_rng(1))
    apr.num_pages, apr.table = pr.num_pages, table
    ob = out8.view(torch.int16).cpu().numpy().view(np.uint16)
    scale = hd ** -0.5
    ro, rlr = kl.worst_ratios(apr, ob, lse.cpu().numpy(), dqbits, hk, hv, hks, hvs, scale, fmt)
    what = f"pipeline {ty} {fmt} d{hd} g{group} p{ps} context {ctx} {form}"
    print(f"margin attn_decode_kv8 {what}: O {ro:.3f}, lse {rlr:.3f} of the bound")
    pl.MARGINS.append((f"attn_decode_kv8 O {what}", ro))
    pl.MARGINS.append((f"attn_decode_kv8 lse {what}", rlr))
    # the accuracy record: no assertion, no tolerance
    _, _, A, _, _ = kl.evaluate(apr, dqbits, hk, hv, hks, hvs, scale, fmt, np.float64)
    diff = np.abs(kl.f32_of(ob, ty).astype(np.float64) - out16.float().cpu().numpy().astype(np.float64))
    rec = float((diff / (A * kl.RSTEP[fmt])).max())
    print(f"record attn_decode_kv8 {what}: worst |O_kv8 - O_16bit| / (A R) = {rec:.3f}, R = {kl.RSTEP[fmt]:g}")
    pl.MARGINS.append((f"attn_decode_kv8 RECORD |O_kv8 - O_16bit| / (A R), R {kl.RSTEP[fmt]:g}, {what}", rec))
    assert ro <= 1.0, f"O: error {ro:.3f} of the bound"
    assert rlr <= 1.0, f"lse: error {rlr:.3f} of the bound"
    assert bool(torch.isfinite(out8.float()).all()) and float(out8.float().abs().max()) > 0


def cpp_header_mirror(gpu):
    """examples/bin/kv8_decode: sparsifyme::rope_append_kv8 and sparsifyme::attn_decode_kv8 over a permuted page table through the headers; the
    example checks the cache's bytes and scales bit for bit against a host loop of the definition and the attention output against a host
    fp64 softmax over the dequantised cache, and exits non-zero on a miss."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "bin", "kv8_decode")
    assert os.path.exists(exe), "examples/bin/kv8_decode is missing: build() makes it"
    for argv in (["3", "8", "2", "128", "300", "e4m3"], ["2", "4", "4", "64", "70", "e5m2"]):
        res = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert res.stdout.count(": yes") == 4 and "NO" not in res.stdout, res.stdout


def test_decode_attention_on_a_host_filled_cache(gpu):
    """ONE test item walks every class above over its case table and reports the failed cases together, each under its id."""
    join = lambda a: "-".join(map(str, a))
    kl.each(CF, lambda cf: "one-hot " + cf_id(cf), lambda cf: one_hot_class_bit_for_bit(gpu, cf))
    kl.each(ALT, lambda cf: "uniform " + cf_id(cf), lambda cf: uniform_class_bit_for_bit(gpu, cf))
    kl.each([("f16", "e4m3", 128), ("bf16", "e4m3", 64), ("f16", "e5m2", 64), ("bf16", "e5m2", 128)], lambda a: "widening " + join(a),
            lambda a: widening_of_every_byte_on_both_sides(gpu, *a))
    kl.each(ALT, lambda cf: "general " + cf_id(cf), lambda cf: general_data_within_the_bound(gpu, cf))
    kl.each([("bf16", "e4m3", 128, 4, 2, 16), ("f16", "e5m2", 64, 8, 1, 32), ("bf16", "e5m2", 128, 16, 1, 128)], lambda a: "alone " + join(a),
            lambda a: a_sequence_alone_equals_the_sequence_among_five(gpu, *a))


def test_pipeline_through_the_fp8_cache_and_the_header_mirror(gpu):
    kl.each([("bf16", "e4m3", 128, 4, 2, 16, 300), ("f16", "e5m2", 64, 8, 1, 32, 70)], lambda a: "pipeline " + "-".join(map(str, a)),
            lambda a: prefill_then_decode_then_attention_through_the_fp8_cache(gpu, *a))
    cpp_header_mirror(gpu)
