"""sm_rope_append_kv8_{f16,bf16} and sm_attn_decode_kv8_{f16,bf16} without a GPU: the four symbols are declared, exported and bound with the
header's arity and prototype, and the two 16-bit sections point to them; every status of both calls is returned before any device work (fake
pointers, never dereferenced) in the order the header states, with a text that names the entry point and the limit; the zero-extent
successes sit behind those checks; the numpy restatements the GPU tests compare the device with (tests/kv8_testlib.py): the decode
definition in float32 against the float64 definition on every case of attn_decode_testlib's table within, per element,
    attn_decode_testlib.bound (A over |vs v8|)  +  (2 2^-24 sabs + 2^-24) A
-- one more 2^-24 in delta for the ks multiply (delta enters twice) and one more 2^-24 in the A term for the p vs multiply: derived from the
definition, not measured --, the append restatement against the definition's own words (dequantised rows within half a step of the format,
the scale rule, an all-zero row, the non-finite bytes), and the premises of the exact classes."""
import ctypes
import os
import re

import numpy as np
import pytest

import attn_decode_testlib as al
import b8_testlib as b8
import kv8_testlib as kl
import rope_append_testlib as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 2
BIG = 1 << 31
RA, AD = b"sm_rope_append_kv8_{f16,bf16}", b"sm_attn_decode_kv8_{f16,bf16}"
RA_NAMES = ["sm_rope_append_kv8_f16", "sm_rope_append_kv8_bf16"]
AD_NAMES = ["sm_attn_decode_kv8_f16", "sm_attn_decode_kv8_bf16"]
# stand-ins for device pointers, all 16-byte aligned and distinct
Q, K, V, QO, KO, KC, VC, KS, VS, CS, POS, TS, SL, BT, O, LSE, WS = (ctypes.c_void_p(0x10000 * (i + 1)) for i in range(17))
P8, P8B, P4 = ctypes.c_void_p(0x90008), ctypes.c_void_p(0xA0008), ctypes.c_void_p(0x90004)          # 8- and 4-byte aligned only


def _err(pkg):
    return pkg.lib().sm_last_error()


def ra(pkg, name="sm_rope_append_kv8_bf16", q=Q, k=K, v=V, qo=QO, ko=KO, kc=KC, vc=VC, ks=KS, vs=VS, cs=CS, pos=POS, ts=TS, sl=SL, bt=BT, tokens=4, seqs=2, q_heads=8,
       kv_heads=2, head_dim=128, rot_dim=128, max_pos=64, num_pages=64, page_size=16, max_pages=4, ldq=None, ldk=None, ldv=None, ldqo=None, ldko=None, ldkv=None,
       page_stride=None, sps=None, ldcs=None, ldbt=None, style=0, fmt=0):
    qw, kw = q_heads * head_dim, kv_heads * head_dim
    d = lambda x, y: y if x is None else x
    ldkv = d(ldkv, kw)
    return getattr(pkg.lib(), name)(q, k, v, qo, ko, kc, vc, ks, vs, cs, pos, ts, sl, bt, tokens, seqs, q_heads, kv_heads, head_dim, rot_dim, max_pos, num_pages,
                                    page_size, max_pages, d(ldq, qw), d(ldk, kw), d(ldv, kw), d(ldqo, qw), d(ldko, kw), ldkv, d(page_stride, page_size * ldkv),
                                    d(sps, kv_heads * page_size), d(ldcs, rot_dim), d(ldbt, max_pages), style, fmt, None)


def ad(pkg, name="sm_attn_decode_kv8_bf16", q=Q, k=KC, v=VC, ks=KS, vs=VS, bt=BT, sl=SL, o=O, lse=LSE, ws=WS, ws_bytes=1 << 62, seqs=2, q_heads=8, kv_heads=2,
       head_dim=128, num_pages=64, page_size=16, max_pages=4, ldq=None, ldkv=None, page_stride=None, sps=None, ldbt=None, ldo=None, scale=1.0, fmt=0):
    d = lambda x, y: y if x is None else x
    ldkv = d(ldkv, kv_heads * head_dim)
    return getattr(pkg.lib(), name)(q, k, v, ks, vs, bt, sl, o, lse, ws, ws_bytes, seqs, q_heads, kv_heads, head_dim, num_pages, page_size, max_pages,
                                    d(ldq, q_heads * head_dim), ldkv, d(page_stride, page_size * ldkv), d(sps, kv_heads * page_size), d(ldbt, max_pages),
                                    d(ldo, q_heads * head_dim), scale, fmt, None)


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    pkg.build()
    L = ctypes.CDLL(pkg.LIB_PATH)
    sz, ci, cf, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    for name in RA_NAMES + AD_NAMES:
        assert name + "(" in header and name in pkg.EXPORTED_SYMBOLS and hasattr(L, name), name
    for name in RA_NAMES:
        assert pkg._SIGS[name] == [vp] * 14 + [sz] * 20 + [ci, ci, vp], name
        proto = re.search(name + r"\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(proto.split(",")) == 37 == len(pkg._SIGS[name])
        assert re.search(r"const void\* Q,\s*const void\* K,\s*const void\* V,\s*void\* Qo,\s*void\* Ko,\s*void\* Kc8,\s*void\* Vc8,\s*float\* Ksc,\s*float\* Vsc,\s*"
                         r"const float\* cs,\s*const int\* positions,\s*const int\* token_seq,\s*const int\* seq_lens,\s*const int\* block_table,\s*size_t tokens,\s*"
                         r"size_t seqs,\s*size_t q_heads,\s*size_t kv_heads,\s*size_t head_dim,\s*size_t rot_dim,\s*size_t max_pos,\s*size_t num_pages,\s*"
                         r"size_t page_size,\s*size_t max_pages,\s*size_t ldq,\s*size_t ldk,\s*size_t ldv,\s*size_t ldqo,\s*size_t ldko,\s*size_t ldkv,\s*"
                         r"size_t page_stride,\s*size_t scale_page_stride,\s*size_t ldcs,\s*size_t ldbt,\s*int style,\s*int fmt,\s*sm_stream_t stream", proto), name
    for name in AD_NAMES:
        assert pkg._SIGS[name] == [vp] * 10 + [sz] * 14 + [cf, ci, vp], name
        proto = re.search(name + r"\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(proto.split(",")) == 27 == len(pkg._SIGS[name])
        assert re.search(r"const void\* Q,\s*const void\* Kc8,\s*const void\* Vc8,\s*const float\* Ksc,\s*const float\* Vsc,\s*const int\* block_table,\s*"
                         r"const int\* seq_lens,\s*void\* O,\s*float\* lse,\s*void\* workspace,\s*size_t workspace_bytes,\s*size_t seqs,\s*size_t q_heads,\s*"
                         r"size_t kv_heads,\s*size_t head_dim,\s*size_t num_pages,\s*size_t page_size,\s*size_t max_pages,\s*size_t ldq,\s*size_t ldkv,\s*"
                         r"size_t page_stride,\s*size_t scale_page_stride,\s*size_t ldbt,\s*size_t ldo,\s*float scale,\s*int fmt,\s*sm_stream_t stream", proto), name
    # no new query: the 16-bit calls' form and workspace queries serve these calls
    assert not [s for s in pkg.EXPORTED_SYMBOLS if "kv8" in s and s not in RA_NAMES + AD_NAMES]
    assert header.index("int sm_rope_append_form(") < header.index("The fp8 paged KV cache") < header.index("int sm_rope_append_kv8_f16(") \
        < header.index("int sm_attn_decode_kv8_f16(") < header.index("fp32 form: the STRIP rule")
    assert callable(pkg.rope_append_kv8) and callable(pkg.attn_decode_kv8)
    # the header states the cache and the two changed lines to the letter, and the 16-bit sections point here
    for text in ("[num_pages][kv_heads][page_size]", "fp32(byte) * Ksc[page][g][slot]", "scale_page_stride >= kv_heads * page_size", "one fmt covers both caches",
                 "sm_quantize_rows_fp8_* gives for the row y[g][0 .. head_dim)", "2^-100", "two correctly rounded fp32 divisions", "writes neither bytes nor scales",
                 "s_t = (dot_t * ks_t) * scale", "acc_c,d = sum_t (fp32(p_t) * vs_t) * fp32(v8_t,d)", "l_c still sums the rounded p_t themselves",
                 "the bytes AND the scales of a masked or absent", "sm_attn_decode_form and sm_attn_decode_workspace_size serve this call too",
                 "sm_rope_append_form serves this call too", "an fp8 cache (that is sm_rope_append_kv8_* below)", "An fp8 cache is sm_attn_decode_kv8_*",
                 "fp8 Q or P on the 1-byte matrix instruction", "different\n *      formats for K and V"):
        assert text in header, text


@pytest.mark.parametrize("name", RA_NAMES)
def test_append_statuses_before_any_device_work_in_the_stated_order(pkg, name):
    c = lambda **kw: ra(pkg, name, **kw)

    def inv(word, **kw):
        assert c(**kw) == INVALID, kw
        assert RA + b": invalid argument" in _err(pkg) and word in _err(pkg), (kw, _err(pkg))

    def uns(word, **kw):
        assert c(**kw) == NOT_SUPPORTED, kw
        assert RA in _err(pkg) and word in _err(pkg), (kw, _err(pkg))
    # 1. INVALID_VALUE, in the header's order
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(qo=None), dict(kc=None), dict(vc=None), dict(ks=None), dict(vs=None), dict(kc=None, vc=None, ks=None, vs=None)):
        inv(b"null Q, K, V, Qo, Kc8, Vc8, Ksc or Vsc", **kw)
    inv(b"null block_table", bt=None)
    inv(b"positions and seq_lens are both null", pos=None, sl=None)
    inv(b"null cs with rot_dim > 0", cs=None)
    for st in (-1, 2, 7):
        inv(b"SM_ROPE_NEOX or SM_ROPE_INTERLEAVED", style=st)
    for kw in (dict(ldq=1016), dict(ldk=248), dict(ldv=248), dict(ldqo=1016), dict(ldko=248), dict(ldkv=240, page_stride=16 * 256), dict(page_stride=16 * 256 - 16),
               dict(ldcs=120), dict(ldbt=3)):
        inv(b"pitch below its extent", **kw)
    for f in (-1, 2, 9):
        inv(b"fmt is SM_FP8_E4M3 or SM_FP8_E5M2", fmt=f)
    for s in (0, 28, 31):
        inv(b"scale_page_stride below kv_heads * page_size", sps=s)
    inv(b"rot_dim exceeds head_dim", rot_dim=144, ldcs=144)
    inv(b"null token_seq with tokens > seqs", ts=None, tokens=3, seqs=2)
    for kw in (dict(qo=K), dict(ko=Q), dict(ko=V), dict(kc=VC), dict(qo=KC), dict(k=Q), dict(qo=Q, ldqo=1032), dict(ko=K, ldko=264), dict(ks=VS), dict(vs=KC),
               dict(ks=QO), dict(vc=V)):
        inv(b"aliased operands", **kw)
    # ... each is answered before the next, and all before every not-supported shape
    inv(b"null Q", q=None, bt=None)
    inv(b"null block_table", bt=None, pos=None, sl=None)
    inv(b"positions and seq_lens", pos=None, sl=None, cs=None)
    inv(b"null cs", cs=None, style=5)
    inv(b"style", style=5, ldq=8)
    inv(b"pitch", ldq=8, fmt=3)
    inv(b"fmt is", fmt=3, sps=1)
    inv(b"scale_page_stride", sps=1, rot_dim=256, ldcs=256)
    inv(b"rot_dim exceeds", rot_dim=256, ldcs=256, ts=None, tokens=9)
    inv(b"token_seq", ts=None, tokens=9, qo=K)
    inv(b"aliased", qo=K, tokens=BIG)
    inv(b"aliased", qo=K, head_dim=96, rot_dim=96, ldkv=192)
    # ... the allowed aliases and spellings pass them (shown by the NOT_SUPPORTED answer behind every INVALID one)
    for kw in (dict(qo=Q), dict(ko=K), dict(qo=Q, ko=K), dict(ko=None), dict(pos=None), dict(sl=None), dict(ts=None, tokens=2), dict(cs=None, rot_dim=0), dict(fmt=1)):
        uns(b"SM_ATTN_DECODE_MIN_HEAD_DIM (64)", head_dim=256, ldq=4096, ldqo=4096, ldk=1024, ldv=1024, ldko=1024, ldkv=1024, **kw)
    # 2. NOT_SUPPORTED: 2^31, then the limits in the listed order
    for kw in (dict(tokens=BIG), dict(seqs=BIG), dict(num_pages=BIG), dict(max_pos=BIG), dict(ldq=BIG), dict(ldk=BIG), dict(ldv=BIG), dict(ldqo=BIG), dict(ldko=BIG),
               dict(ldkv=BIG, page_stride=BIG * 16), dict(page_stride=BIG), dict(sps=BIG), dict(ldcs=BIG), dict(ldbt=BIG), dict(max_pages=1 << 27, ldbt=1 << 27)):
        uns(b"2^31-1", **kw)
    uns(b"2^31-1", tokens=BIG, head_dim=96, rot_dim=96, ldkv=192)
    for hd in (8, 32, 40, 96, 192, 256):
        uns(b"SM_ATTN_DECODE_MAX_HEAD_DIM (128)", head_dim=hd, rot_dim=8, ldcs=8, page_size=8, q=P8, ldq=8 * hd, ldqo=8 * hd, ldk=2 * hd, ldv=2 * hd, ldko=2 * hd, ldkv=2 * hd)
    for rot in (2, 8, 24, 40, 100, 120):
        uns(b"SM_ROPE_APPEND_ROT_DIM_MULTIPLE (16)", rot_dim=rot, ldcs=rot, page_size=8, q=P8)
    for ps in (0, 1, 8, 24, 48, 96, 256, 1024):
        uns(b"SM_ATTN_DECODE_MIN_PAGE_SIZE (16)", page_size=ps, q=P8, max_pages=2)
    for kw in (dict(q=P8), dict(k=P8), dict(v=P8), dict(qo=P8), dict(ko=P8), dict(ldq=1028), dict(ldk=260), dict(ldv=260), dict(ldqo=1036), dict(ldko=260)):
        uns(b"16-byte aligned rows of Q, K, V, Qo and Ko", kc=P8B, cs=P4, **kw)
    for kw in (dict(kc=P8), dict(vc=P8), dict(ks=P8), dict(vs=P4), dict(ldkv=264, page_stride=16 * 264), dict(page_stride=16 * 256 + 8), dict(sps=34)):
        uns(b"16-byte aligned rows of Kc8 and Vc8", cs=P4, **kw)
    for kw in (dict(cs=P8), dict(cs=P4), dict(ldcs=130)):
        uns(b"16-byte aligned rows of cs", **kw)
    # ... what is not read is not checked; every allowed value passes (tokens = 0: nothing is enqueued)
    e = dict(tokens=0)
    assert c(ko=None, ldko=0, **e) == 0 and c(rot_dim=0, cs=None, ldcs=0, max_pos=1 << 40, **e) == 0
    for hd in (64, 128):
        for rot in (r for r in (0, 16, 32, 48, 64, 96, 128) if r <= hd):
            for ps in pkg.ATTN_DECODE_PAGE_SIZES:
                for st in (pkg.ROPE_NEOX, pkg.ROPE_INTERLEAVED):
                    for f in (pkg.FP8_E4M3, pkg.FP8_E5M2):
                        assert c(head_dim=hd, rot_dim=rot, page_size=ps, style=st, fmt=f, **e) == 0, (hd, rot, ps, st, f)
    assert c(sps=36, **e) == 0 and c(ldkv=272, page_stride=16 * 272 + 16, **e) == 0
    # 3. a zero extent: success, nothing enqueued -- but only behind the checks above
    for kw in (dict(tokens=0), dict(q_heads=0, kv_heads=0), dict(tokens=0, seqs=0), dict(tokens=0, max_pages=0), dict(tokens=0, num_pages=0)):
        assert c(**kw) == 0, kw
    assert c(tokens=0, q=None) == INVALID and c(tokens=0, fmt=2) == INVALID and c(tokens=0, kc=P8) == NOT_SUPPORTED and c(tokens=0, head_dim=0, rot_dim=0) == NOT_SUPPORTED


@pytest.mark.parametrize("name", AD_NAMES)
def test_decode_statuses_before_any_device_work_in_the_stated_order(pkg, name):
    c = lambda **kw: ad(pkg, name, **kw)
    C = pkg.ATTN_DECODE_CHUNK
    split = dict(max_pages=C // 16 + 1)

    def inv(word, **kw):
        assert c(**kw) == INVALID, kw
        assert AD + b": invalid argument" in _err(pkg) and word in _err(pkg), (kw, _err(pkg))

    def uns(word, **kw):
        assert c(**kw) == NOT_SUPPORTED, kw
        assert AD in _err(pkg) and word in _err(pkg), (kw, _err(pkg))
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(ks=None), dict(vs=None), dict(bt=None), dict(sl=None), dict(o=None)):
        inv(b"null Q, Kc8, Vc8, Ksc, Vsc, block_table, seq_lens or O", **kw)
    for kw in (dict(ldq=8 * 128 - 8), dict(ldkv=240, page_stride=16 * 256), dict(page_stride=16 * 256 - 16), dict(ldbt=3), dict(ldo=1016)):
        inv(b"pitch below its extent", **kw)
    for f in (-1, 2, 9):
        inv(b"fmt is SM_FP8_E4M3 or SM_FP8_E5M2", fmt=f)
    for s in (0, 28, 31):
        inv(b"scale_page_stride below kv_heads * page_size", sps=s)
    inv(b"kv_heads is 0", kv_heads=0)
    inv(b"multiple of kv_heads", kv_heads=3)
    need = pkg.attn_decode_workspace_size(2, 8, 128, 16, C // 16 + 1)
    for kw in (dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(0x80002))):
        inv(b"workspace", **dict(split, **kw))
    assert c(seqs=0, ws_bytes=0, **split) == 0 and c(ws_bytes=need, seqs=0, **split) == 0 and c(seqs=0, ws=None, ws_bytes=0) == 0
    inv(b"scale is NaN", scale=float("nan"))
    # ... in this order
    inv(b"null", q=None, ldq=8)
    inv(b"pitch", ldq=8, fmt=5)
    inv(b"fmt is", fmt=5, sps=1)
    inv(b"scale_page_stride", sps=16, kv_heads=3, ldkv=384)
    inv(b"kv_heads is 0", kv_heads=0, ldkv=0, page_stride=0, scale=float("nan"))
    inv(b"multiple", kv_heads=3, ws=None, ldkv=384, sps=48, **split)
    inv(b"workspace", ws=None, scale=float("nan"), **split)
    inv(b"scale is NaN", scale=float("nan"), head_dim=96)
    for kw in (dict(seqs=BIG), dict(num_pages=BIG), dict(ldq=BIG), dict(ldkv=BIG, page_stride=BIG * 16), dict(page_stride=BIG), dict(sps=BIG), dict(ldbt=BIG), dict(ldo=BIG),
               dict(max_pages=BIG, ldbt=BIG), dict(seqs=1 << 28, q_heads=8)):
        uns(b"2^31-1", **kw)
    for hd in (0, 8, 32, 96, 192, 256):
        uns(b"SM_ATTN_DECODE_MIN_HEAD_DIM (64)", head_dim=hd, page_size=8, q_heads=34, q=P8)
    for ps in (0, 1, 8, 24, 48, 96, 256, 1024):
        uns(b"SM_ATTN_DECODE_MAX_PAGE_SIZE (128)", page_size=ps, q_heads=34, q=P8, max_pages=2)
    for qh, kvh in ((17, 1), (34, 2), (96, 3)):
        uns(b"SM_ATTN_DECODE_MAX_GROUP (16)", q_heads=qh, kv_heads=kvh, q=P8)
    for ps, mp in ((16, 1 << 27), (128, 1 << 24)):
        uns(b"SM_ATTN_DECODE_MAX_CONTEXT", page_size=ps, max_pages=mp, q=P8)
    for kw in (dict(q=P8), dict(o=P8), dict(ldq=1028), dict(ldo=1036)):
        uns(b"16-byte aligned rows of Q and O", k=P8B, **kw)
    for kw in (dict(k=P8), dict(v=P8), dict(ks=P8), dict(vs=P4), dict(ldkv=264, page_stride=16 * 264), dict(page_stride=16 * 256 + 8), dict(sps=34)):
        uns(b"16-byte aligned rows of Kc8 and Vc8", **kw)
    for hd in pkg.ATTN_DECODE_HEAD_DIMS:
        for ps in pkg.ATTN_DECODE_PAGE_SIZES:
            for qh, kvh in ((1, 1), (5, 1), (16, 1), (32, 2), (3, 3)):
                for f in (pkg.FP8_E4M3, pkg.FP8_E5M2):
                    assert c(seqs=0, head_dim=hd, page_size=ps, q_heads=qh, kv_heads=kvh, fmt=f) == 0, (hd, ps, qh, kvh, f)
    assert c(seqs=0, lse=None, ldbt=7, sps=36) == 0
    for kw in (dict(seqs=0), dict(q_heads=0), dict(q_heads=0, kv_heads=0), dict(seqs=0, max_pages=0)):
        assert c(**kw) == 0, kw
    assert c(seqs=0, q=None) == INVALID and c(seqs=0, fmt=2) == INVALID and c(seqs=0, k=P8) == NOT_SUPPORTED and c(q_heads=0, page_size=8) == NOT_SUPPORTED


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("case", al.CASES, ids=al.case_id)
def test_decode_restatement_in_fp32_against_the_fp64_definition_within_the_bound(pkg, case):
    n = al.CASES.index(case)
    fmt = kl.FMTS[n % 2]
    rng = np.random.default_rng(kl.seed(kl.SALT, "restate", n))
    pr = al.Problem(case, pkg.ATTN_DECODE_CHUNK, rng)
    for sigma, mult in ((1.0, 1.0), (30.0, 8.0)):
        Qb, K8, V8, Ks, Vs = kl.general(pr, rng, sigma, fmt)
        scale = mult * pr.hd ** -0.5
        ob, lse = kl.restate32(pr, Qb, K8, V8, Ks, Vs, scale, fmt)
        ro, rlr = kl.worst_ratios(pr, ob, lse, Qb, K8, V8, Ks, Vs, scale, fmt)
        print(f"restatement {al.case_id(case)} {fmt} sigma {sigma:g} x{mult:g}: O {ro:.3f}, lse {rlr:.3f} of the bound")
        assert ro <= 1.0 and rlr <= 1.0, (ro, rlr)


@pytest.mark.parametrize("fmt", kl.FMTS)
@pytest.mark.parametrize("case", al.CASES[:6], ids=al.case_id)
def test_premises_of_the_exact_classes(pkg, case, fmt):
    """one-hot: the restatement gives the expected bits; uniform: likewise (the builders assert their own premises: exact K, exact integers,
    7 * 4 * L < 2^24)"""
    rng = np.random.default_rng(kl.seed(kl.SALT, "exact", al.CASES.index(case)))
    pr = al.Problem(case, pkg.ATTN_DECODE_CHUNK, rng)
    Qb, K8, V8, Ks, Vs, _, want, wl = kl.one_hot(pr, rng, fmt)
    ob, lse = kl.restate32(pr, Qb, K8, V8, Ks, Vs, 1.0, fmt)
    assert np.array_equal(ob, want) and np.array_equal(lse, wl)
    Qb, K8, V8, Ks, Vs, want, wl = kl.uniform(pr, rng, fmt)
    ob, lse = kl.restate32(pr, Qb, K8, V8, Ks, Vs, pr.hd ** -0.5, fmt)
    assert np.array_equal(ob, want)
    fin = np.isfinite(wl)
    assert np.array_equal(np.isneginf(lse), ~fin) and np.all(np.abs(lse[fin] - wl[fin]) <= 2 * np.spacing(np.abs(wl[fin]).astype(np.float32)))
    for f in kl.FMTS:
        fb = kl.finite_bytes(f)
        assert fb.size == {"e4m3": 254, "e5m2": 248}[f]
        # every finite byte is a value of fp16 and of bf16: the widening the kernel relies on
        v = kl.val32(fb, f)
        assert np.array_equal(kl.f32_of(kl.rne16(v, "f16"), "f16"), v) and np.array_equal(kl.f32_of(kl.rne16(v, "bf16"), "bf16"), v)


def test_append_restatement_states_the_per_row_rule(pkg):
    """the restated append on the special rows and on general data: the scale is max(amax, 2^-100) / FMAX, a finite row dequantises to within
    half a step of the format, an all-zero row has zero bytes that keep their sign, NaN and inf become the stated bytes"""
    for c, fmt in [cf for cf in kl.append_cases() if cf[0]["data"] in ("special_rows", "general")][-8:]:
        pr, (Qb, Kb, Vb, cs) = kl.make_append(c)
        kbits, kq, ks, vq, vs = kl.append_restated(pr, Kb, Vb, cs, fmt)
        live = np.flatnonzero(pr.live)
        for bits, q, sc in ((kbits[live], kq[live], ks[live]), (Vb[live], vq[live], vs[live])):
            x = kl.f32_of(bits, pr.ty).astype(np.float64)
            fin = np.isfinite(x)
            amax = np.where(fin, np.abs(x), 0).max(axis=2)
            assert np.array_equal(sc, (np.maximum(amax, 2.0 ** -100).astype(np.float32) / np.float32(b8.FMAX[fmt])).astype(np.float32))
            deq = kl.val32(q, fmt).astype(np.float64) * sc[..., None]
            step = kl.RSTEP[fmt] * np.maximum(np.abs(x), amax[..., None] * 2.0 ** -6 / 1.75)     # half a step, relative; subnormals of the format below
            with np.errstate(invalid="ignore"):
                assert np.all(np.abs(deq - x)[fin] <= step[fin] + 2.0 ** -120)
            zero = (bits & 0x7FFF) == 0
            assert np.array_equal(q[zero], (bits[zero] >> 8).astype(np.uint8))                 # +0 -> 0x00, -0 -> 0x80
            assert np.all(q[np.isnan(x)] == 0x7F)
            assert np.all(q[np.isinf(x)] == (0x7F if fmt == "e4m3" else np.where(x[np.isinf(x)] < 0, 0xFC, 0x7C)))


def test_append_case_table_covers_what_the_kernel_switches_on(pkg):
    cases = kl.append_cases()
    assert len({kl.append_case_id(cf) for cf in cases}) == len(cases)
    combos = {(c["ty"], fmt, c["hd"], c["style"]) for c, fmt in cases}
    assert combos == {(ty, f, hd, st) for ty in rl.TYPES for f in kl.FMTS for hd in (64, 128) for st in (rl.NEOX, rl.INTERLEAVED)}
    items = {c["rot"] // 16 + (c["hd"] - c["rot"]) // 8 if c["style"] == rl.NEOX else c["hd"] // 8 for c, _ in cases}
    assert {4, 6, 7, 8, 12, 15, 16} <= items, items                  # lanes per head, powers of two and not
    assert {c["rot"] for c, _ in cases} >= {0, 16, 32, 64, 128}
    assert {"decode", "decode_pos", "seq_only", "prefill"} == {c["spelling"] for c, _ in cases} and {"inplace", "out", "ko_null"} == {c["alias"] for c, _ in cases}
    assert any(c["absent"] for c, _ in cases) and {"general", "special", "special_rows"} == {c["data"] for c, _ in cases}


def test_one_hot_targets_cover_every_finite_byte(pkg):
    """the premise of the GPU one-hot class's widening claim (same seeds as tests/test_gpu_kv8_decode.py): over the case table, the expected
    target rows hold every finite byte of both formats"""
    for fmt in kl.FMTS:
        seen = set()
        for n, case in enumerate(al.CASES):
            rng = np.random.default_rng(kl.seed(kl.SALT, "exact", n))
            pr = al.Problem(case, pkg.ATTN_DECODE_CHUNK, rng)
            _, _, V8, _, _, targets, _, _ = kl.one_hot(pr, rng, fmt)
            for (s, h), (pg, slot, _) in targets.items():
                seen.update(V8[pg, slot, h // pr.group].tolist())
        assert seen == set(kl.finite_bytes(fmt).tolist()), fmt
