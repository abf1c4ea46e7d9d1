"""sm_attn_decode_{f16,bf16}, sm_attn_decode_workspace_size and sm_attn_decode_form without a GPU: the four symbols are declared, exported and
bound with the header's arity, the #defines match the package's constants and the header states the definition and what is not covered;
every status is returned before any device work (fake pointers, never dereferenced) in the order the header states, with a text that names
the entry point and the limit; the zero-extent successes sit behind those checks; the form and the workspace size on both sides of
max_pages * page_size = CHUNK and at every allowed and refused head_dim, page_size and group, the size against its formula restated; and the
numpy restatement the GPU test uses (tests/attn_decode_testlib.py): the fp32 restatement -- chunked, p rounded, ascending combine -- against
the fp64 definition on EVERY general-data case of the GPU table within that case's bound (so the bound is shown sufficient here, without a
device), and both exact classes bit for bit through the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

import attn_decode_testlib as al

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 2
BIG = 1 << 31
WHO = b"sm_attn_decode_{f16,bf16}"
NAMES = ["sm_attn_decode_f16", "sm_attn_decode_bf16"]
# stand-ins for device pointers, all 16-byte aligned and distinct
Q, K, V, BT, SL, O, LSE, WS = (ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8))
SIGMAS = (0.01, 1.0, 30.0)


def _err(pkg):
    return pkg.lib().sm_last_error()


def call(pkg, name="sm_attn_decode_bf16", q=Q, k=K, v=V, bt=BT, sl=SL, o=O, lse=LSE, ws=WS, ws_bytes=1 << 62, seqs=2, q_heads=8, kv_heads=2, head_dim=128,
         num_pages=64, page_size=16, max_pages=4, ldq=None, ldkv=None, page_stride=None, ldbt=None, ldo=None, scale=1.0):
    ldq = q_heads * head_dim if ldq is None else ldq
    ldkv = kv_heads * head_dim if ldkv is None else ldkv
    page_stride = page_size * ldkv if page_stride is None else page_stride
    return getattr(pkg.lib(), name)(q, k, v, bt, sl, o, lse, ws, ws_bytes, seqs, q_heads, kv_heads, head_dim, num_pages, page_size, max_pages, ldq, ldkv,
                                    page_stride, max_pages if ldbt is None else ldbt, q_heads * head_dim if ldo is None else ldo, scale, None)


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    pkg.build()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES + ["sm_attn_decode_form", "sm_attn_decode_workspace_size"]:
        assert name + "(" in header and name in pkg.EXPORTED_SYMBOLS and hasattr(L, name), name
    sz, ci, cf, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    for name in NAMES:
        assert pkg._SIGS[name] == [vp] * 8 + [sz] * 13 + [cf, vp], name
        proto = re.search(name + r"\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(proto.split(",")) == 23 == len(pkg._SIGS[name])
        assert re.search(r"const void\* Q,\s*const void\* Kc,\s*const void\* Vc,\s*const int\* block_table,\s*const int\* seq_lens,\s*void\* O,\s*float\* lse,\s*"
                         r"void\* workspace,\s*size_t workspace_bytes,\s*size_t seqs,\s*size_t q_heads,\s*size_t kv_heads,\s*size_t head_dim,\s*size_t num_pages,\s*"
                         r"size_t page_size,\s*size_t max_pages,\s*size_t ldq,\s*size_t ldkv,\s*size_t page_stride,\s*size_t ldbt,\s*size_t ldo,\s*float scale,\s*"
                         r"sm_stream_t stream", proto), name
    assert re.search(r"int sm_attn_decode_workspace_size\(size_t seqs,\s*size_t q_heads,\s*size_t head_dim,\s*size_t page_size,\s*size_t max_pages,\s*size_t\* bytes\);", header)
    assert re.search(r"int sm_attn_decode_form\(size_t seqs,\s*size_t q_heads,\s*size_t kv_heads,\s*size_t head_dim,\s*size_t page_size,\s*size_t max_pages,\s*int\* form\);",
                     header)
    assert len(pkg._SIGS["sm_attn_decode_workspace_size"]) == 6 and len(pkg._SIGS["sm_attn_decode_form"]) == 7
    for k, v in (("SM_ATTN_DECODE_FORM_INVALID", 0), ("SM_ATTN_DECODE_FORM_EMPTY", 1), ("SM_ATTN_DECODE_FORM_DIRECT", 2), ("SM_ATTN_DECODE_FORM_SPLIT", 3),
                 ("SM_ATTN_DECODE_CHUNK", pkg.ATTN_DECODE_CHUNK), ("SM_ATTN_DECODE_MIN_HEAD_DIM", min(pkg.ATTN_DECODE_HEAD_DIMS)),
                 ("SM_ATTN_DECODE_MAX_HEAD_DIM", max(pkg.ATTN_DECODE_HEAD_DIMS)), ("SM_ATTN_DECODE_MIN_PAGE_SIZE", min(pkg.ATTN_DECODE_PAGE_SIZES)),
                 ("SM_ATTN_DECODE_MAX_PAGE_SIZE", max(pkg.ATTN_DECODE_PAGE_SIZES)), ("SM_ATTN_DECODE_MAX_GROUP", pkg.ATTN_DECODE_MAX_GROUP),
                 ("SM_ATTN_DECODE_MAX_CONTEXT", pkg.ATTN_DECODE_MAX_CONTEXT)):
        assert re.search(r"#define %s %d\b" % (k, v), header), k
    assert pkg.ATTN_DECODE_FORMS == ("invalid", "empty", "direct", "split") and pkg.ATTN_DECODE_HEAD_DIMS == (64, 128)
    assert pkg.ATTN_DECODE_PAGE_SIZES == (16, 32, 64, 128) and pkg.ATTN_DECODE_MAX_GROUP == 16 and pkg.ATTN_DECODE_MAX_CONTEXT == 2 ** 31 - 1
    # the chunk is one of the three candidates and a multiple of every allowed page size
    assert pkg.ATTN_DECODE_CHUNK in (128, 256, 512) and all(pkg.ATTN_DECODE_CHUNK % p == 0 for p in pkg.ATTN_DECODE_PAGE_SIZES)
    assert callable(pkg.attn_decode) and callable(pkg.attn_decode_form) and callable(pkg.attn_decode_workspace_size)
    # the header states the definition to the letter and says what is not covered
    for text in ("L = clamp(seq_lens[s], 0, max_pages * page_size)", "s_t = scale * sum_d fp32(q_d) * fp32(k_t,d)", "m_c = max_t s_t",
                 "p_t = rne16(exp2f((s_t - m_c) * log2e))", "l_c = sum_t fp32(p_t)", "acc_c,d = sum_t fp32(p_t) * fp32(v_t,d)", "w_c = exp2f((m_c - m) * log2e)",
                 "ASCENDING c", "O_d = rne16(acc_d / l)", "lse = m + logf(l)", "O = +0 and lse = -inf", "masked by selection", "h / (q_heads / kv_heads)",
                 "more than one query token per sequence", "a sliding window", "soft-capping", "ALiBi", "an fp8 cache", "head dimensions", "RoPE",
                 "the cache append", "prefill"):
        assert text in header, text


@pytest.mark.parametrize("name", NAMES)
def test_statuses_before_any_device_work_in_the_stated_order(pkg, name):
    c = lambda **kw: call(pkg, name, **kw)
    C = pkg.ATTN_DECODE_CHUNK
    P2 = ctypes.c_void_p(0x90008)          # 8-byte aligned only
    split = dict(max_pages=C // 16 + 1)    # a shape of the SPLIT form
    inv = lambda kw: (c(**kw) == INVALID and WHO + b": invalid argument" in _err(pkg), kw)
    # 1. null operands
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(bt=None), dict(sl=None), dict(o=None)):
        assert all(inv(kw)) and b"null" in _err(pkg), kw
    # 2. a pitch below its extent
    for kw in (dict(ldq=8 * 128 - 8), dict(ldkv=2 * 128 - 8, page_stride=16 * 256), dict(page_stride=16 * 256 - 8), dict(ldbt=3), dict(ldo=1016)):
        assert all(inv(kw)) and b"pitch below its extent" in _err(pkg), kw
    # 3. kv_heads == 0 with q_heads > 0, 4. q_heads % kv_heads != 0
    assert all(inv(dict(kv_heads=0))) and b"kv_heads is 0" in _err(pkg)
    assert all(inv(dict(kv_heads=3))) and b"multiple of kv_heads" in _err(pkg)
    # 5. the SPLIT form with a null or short workspace (the DIRECT form takes none)
    need = pkg.attn_decode_workspace_size(2, 8, 128, 16, C // 16 + 1)
    for kw in (dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=need - 1), dict(ws=ctypes.c_void_p(0x80002))):
        assert all(inv(dict(split, **kw))) and b"SM_ATTN_DECODE_CHUNK" in _err(pkg) and b"workspace" in _err(pkg), kw
    assert c(seqs=0, ws_bytes=0, ws=None, **split) == INVALID and c(seqs=0, ws_bytes=0, **split) == 0 and c(seqs=0, ws_bytes=need, **split) == 0
    assert c(seqs=0, ws=None, ws_bytes=0) == 0 and c(seqs=0, ws=None, ws_bytes=0, max_pages=C // 16) == 0
    # 6. scale NaN (an infinite or a zero scale is the caller's business)
    assert all(inv(dict(scale=float("nan")))) and b"scale is NaN" in _err(pkg)
    assert c(seqs=0, scale=float("inf")) == 0 and c(seqs=0, scale=0.0) == 0 and c(seqs=0, scale=-1.0) == 0
    # ... in this order: each is answered before the next, and all before every not-supported shape
    assert c(q=None, ldq=8) == INVALID and b"null" in _err(pkg)
    assert c(ldq=8, kv_heads=0) == INVALID and b"pitch" in _err(pkg)
    assert c(kv_heads=0, ldkv=0, page_stride=0, scale=float("nan")) == INVALID and b"kv_heads is 0" in _err(pkg)
    assert c(kv_heads=3, ws=None, ldkv=384, **split) == INVALID and b"multiple" in _err(pkg)
    assert c(ws=None, scale=float("nan"), **split) == INVALID and b"workspace" in _err(pkg)
    assert c(scale=float("nan"), head_dim=96) == INVALID and c(o=None, seqs=BIG) == INVALID and c(scale=float("nan"), q=P2) == INVALID
    # 7. a dimension, a pitch or a product past 2^31 - 1
    for kw in (dict(seqs=BIG), dict(seqs=1 << 40), dict(num_pages=BIG), dict(ldq=BIG), dict(ldkv=BIG, page_stride=BIG * 16), dict(page_stride=BIG), dict(ldbt=BIG),
               dict(ldo=BIG), dict(max_pages=BIG, ldbt=BIG), dict(q_heads=1 << 24, kv_heads=1 << 24, ldq=BIG, ldo=BIG, ldkv=BIG, page_stride=BIG * 16),
               dict(seqs=1 << 28, q_heads=8)):
        assert c(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"2^31-1" in _err(pkg), kw
    assert c(seqs=BIG, head_dim=96, ldq=768, ldo=768, ldkv=192) == NOT_SUPPORTED and b"2^31-1" in _err(pkg)
    # 8. the limits, in the listed order: head_dim, page_size, the group, the context, the alignment
    for hd in (0, 8, 32, 96, 120, 192, 256):
        kw = dict(head_dim=hd, page_size=8, q_heads=34, q=P2)
        assert c(**kw) == NOT_SUPPORTED and WHO in _err(pkg) and b"SM_ATTN_DECODE_MIN_HEAD_DIM (64)" in _err(pkg) and b"SM_ATTN_DECODE_MAX_HEAD_DIM (128)" in _err(pkg), hd
    for ps in (0, 1, 8, 24, 48, 96, 256, 1024):
        kw = dict(page_size=ps, q_heads=34, q=P2, max_pages=2)
        assert c(**kw) == NOT_SUPPORTED and WHO in _err(pkg) and b"SM_ATTN_DECODE_MIN_PAGE_SIZE (16)" in _err(pkg) and b"SM_ATTN_DECODE_MAX_PAGE_SIZE (128)" in _err(pkg), ps
    for qh, kvh in ((17, 1), (34, 2), (64, 2), (96, 3)):
        assert c(q_heads=qh, kv_heads=kvh, q=P2) == NOT_SUPPORTED and WHO in _err(pkg) and b"SM_ATTN_DECODE_MAX_GROUP (16)" in _err(pkg), (qh, kvh)
    for ps, mp in ((16, 1 << 27), (128, 1 << 24), (32, (1 << 26) + 5)):
        assert c(page_size=ps, max_pages=mp, q=P2) == NOT_SUPPORTED and WHO in _err(pkg) and b"SM_ATTN_DECODE_MAX_CONTEXT" in _err(pkg), (ps, mp)
    for kw in (dict(q=P2), dict(k=P2), dict(v=P2), dict(o=P2), dict(ldq=1028), dict(ldkv=260, page_stride=16 * 260), dict(page_stride=16 * 256 + 4), dict(ldo=1036)):
        assert c(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"16-byte aligned" in _err(pkg), kw
    # ... every allowed value passes them (seqs = 0: nothing is enqueued), lse may be NULL, ldbt and the int32 operands carry no alignment rule
    for hd in pkg.ATTN_DECODE_HEAD_DIMS:
        for ps in pkg.ATTN_DECODE_PAGE_SIZES:
            for qh, kvh in ((1, 1), (2, 1), (4, 1), (5, 1), (8, 1), (16, 1), (32, 2), (48, 3), (3, 3)):
                assert c(seqs=0, head_dim=hd, page_size=ps, q_heads=qh, kv_heads=kvh) == 0, (hd, ps, qh, kvh)
    assert c(seqs=0, lse=None, ldbt=7, bt=ctypes.c_void_p(0x50004), sl=ctypes.c_void_p(0x60004)) == 0
    # 9. a zero extent: success, nothing enqueued (the fake pointers never reach a launch) -- but only behind the checks above
    for kw in (dict(seqs=0), dict(q_heads=0), dict(q_heads=0, kv_heads=0), dict(seqs=0, q_heads=0), dict(seqs=0, max_pages=0), dict(seqs=0, num_pages=0)):
        assert c(**kw) == 0, kw
    assert c(seqs=0, q=None) == INVALID and c(seqs=0, kv_heads=0) == INVALID and c(q_heads=0, scale=float("nan")) == INVALID
    assert c(seqs=0, head_dim=96, ldq=768, ldo=768, ldkv=192) == NOT_SUPPORTED and c(seqs=0, q=P2) == NOT_SUPPORTED and c(q_heads=0, page_size=8) == NOT_SUPPORTED


def test_form_and_workspace_size_at_every_boundary(pkg):
    C = pkg.ATTN_DECODE_CHUNK
    lib = pkg.lib()
    assert lib.sm_attn_decode_form(1, 1, 1, 128, 16, 1, None) == INVALID and b"sm_attn_decode_form" in _err(pkg)
    assert lib.sm_attn_decode_workspace_size(1, 1, 128, 16, 1, None) == INVALID and b"sm_attn_decode_workspace_size" in _err(pkg)

    def form(seqs=3, q_heads=8, kv_heads=2, head_dim=128, page_size=16, max_pages=4):
        f = ctypes.c_int(-1)
        assert lib.sm_attn_decode_form(seqs, q_heads, kv_heads, head_dim, page_size, max_pages, ctypes.byref(f)) == 0
        assert pkg.attn_decode_form(seqs, q_heads, kv_heads, head_dim, page_size, max_pages) == pkg.ATTN_DECODE_FORMS[f.value]
        return pkg.ATTN_DECODE_FORMS[f.value]

    def size(seqs, q_heads, head_dim, page_size, max_pages):
        ctx = page_size * max_pages
        want = 0 if ctx <= C else seqs * q_heads * -(-ctx // C) * (head_dim + 2) * 4        # the formula of the header, restated
        got = pkg.attn_decode_workspace_size(seqs, q_heads, head_dim, page_size, max_pages)
        assert got == want, (seqs, q_heads, head_dim, page_size, max_pages, got, want)
        return got

    seen = set()
    for ps in pkg.ATTN_DECODE_PAGE_SIZES:
        for hd in pkg.ATTN_DECODE_HEAD_DIMS:
            n = C // ps
            for mp, want in ((0, "direct"), (1, "direct"), (n - 1, "direct"), (n, "direct"), (n + 1, "split"), (2 * n, "split"), (2 * n + 1, "split"), (5 * n, "split")):
                assert form(head_dim=hd, page_size=ps, max_pages=mp) == want, (ps, hd, mp)
                assert (size(3, 8, hd, ps, mp) > 0) == (want == "split")
                seen.add(want)
            assert size(3, 8, hd, ps, n + 1) == 3 * 8 * 2 * (hd + 2) * 4 and size(1, 1, hd, ps, 5 * n) == 5 * (hd + 2) * 4
            assert size(0, 8, hd, ps, 5 * n) == 0 and size(7, 0, hd, ps, 5 * n) == 0
    for group in range(1, 20):
        for kvh in (1, 2, 3):
            assert form(q_heads=group * kvh, kv_heads=kvh) == ("direct" if group <= 16 else "invalid"), (group, kvh)
    for hd in (0, 8, 32, 63, 65, 96, 127, 129, 192, 256):
        assert form(head_dim=hd) == "invalid", hd
    for ps in (0, 1, 8, 15, 17, 24, 48, 96, 127, 129, 256):
        assert form(page_size=ps) == "invalid", ps
    assert form(q_heads=8, kv_heads=0) == "invalid" and form(q_heads=8, kv_heads=3) == "invalid" and form(q_heads=2, kv_heads=4) == "invalid"
    assert form(page_size=16, max_pages=1 << 27) == "invalid" and form(page_size=16, max_pages=(1 << 27) - 1) == "split"
    assert form(seqs=0) == "empty" and form(q_heads=0) == "empty" and form(q_heads=0, kv_heads=0) == "empty" and form(seqs=0, max_pages=1000) == "empty"
    assert form(seqs=0, head_dim=96) == "invalid"
    seen |= {"empty", "invalid"}
    assert seen == set(pkg.ATTN_DECODE_FORMS)
    assert lib.sm_attn_decode_workspace_size(1 << 40, 1 << 20, 128, 16, 1 << 26, ctypes.byref(ctypes.c_size_t(0))) == NOT_SUPPORTED and b"overflows" in _err(pkg)


# ------------------------------------------------------------------------------------------------ the numpy restatement
@pytest.mark.parametrize("case", al.CASES, ids=al.case_id)
def test_restatement_in_fp32_against_the_fp64_definition_on_every_general_case(pkg, case):
    """what the GPU test asks of the device, asked of the fp32 restatement: every sigma, and the peaked softmax (8 times the scale)"""
    i = al.CASES.index(case)
    rng = np.random.default_rng(al.seed(al.SALT, "general", i))
    pr = al.Problem(case, pkg.ATTN_DECODE_CHUNK, rng)
    for sigma, mult in [(s, 1.0) for s in SIGMAS] + [(1.0, 8.0)]:
        Q, K, V = al.general(pr, rng, sigma)
        scale = mult * pr.hd ** -0.5
        ob, lse = al.restate32(pr, Q, K, V, scale)
        ro, rl = al.worst_ratios(pr, ob, lse, Q, K, V, scale)
        print(f"restatement {al.case_id(case)} sigma {sigma} scale x{mult:g}: O {ro:.3f}, lse {rl:.3f} of the bound")
        assert ro <= 1.0 and rl <= 1.0, (sigma, mult, ro, rl)


@pytest.mark.parametrize("case", al.CASES, ids=al.case_id)
def test_both_exact_classes_bit_for_bit_through_the_restatement(pkg, case):
    i = al.CASES.index(case)
    rng = np.random.default_rng(al.seed(al.SALT, "exact", i))
    pr = al.Problem(case, pkg.ATTN_DECODE_CHUNK, rng)
    assert al.form_of(pr) == pkg.attn_decode_form(pr.seqs, pr.q_heads, pr.kvh, pr.hd, pr.ps, pr.max_pages)
    Q, K, V, targets, want, wl = al.one_hot(pr, rng)
    ob, lse = al.restate32(pr, Q, K, V, 1.0)
    assert np.array_equal(ob, want) and np.array_equal(lse, wl), "one-hot: the restatement is not V's target row"
    assert not np.any(want[[s for s in range(pr.seqs) if pr.tokens(s)[0].size]] == 0x8000)
    Q, K, V, want, wl = al.uniform(pr, rng)
    ob, lse = al.restate32(pr, Q, K, V, pr.hd ** -0.5)
    assert np.array_equal(ob, want), "uniform: the restatement is not rne16(sum v / T)"
    fin = np.isfinite(wl)
    assert np.array_equal(np.isneginf(lse), ~fin) and np.all(np.abs(lse[fin] - wl[fin]) <= 2 * np.spacing(np.abs(wl[fin]).astype(np.float32)))
