"""sm_rope_append_{f16,bf16} and sm_rope_append_form without a GPU: the three symbols are declared, exported and bound with the header's
arity and prototype, every #define matches the package's constant and the header states the definition's formulas and what is not
covered; every status is returned before any device work (fake pointers, never dereferenced) in the order the header states, with a
text that names the entry point and the limit -- and what is not read is not checked: ldko without Ko, the cache's pitches and sizes
without a cache, cs with rot_dim == 0; the zero-extent successes sit behind those checks; the form at 0, 1, BLOCK_MAX_TOKENS and
BLOCK_MAX_TOKENS + 1 tokens and at every refused head_dim / rot_dim; and the numpy restatement the GPU test compares the device with
(tests/rope_append_testlib.py): in float32 against the float64 definition on EVERY general-data case of the GPU table within, per element,
    1/2 ulp16 at max(|ref|, |y|) + 3 2^-24 (|x_a c| + |x_b s|)
-- one rounding to 16 bits; two rounded fp32 products and one rounded fp32 sum: an allowance from the definition, not a measurement --,
against the usual torch CPU spelling x cos + rotate_half(x) sin in fp32 within the same bound, the contraction witnesses' premise, and
rope_table against numpy's float64 cos / sin rounded once."""
import ctypes
import os
import re

import numpy as np
import pytest

import rope_append_testlib as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NOT_SUPPORTED = 1, 2
BIG = 1 << 31
WHO = b"sm_rope_append_{f16,bf16}"
NAMES = ["sm_rope_append_f16", "sm_rope_append_bf16"]
# stand-ins for device pointers, all 16-byte aligned and distinct
Q, K, V, QO, KO, KC, VC, CS, POS, TS, SL, BT = (ctypes.c_void_p(0x10000 * (i + 1)) for i in range(12))
GENERAL = [c for c in rl.CASES if c["data"] in ("general", "witness")]


def _err(pkg):
    return pkg.lib().sm_last_error()


def call(pkg, name="sm_rope_append_bf16", q=Q, k=K, v=V, qo=QO, ko=KO, kc=KC, vc=VC, cs=CS, pos=POS, ts=TS, sl=SL, bt=BT, tokens=4, seqs=2, q_heads=8, kv_heads=2,
         head_dim=128, rot_dim=128, max_pos=64, num_pages=64, page_size=16, max_pages=4, ldq=None, ldk=None, ldv=None, ldqo=None, ldko=None, ldkv=None,
         page_stride=None, ldcs=None, ldbt=None, style=0):
    qw, kw = q_heads * head_dim, kv_heads * head_dim
    d = lambda x, y: y if x is None else x
    ldkv = d(ldkv, kw)
    return getattr(pkg.lib(), name)(q, k, v, qo, ko, kc, vc, cs, pos, ts, sl, bt, tokens, seqs, q_heads, kv_heads, head_dim, rot_dim, max_pos, num_pages, page_size,
                                    max_pages, d(ldq, qw), d(ldk, kw), d(ldv, kw), d(ldqo, qw), d(ldko, kw), ldkv, d(page_stride, page_size * ldkv), d(ldcs, rot_dim),
                                    d(ldbt, max_pages), style, None)


def test_symbols_exported_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    pkg.build()
    L = ctypes.CDLL(pkg.LIB_PATH)
    for name in NAMES + ["sm_rope_append_form"]:
        assert name + "(" in header and name in pkg.EXPORTED_SYMBOLS and hasattr(L, name), name
    sz, ci, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    for name in NAMES:
        assert pkg._SIGS[name] == [vp] * 12 + [sz] * 19 + [ci, vp], name
        proto = re.search(name + r"\(([^;]*?)\);", header, flags=re.S).group(1)
        assert len(proto.split(",")) == 33 == len(pkg._SIGS[name])
        assert re.search(r"const void\* Q,\s*const void\* K,\s*const void\* V,\s*void\* Qo,\s*void\* Ko,\s*void\* Kc,\s*void\* Vc,\s*const float\* cs,\s*"
                         r"const int\* positions,\s*const int\* token_seq,\s*const int\* seq_lens,\s*const int\* block_table,\s*size_t tokens,\s*size_t seqs,\s*"
                         r"size_t q_heads,\s*size_t kv_heads,\s*size_t head_dim,\s*size_t rot_dim,\s*size_t max_pos,\s*size_t num_pages,\s*size_t page_size,\s*"
                         r"size_t max_pages,\s*size_t ldq,\s*size_t ldk,\s*size_t ldv,\s*size_t ldqo,\s*size_t ldko,\s*size_t ldkv,\s*size_t page_stride,\s*"
                         r"size_t ldcs,\s*size_t ldbt,\s*int style,\s*sm_stream_t stream", proto), name
    assert re.search(r"int sm_rope_append_form\(size_t tokens,\s*size_t q_heads,\s*size_t kv_heads,\s*size_t head_dim,\s*size_t rot_dim,\s*int\* form\);", header)
    assert len(pkg._SIGS["sm_rope_append_form"]) == 6
    # the declaration sits directly after the attention block
    assert header.index("int sm_attn_decode_form(") < header.index("RoPE + paged KV-cache append") < header.index("int sm_rope_append_f16(") < header.index("fp32 form: the STRIP rule")
    # every #define against the package's constant
    defines = dict(re.findall(r"#define (SM_ROPE_\w+) (\d+)\b", header))
    want = {"SM_ROPE_NEOX": pkg.ROPE_NEOX, "SM_ROPE_INTERLEAVED": pkg.ROPE_INTERLEAVED, "SM_ROPE_APPEND_MAX_HEAD_DIM": pkg.ROPE_APPEND_MAX_HEAD_DIM,
            "SM_ROPE_APPEND_ROT_DIM_MULTIPLE": pkg.ROPE_APPEND_ROT_DIM_MULTIPLE, "SM_ROPE_APPEND_BLOCK_MAX_TOKENS": pkg.ROPE_APPEND_BLOCK_MAX_TOKENS,
            "SM_ROPE_APPEND_FORM_INVALID": 0, "SM_ROPE_APPEND_FORM_EMPTY": 1, "SM_ROPE_APPEND_FORM_BLOCK": 2, "SM_ROPE_APPEND_FORM_WAVE": 3}
    assert {k: int(v) for k, v in defines.items()} == want
    assert pkg.ROPE_APPEND_FORMS == ("invalid", "empty", "block", "wave") and (pkg.ROPE_NEOX, pkg.ROPE_INTERLEAVED) == (0, 1)
    assert pkg.ROPE_APPEND_MAX_HEAD_DIM == 256 and pkg.ROPE_APPEND_ROT_DIM_MULTIPLE == 16 and pkg.ROPE_APPEND_BLOCK_MAX_TOKENS >= 1
    assert callable(pkg.rope_append) and callable(pkg.rope_append_form) and callable(pkg.rope_table)
    # the header states the definition to the letter and says what is not covered
    for text in ("s_i = token_seq ? token_seq[i] : i", "pos_i = positions ? positions[i] : seq_lens[s_i] - 1", "pos_i = -1", "PADDING token",
                 "half = rot_dim / 2", "c_j = cs[pos_i][j]", "s_j = cs[pos_i][half + j]", "(a, b) = (j, j + half)", "(a, b) = (2j, 2j + 1)",
                 "y_a = rne16(fp32(x_a) * c_j - fp32(x_b) * s_j)", "y_b = rne16(fp32(x_b) * c_j + fp32(x_a) * s_j)", "NOT", "contracted", "never an fma",
                 "copied bit for bit", "subnormals are not flushed", "pg = block_table[s_i][pos_i / page_size]", "Kc[pg][pos_i % page_size]", "64-bit arithmetic",
                 "Qo == Q and Ko == K", "an fp8 cache", "multi-axis (M-RoPE) positions", "per-head QK-norm", "a 16-bit table", "computing the table on the device",
                 "incrementing seq_lens", "a cache layout other than"):
        assert text in header, text
    # the attention entry point's comment is as it was
    assert "other than the two, RoPE, the cache append, prefill. */" in header


@pytest.mark.parametrize("name", NAMES)
def test_statuses_before_any_device_work_in_the_stated_order(pkg, name):
    c = lambda **kw: call(pkg, name, **kw)
    P2 = ctypes.c_void_p(0x90008)          # 8-byte aligned only
    P4 = ctypes.c_void_p(0x90004)

    def inv(word, **kw):
        assert c(**kw) == INVALID, kw
        assert WHO + b": invalid argument" in _err(pkg) and word in _err(pkg), (kw, _err(pkg))
    # 1. the null operands and the operand rules, in the header's order
    for kw in (dict(q=None), dict(k=None), dict(v=None), dict(qo=None)):
        inv(b"null Q, K, V or Qo", **kw)
    inv(b"exactly one of Kc / Vc", kc=None)
    inv(b"exactly one of Kc / Vc", vc=None)
    inv(b"Kc and Ko are both null", kc=None, vc=None, ko=None)
    inv(b"null block_table with a cache", bt=None)
    inv(b"positions and seq_lens are both null", pos=None, sl=None)
    inv(b"null cs with rot_dim > 0", cs=None)
    for st in (-1, 2, 7):
        inv(b"SM_ROPE_NEOX or SM_ROPE_INTERLEAVED", style=st)
    for kw in (dict(ldq=1016), dict(ldk=248), dict(ldv=248), dict(ldqo=1016), dict(ldko=248), dict(ldkv=248, page_stride=16 * 256), dict(page_stride=16 * 256 - 8),
               dict(ldcs=120), dict(ldbt=3)):
        inv(b"pitch below its extent", **kw)
    inv(b"rot_dim exceeds head_dim", rot_dim=144, ldcs=144)
    inv(b"null token_seq with tokens > seqs", ts=None, tokens=3, seqs=2)
    for kw in (dict(qo=K), dict(ko=Q), dict(ko=V), dict(kc=VC), dict(qo=KC), dict(k=Q), dict(v=K, ldq=2048, ldqo=2048), dict(qo=Q, ldqo=1032), dict(ko=K, ldko=264),
               dict(kc=K, ldk=512), dict(vc=V)):
        inv(b"aliased operands", **kw)
    # ... each is answered before the next, and all before every not-supported shape
    inv(b"null Q", q=None, kc=None)
    inv(b"exactly one", kc=None, ko=None, bt=None)
    inv(b"both null: the rotated K", kc=None, vc=None, ko=None, pos=None, sl=None)
    inv(b"block_table", bt=None, pos=None, sl=None)
    inv(b"positions and seq_lens", pos=None, sl=None, cs=None)
    inv(b"null cs", cs=None, style=5)
    inv(b"style", style=5, ldq=8)
    inv(b"pitch", ldq=8, rot_dim=256, ldcs=256)
    inv(b"rot_dim exceeds", rot_dim=256, ldcs=256, ts=None, tokens=9)
    inv(b"token_seq", ts=None, tokens=9, qo=K)
    inv(b"aliased", qo=K, tokens=BIG)
    inv(b"aliased", qo=K, head_dim=4, rot_dim=0)
    inv(b"null Q", q=None, head_dim=260, rot_dim=8, page_size=3)
    # ... the allowed aliases and the decode spellings pass (tokens = 0 would hide them: a non-empty call with fake pointers cannot be made, so
    # they are shown by the NOT_SUPPORTED answer that lies behind every INVALID one)
    for kw in (dict(qo=Q), dict(ko=K), dict(qo=Q, ko=K), dict(ko=None), dict(kc=None, vc=None), dict(kc=None, vc=None, bt=None), dict(pos=None), dict(sl=None),
               dict(ts=None, tokens=2), dict(ts=None, pos=None, tokens=2), dict(cs=None, rot_dim=0)):
        assert c(head_dim=260, ldq=4096, ldqo=4096, ldk=1024, ldv=1024, ldko=1024, ldkv=1024, **kw) == NOT_SUPPORTED, kw
        assert b"SM_ROPE_APPEND_MAX_HEAD_DIM (256)" in _err(pkg), kw
    # 2. a dimension, a pitch or a product past 2^31 - 1
    for kw in (dict(tokens=BIG), dict(tokens=1 << 40), dict(seqs=BIG), dict(num_pages=BIG), dict(max_pos=BIG), dict(ldq=BIG), dict(ldk=BIG), dict(ldv=BIG), dict(ldqo=BIG),
               dict(ldko=BIG), dict(ldkv=BIG, page_stride=BIG * 16), dict(page_stride=BIG), dict(ldcs=BIG), dict(ldbt=BIG), dict(max_pages=BIG, ldbt=BIG),
               dict(max_pages=1 << 27, ldbt=1 << 27), dict(q_heads=1 << 24, ldq=BIG, ldqo=BIG), dict(kv_heads=1 << 24, ldk=BIG, ldv=BIG, ldko=BIG, ldkv=BIG, page_stride=BIG * 16)):
        assert c(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"2^31-1" in _err(pkg), kw
    assert c(tokens=BIG, head_dim=12, rot_dim=0) == NOT_SUPPORTED and b"2^31-1" in _err(pkg)
    # 3. the limits, in the listed order: head_dim, rot_dim, page_size, the 16-bit rows, the table's rows
    for hd in (4, 12, 36, 100, 257, 260, 264, 512):
        assert c(head_dim=hd, rot_dim=min(8, hd), ldcs=8, page_size=8, q=P2, ldq=8 * hd, ldqo=8 * hd, ldk=2 * hd, ldv=2 * hd, ldko=2 * hd, ldkv=2 * hd) == NOT_SUPPORTED, hd
        assert WHO in _err(pkg) and b"multiple of 8" in _err(pkg) and b"SM_ROPE_APPEND_MAX_HEAD_DIM (256)" in _err(pkg), hd
    for rot in (2, 8, 24, 40, 100, 120):
        assert c(rot_dim=rot, ldcs=rot, page_size=8, q=P2) == NOT_SUPPORTED and WHO in _err(pkg) and b"SM_ROPE_APPEND_ROT_DIM_MULTIPLE (16)" in _err(pkg), rot
    for ps in (0, 1, 8, 24, 48, 96, 256, 1024):
        assert c(page_size=ps, q=P2, max_pages=2) == NOT_SUPPORTED, ps
        assert WHO in _err(pkg) and b"SM_ATTN_DECODE_MIN_PAGE_SIZE (16)" in _err(pkg) and b"SM_ATTN_DECODE_MAX_PAGE_SIZE (128)" in _err(pkg), ps
    for kw in (dict(q=P2), dict(k=P2), dict(v=P2), dict(qo=P2), dict(ko=P2), dict(kc=P2), dict(vc=P2), dict(ldq=1028), dict(ldk=260), dict(ldv=260), dict(ldqo=1036),
               dict(ldko=260), dict(ldkv=260, page_stride=16 * 260 + 4), dict(page_stride=16 * 256 + 4)):
        assert c(cs=P4, **kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"16-byte aligned rows of Q, K, V, Qo, Ko, Kc and Vc" in _err(pkg), kw
    for kw in (dict(cs=P2), dict(cs=P4), dict(ldcs=130)):
        assert c(**kw) == NOT_SUPPORTED, kw
        assert WHO in _err(pkg) and b"16-byte aligned rows of cs" in _err(pkg), kw
    # ... what is not read is not checked: ldko without Ko; the cache's pitches, sizes and page_size without a cache; cs, ldcs and max_pos with rot_dim == 0
    e = dict(tokens=0)
    assert c(ko=None, ldko=0, **e) == 0 and c(ko=None, ldko=BIG + 3, **e) == 0
    assert c(kc=None, vc=None, bt=None, ldkv=3, page_stride=1, ldbt=0, num_pages=BIG, page_size=7, max_pages=1 << 40, **e) == 0
    assert c(rot_dim=0, cs=None, ldcs=0, max_pos=1 << 40, **e) == 0 and c(rot_dim=0, cs=P4, ldcs=1, **e) == 0
    # ... every allowed value passes them (tokens = 0: nothing is enqueued); the int32 operands carry no alignment rule
    for hd in (8, 40, 64, 96, 128, 256):
        for rot in (r for r in (0, 16, 32, 48, 64, 96, 128, 256) if r <= hd):
            for ps in pkg.ATTN_DECODE_PAGE_SIZES:
                for st in (pkg.ROPE_NEOX, pkg.ROPE_INTERLEAVED):
                    assert c(head_dim=hd, rot_dim=rot, page_size=ps, style=st, **e) == 0, (hd, rot, ps, st)
    assert c(pos=P4, ts=ctypes.c_void_p(0x50004), sl=ctypes.c_void_p(0x60004), bt=ctypes.c_void_p(0x70004), ldbt=7, **e) == 0
    # 4. a zero extent: success, nothing enqueued (the fake pointers never reach a launch) -- but only behind the checks above
    for kw in (dict(tokens=0), dict(q_heads=0, kv_heads=0), dict(tokens=0, seqs=0), dict(tokens=0, max_pages=0), dict(tokens=0, num_pages=0), dict(tokens=0, max_pos=0),
               dict(head_dim=0, rot_dim=0, cs=None)):
        assert c(**kw) == 0, kw
    assert c(tokens=0, q=None) == INVALID and c(tokens=0, style=3) == INVALID and c(q_heads=0, kv_heads=0, cs=None) == INVALID
    assert c(tokens=0, head_dim=260, ldq=4096, ldqo=4096, ldk=1024, ldv=1024, ldko=1024, ldkv=1024) == NOT_SUPPORTED and c(tokens=0, q=P2) == NOT_SUPPORTED
    assert c(q_heads=0, kv_heads=0, page_size=8) == NOT_SUPPORTED and c(tokens=0, rot_dim=8, ldcs=8) == NOT_SUPPORTED


def test_form_at_every_boundary(pkg):
    B = pkg.ROPE_APPEND_BLOCK_MAX_TOKENS
    lib = pkg.lib()
    assert lib.sm_rope_append_form(1, 1, 1, 128, 128, None) == INVALID and b"sm_rope_append_form" in _err(pkg)

    def form(tokens=3, q_heads=8, kv_heads=2, head_dim=128, rot_dim=64):
        f = ctypes.c_int(-1)
        assert lib.sm_rope_append_form(tokens, q_heads, kv_heads, head_dim, rot_dim, ctypes.byref(f)) == 0
        assert pkg.rope_append_form(tokens, q_heads, kv_heads, head_dim, rot_dim) == pkg.ROPE_APPEND_FORMS[f.value]
        return pkg.ROPE_APPEND_FORMS[f.value]

    seen = set()
    for tokens, want in ((0, "empty"), (1, "block"), (B, "block"), (B + 1, "wave"), (B + 5, "wave"), (1 << 20, "wave")):
        for hd, rot in ((128, 128), (64, 0), (40, 32), (256, 16)):
            assert form(tokens=tokens, head_dim=hd, rot_dim=rot) == want, (tokens, hd, rot)
        seen.add(want)
    assert form(q_heads=0, kv_heads=0) == "empty" and form(q_heads=0) == "block" and form(kv_heads=0) == "block" and form(tokens=0, q_heads=0) == "empty"
    for hd in (4, 12, 36, 100, 257, 260, 264, 512):
        assert form(head_dim=hd, rot_dim=0) == "invalid" and form(tokens=0, head_dim=hd, rot_dim=0) == "invalid", hd
    for rot in (2, 8, 24, 40, 100, 120, 144, 256):
        assert form(rot_dim=rot) == "invalid" and form(tokens=0, rot_dim=rot) == "invalid", rot
    assert form(tokens=BIG) == "invalid" and form(q_heads=1 << 24) == "invalid" and form(kv_heads=1 << 24) == "invalid"
    assert form(head_dim=0, rot_dim=0) == "empty"
    seen.add("invalid")
    assert seen == set(pkg.ROPE_APPEND_FORMS)


# ------------------------------------------------------------------------------------------------ the numpy restatement
def _worst(pr, ev32, ev64):
    worst = 0.0
    for n in ("q", "k"):
        live = np.flatnonzero(pr.live)
        if live.size == 0:
            continue
        got = rl.f32_of(ev32[n + "bits"], pr.ty).astype(np.float64)[live]
        ref = ev64[n][live]
        assert np.isfinite(got).all() and np.isfinite(ref).all()
        b = rl.bound(pr, ref, got, ev64[n + "mag"][live])
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(b > 0, np.abs(got - ref) / np.where(b > 0, b, 1), np.where(got == ref, 0.0, np.inf))
        worst = max(worst, float(r.max()))
    return worst


@pytest.mark.parametrize("case", GENERAL, ids=rl.case_id)
def test_restatement_in_fp32_against_the_fp64_definition_on_every_general_case(pkg, case):
    pr, (Qb, Kb, Vb, cs) = rl.make(case)
    ev32, ev64 = rl.evaluate(pr, Qb, Kb, Vb, cs, np.float32), rl.evaluate(pr, Qb, Kb, Vb, cs, np.float64)
    w = _worst(pr, ev32, ev64)
    print(f"restatement {rl.case_id(case)}: worst share of the bound {w:.3f}")
    assert w <= 1.0, w
    # elements at or beyond rot_dim are the input's bits; padding tokens are never rotated
    a, b = pr.pairs()
    keep = np.setdiff1d(np.arange(pr.hd), np.concatenate([a, b]))
    assert np.array_equal(ev32["qbits"][:, :, keep], Qb[:, :, keep]) and np.array_equal(ev32["kbits"][:, :, keep], Kb[:, :, keep])


@pytest.mark.parametrize("case", [c for c in GENERAL if c["rot"] > 0][::3], ids=rl.case_id)
def test_restatement_against_the_torch_cpu_spelling(pkg, case):
    """x cos + rotate_half(x) sin in fp32 on the CPU, the spelling a caller has today, within the bound of the definition"""
    import torch
    pr, (Qb, Kb, Vb, cs) = rl.make(case)
    ev32, ev64 = rl.evaluate(pr, Qb, Kb, Vb, cs, np.float32), rl.evaluate(pr, Qb, Kb, Vb, cs, np.float64)
    live = np.flatnonzero(pr.live)
    half, rot = pr.half, pr.rot
    for n, X in (("q", Qb), ("k", Kb)):
        x = torch.from_numpy(rl.f32_of(X, pr.ty)[live])                                  # [live][heads][hd] fp32
        row = torch.from_numpy(np.ascontiguousarray(cs[pr.pos[live]]))[:, None, :]     # [live][1][rot]
        xr = x[..., :rot]
        if pr.style == rl.NEOX:
            cos, sin = torch.cat([row[..., :half]] * 2, -1), torch.cat([row[..., half:rot]] * 2, -1)
            rh = torch.cat([-xr[..., half:], xr[..., :half]], -1)
        else:
            cos, sin = row[..., :half].repeat_interleave(2, -1), row[..., half:rot].repeat_interleave(2, -1)
            rh = torch.stack([-xr[..., 1::2], xr[..., 0::2]], -1).flatten(-2)
        y = torch.cat([xr * cos + rh * sin, x[..., rot:]], -1).numpy().astype(np.float64)
        got16 = rl.f32_of(rl.rne16(y.astype(np.float32), pr.ty), pr.ty).astype(np.float64)
        b = rl.bound(pr, ev64[n][live], got16, ev64[n + "mag"][live])
        assert np.all(np.abs(got16 - ev64[n][live]) <= b), "the torch spelling is outside the definition's bound"
        mine = rl.f32_of(ev32[n + "bits"], pr.ty).astype(np.float64)[live]
        assert np.all(np.abs(mine - got16) <= 2 * b), "the restatement and the torch spelling are further apart than both bounds allow"


@pytest.mark.parametrize("ty", rl.TYPES)
def test_contraction_witnesses_exist_and_separate(pkg, ty):
    rng = np.random.default_rng(rl.seed(rl.SALT, "witness", ty))
    found = rl.find_witnesses(ty, rng)
    assert set(found) == {"ya1", "ya2", "yb1", "yb2"} and all(len(v) >= 1 for v in found.values())
    case = next(c for c in rl.CASES if c["data"] == "witness" and c["ty"] == ty)
    rl.make(case)          # plants them and asserts the premise


def test_special_values_go_through_ieee_arithmetic(pkg):
    """the restatement on the special pool: NaN where IEEE has NaN, fp32 subnormal products kept (not flushed) on bf16 inputs"""
    for case in (c for c in rl.CASES if c["data"] == "special"):
        pr, (Qb, Kb, Vb, cs) = rl.make(case)
        ev = rl.evaluate(pr, Qb, Kb, Vb, cs, np.float32)
        live = np.flatnonzero(pr.live)
        assert rl.is_nan16(ev["qbits"][live], pr.ty).any() and (ev["qbits"][live] == 0x8000).any()
        if pr.ty == "bf16":
            assert (ev["qbits"][live] == 0x0001).any() or (ev["qbits"][live] == 0x8001).any(), "a subnormal of the type survives a multiply by +-1"


def test_rope_table_against_numpy_float64_rounded_once(pkg):
    for max_pos, rot, base in ((1, 16, 10000.0), (300, 128, 10000.0), (64, 32, 500000.0), (17, 0, 10000.0), (0, 64, 10000.0)):
        t = pkg.rope_table(max_pos, rot, base)
        assert tuple(t.shape) == (max_pos, rot) and str(t.dtype) == "torch.float32"
        half = rot // 2
        theta = np.float64(base) ** (-2.0 * np.arange(half, dtype=np.float64) / max(rot, 1))
        ang = np.arange(max_pos, dtype=np.float64)[:, None] * theta[None, :]
        want = np.concatenate([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32)
        assert np.array_equal(t.numpy().view(np.uint32), want.view(np.uint32)), (max_pos, rot, base)
        assert np.array_equal(want, rl.table64(max_pos, rot, base).astype(np.float32))
    assert np.array_equal(pkg.rope_table(4, 8).numpy()[0], np.array([1, 1, 1, 1, 0, 0, 0, 0], dtype=np.float32))
    with pytest.raises(pkg.SparsifymeError):
        pkg.rope_table(4, 7)
