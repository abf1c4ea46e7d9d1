"""The dispatch of prune / check / compress / decompress / one-pass prune + compress as host-side queries (sm_prune24_form,
sm_prune24_check_form, sm_compress24_form, sm_decompress24_form, sm_prune24_compress24_form), without a GPU: the class of every case
of tests/test_gpu_prune_classes.py from dummy addresses (one-pass rows at 256 CUs), both sides of every threshold, every refusal's status
and message, the numpy restatement of STRIP against the oracle on the specials pool, and the GPU file's own instruments."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_gpu_prune_classes as pc   # (as a module: its test functions must not be collected here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIGIN_IN, ORIGIN_OUT, BLOB, FLAG = 0x10000000, 0x20000000, 0x30000000, 0x40000040   # 16-byte multiples: a base's alignment is its offset's
TILE, STRIP = pc.TILE, pc.STRIP


def addr(origin, off, ty):
    return origin + (pc.GUARD + off) * pc.ELT[ty]


# ---------------------------------------------------------------------------------------------
# the ABI
# ---------------------------------------------------------------------------------------------
def test_queries_are_declared_bound_and_named_as_the_header_names_them(pkg):
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = pkg.lib()
    for fn in ("sm_prune24_form", "sm_prune24_check_form", "sm_compress24_form", "sm_decompress24_form", "sm_prune24_compress24_form"):
        assert fn + "(" in header and fn in pkg.EXPORTED_SYMBOLS and hasattr(L, fn)
    for prefix, names in (("SM_PRUNE24_FORM_", pkg.PRUNE24_FORMS), ("SM_COMPRESS24_FORM_", pkg.COMPRESS24_FORMS),
                          ("SM_DECOMPRESS24_FORM_", pkg.DECOMPRESS24_FORMS), ("SM_PRUNE24_COMPRESS24_FORM_", pkg.PRUNE24_COMPRESS24_FORMS)):
        for value, name in enumerate(names):
            assert re.search(r"#define %s%s %d\b" % (prefix, name.upper(), value), header), prefix + name
        assert len(re.findall(r"#define %s[A-Z0-9_]+ \d+" % prefix, header)) == len(names)


def test_queries_validate_their_own_arguments(pkg):
    L = pkg.lib()
    out = ctypes.c_int(-1)
    assert L.sm_prune24_form(16, 32, 4, 4, 4, 2, STRIP, None, None) == 1 and b"sm_prune24_form" in L.sm_last_error()
    assert L.sm_prune24_form(16, 32, 4, 4, 4, 3, STRIP, ctypes.byref(out), None) == 1
    assert L.sm_prune24_check_form(16, 32, 4, 4, 4, 8, ctypes.byref(out)) == 1 and b"sm_prune24_check_form" in L.sm_last_error()
    assert L.sm_compress24_form(16, 32, 4, 4, 4, 1, 16, 1, ctypes.byref(out)) == 1 and b"sm_compress24_form" in L.sm_last_error()
    assert L.sm_decompress24_form(16, 32, 4, 4, 4, 1, 16, 2, None) == 1 and b"sm_decompress24_form" in L.sm_last_error()
    assert L.sm_prune24_compress24_form(16, 32, 4, 64, 64, 1, 256, 48, 0, TILE, 256, ctypes.byref(out), None) == 1
    assert b"sm_prune24_compress24_form" in L.sm_last_error() and out.value == -1
    # span_rows and plan may be null; invalid and empty calls are answered, not refused
    assert L.sm_prune24_form(16, 32, 4, 4, 4, 2, STRIP, ctypes.byref(out), None) == 0 and pkg.PRUNE24_FORMS[out.value] == "strip_scalar"
    assert L.sm_prune24_compress24_form(16, 32, 4, 64, 64, 1, 256, 48, 2, TILE, 256, ctypes.byref(out), None) == 0
    assert pkg.prune24_form(None, 32, 4, 4, 4, 2) == "invalid" and pkg.prune24_form(16, 32, 4, 4, 3, 2) == "invalid"
    assert pkg.prune24_form(16, 32, 4, 4, 4, 2, alg=2) == "invalid" and pkg.prune24_form(16, 32, 0, 4, 4, 2) == "empty"
    assert pkg.prune24_check_form(16, None, 4, 4, 4, 2) == "invalid" and pkg.prune24_check_form(16, 32, 4, 0, 4, 2) == "empty"
    assert pkg.compress24_form(16, 40, 4, 4, 4, 1, 16, 2) == "invalid" and pkg.compress24_form(16, 48, 4, 4, 4, 0, 16, 2) == "empty"
    assert pkg.decompress24_form(None, 16, 4, 4, 4, 1, 16, 2) == "invalid" and pkg.decompress24_form(48, 16, 4, 0, 4, 1, 16, 4) == "empty"
    assert pkg.prune24_compress24_form(16, None, 4, 64, 64, 1, 256, 40, 2, cus=256)[0] == "invalid"
    assert pkg.prune24_compress24_form(16, None, 4, 64, 64, 0, 256, None, 2, cus=256)[0] == "empty"


# ---------------------------------------------------------------------------------------------
# every GPU case reaches the class its row names
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct", pc.fams(pc.PRUNE_CASES), ids=pc.cid)
def test_prune_case_class(pkg, ct):
    c, ty = ct
    got = pc.query_prune(pkg, c, ty, addr(ORIGIN_IN, c.off_in, ty), addr(ORIGIN_OUT, c.off_out, ty))
    assert got == (c.cls, c.span_rows)
    if c.alg == STRIP:     # the check on the same layout
        assert pkg.prune24_check_form(addr(ORIGIN_IN, c.off_in, ty), FLAG, c.m, c.k, c.k + c.ld_pad, pc.ELT[ty]) == \
            pkg.prune24_form(addr(ORIGIN_IN, c.off_in, ty), addr(ORIGIN_IN, c.off_in, ty), c.m, c.k, c.k + c.ld_pad, pc.ELT[ty], STRIP)
    if c.cls == "span":
        spans = -(-c.m // c.span_rows)
        assert c.span_rows % 8 == 0 and 8 <= c.span_rows <= 64 and c.span_rows * c.k * 2 <= 64 * 1024 and c.k % 8 != 0 and c.ld_pad == 0
        assert c.m < 8 or spans > 1


def test_check_cases_reach_their_class(pkg):
    for c, ty in pc.fams(pc.CHECK_CASES):
        assert pkg.prune24_check_form(addr(ORIGIN_IN, c.off_in, ty), FLAG, c.m, c.k, c.k + c.ld_pad, pc.ELT[ty]) == c.cls


@pytest.mark.parametrize("ct", pc.fams(pc.COMPRESS_CASES), ids=pc.cid)
def test_compress_and_decompress_case_class(pkg, ct):
    c, ty = ct
    assert pc.query_compress(pkg, c, ty, addr(ORIGIN_IN, c.off, ty), BLOB) == c.cls
    assert pc.query_decompress(pkg, c, ty, BLOB, addr(ORIGIN_OUT, c.off, ty)) == c.dcls


@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("ct", pc.fams(pc.ONEPASS_CASES), ids=pc.cid)
def test_onepass_case_class_at_256_cus(pkg, ct, variant):
    c, ty = ct
    a_in = addr(ORIGIN_IN, c.off, ty)
    a_out = {"in_place": a_in, "no_out": None}.get(variant, addr(ORIGIN_OUT, c.off, ty))
    form, plan = pc.query_onepass(pkg, c, ty, a_in, a_out, None if variant == "no_blob" else BLOB, cus=256)
    assert form == pc.onepass_expect(c, ty, variant)
    if form.startswith("onepass"):
        assert plan == dict(flat=c.flat, lpr_log2=c.lpr, nj=c.nj, grid=plan["grid"], capped=False)
        assert c.k // 8 == c.nj << c.lpr and (c.k // 8) % (2 << c.lpr) != 0 or c.lpr == 6
        if c.nj > 1:
            assert (4 * plan["grid"]) % c.nj != 0 and plan["grid"] > 1
            tile_rows = -(-c.m * c.batch // 4) if c.flat else c.batch * -(-c.m // 4)
            assert -(-tile_rows // (64 >> c.lpr)) <= 7       # row groups: what the 8-fold guard behind the blob is sized for (Blob)
    elif form.startswith("fallback"):
        assert plan == dict(matrices=c.batch if form == "fallback_per_batch" else 1)
        # what the per-batch loops are there for: matrices whose bases differ in alignment
        if "odd matrices" in c.name:
            stride_bytes = c.m * (c.k + c.ld_pad) * pc.ELT[ty]
            assert stride_bytes % 16 == (8 if "8 B" in c.name else (14 if pc.ELT[ty] == 2 else 12))
        # the class of each matrix's own sm_prune24_* call
        if form == "fallback_per_batch" and a_out is not None:
            step = (c.m * (c.k + c.ld_pad) + c.gap) * pc.ELT[ty]
            got = tuple(pkg.prune24_form(a_in + b * step, a_out + b * step, c.m, c.k, c.k + c.ld_pad, pc.ELT[ty], c.alg) for b in range(c.batch))
            assert got == pc.PER_MATRIX[(c.name, pc.FAM[ty])], got


def test_pool_and_tile_forms_reach_their_class(pkg):
    for f, ty in pc.fams(pc.STRIP_FORMS):
        a, o = addr(ORIGIN_IN, f.off, ty), addr(ORIGIN_OUT, f.off, ty)
        ld = f.k + f.ld_pad
        assert f.batch * f.m * f.k == 4 * 14 ** 4
        if f.op == "prune":
            assert pkg.prune24_form(a, o, f.m, f.k, ld, pc.ELT[ty], STRIP) == f.cls and f.batch == 1
        elif f.op == "compress":
            assert pkg.compress24_form(a, BLOB, f.m, f.k, ld, f.batch, f.m * ld + f.gap, pc.ELT[ty]) == f.cls
        else:
            form, plan = pkg.prune24_compress24_form(a, o, f.m, f.k, ld, f.batch, f.m * ld + f.gap, BLOB, pc.ELT[ty], STRIP, cus=256)
            assert form == f.cls and plan["flat"] == (f.batch == 1)
    assert set(pc.CHECK_LAYOUTS) == {"strip_scalar", "strip_vec", "strip_flat_scalar", "strip_flat_vec"}
    for cls, (ld_pad, off) in pc.CHECK_LAYOUTS.items():
        for ty in pc.TYPES:
            assert pkg.prune24_check_form(addr(ORIGIN_IN, off, ty), FLAG, pc.POOL_M, pc.POOL_K, pc.POOL_K + ld_pad, pc.ELT[ty]) == cls
    for f, ty in pc.fams(pc.TILE_FORMS):
        a, o = addr(ORIGIN_IN, f.off, ty), addr(ORIGIN_OUT, f.off, ty)
        ld = f.k + f.ld_pad
        if f.op == "prune":
            assert pkg.prune24_form(a, o, pc.TILE_M, f.k, ld, pc.ELT[ty], TILE) == f.cls
        else:
            assert pkg.prune24_compress24_form(a, o, pc.TILE_M, f.k, ld, 1, pc.TILE_M * ld, BLOB if f.op == "onepass" else None, pc.ELT[ty], TILE, cus=256)[0] == f.cls


def test_every_class_has_a_case_per_type_and_a_specials_case(pkg):
    for ty in pc.TYPES:
        fam = pc.FAM[ty]
        mine = lambda cases: [c for c in cases if c.fam in ("any", fam)]
        prune = {c.cls for c in mine(pc.PRUNE_CASES)}
        want = set(pkg.PRUNE24_FORMS) - {"invalid", "empty"} - ({"tile2", "span"} if fam == "32" else set())
        assert prune == want, (ty, prune ^ want)
        assert {c.cls for c in mine(pc.CHECK_CASES)} == {"strip_scalar", "strip_vec", "strip_flat_scalar", "strip_flat_vec"}
        comp = {c.cls for c in mine(pc.COMPRESS_CASES)}
        assert comp == set(pkg.COMPRESS24_FORMS) - {"invalid", "empty"} - ({"rowspan"} if fam == "32" else set())
        assert {c.dcls for c in mine(pc.COMPRESS_CASES)} == {"vec", "scalar"}
        one = {(pc.onepass_expect(c, ty, v), c.flat) for c in mine(pc.ONEPASS_CASES) for v in pc.VARIANTS}
        kernels = ["onepass_tile", "onepass_strip"] + (["onepass_tile_noblob"] if fam == "16" else [])
        assert {(f, fl) for f in kernels for fl in (True, False)} <= one
        assert {f for f, _ in one} == set(pkg.PRUNE24_COMPRESS24_FORMS) - {"invalid", "empty"} - ({"fallback_tall_span", "onepass_tile_noblob"} if fam == "32" else set())
        assert {c.lpr for c in mine(pc.ONEPASS_CASES) if c.lpr} == {3, 4, 5, 6} and {c.nj for c in mine(pc.ONEPASS_CASES) if c.nj} == {1, 3, 9}
        # the specials: every STRIP form (vec and scalar prune, flat, rowspan and general compress, one-pass) and every TILE form
        strip = {f.cls for f in mine(pc.STRIP_FORMS)}
        assert strip >= {"strip_flat_vec", "strip_flat_scalar", "strip_vec", "strip_scalar", "flat", "general_scalar", "general_vec", "onepass_strip"} | ({"rowspan"} if fam == "16" else set())
        assert {f.batch > 1 for f in mine(pc.STRIP_FORMS) if f.op == "onepass"} == {True, False}      # the FLAT and the per-batch instantiation
        tile = {f.cls for f in mine(pc.TILE_FORMS)}
        assert tile == ({"tile2", "span", "element_vec", "element_scalar", "onepass_tile", "onepass_tile_noblob"} if fam == "16" else {"element_vec", "element_scalar", "onepass_tile"})
    # every write-capable entry point with a moved base, ld > k and guarded outputs
    assert any(c.off_out and c.ld_pad for c in pc.PRUNE_CASES) and any(c.off and c.ld_pad for c in pc.ONEPASS_CASES)
    assert any(c.off for c in pc.COMPRESS_CASES) and any(c.ld_pad and c.gap for c in pc.ONEPASS_CASES)


# ---------------------------------------------------------------------------------------------
# both sides of every threshold
# ---------------------------------------------------------------------------------------------
A, O = ORIGIN_IN, ORIGIN_OUT


def test_thresholds_of_prune(pkg):
    pf = lambda m, k, ld, elt, alg, a=A, o=O: pkg.prune24_form(a, o, m, k, ld, elt, alg, with_span_rows=True)
    # the span form: k 4095 | 4097 (4096 is the two-tile kernel's); rows per span: the first multiple of 8 with the best fill of 256 threads
    # (k = 2047: 8 rows are 1024 tiles, full; k = 147: 24 rows are 222 tiles, 87 %; k = 30: 64 rows are 128 tiles, 50 %)
    assert pf(9, 4095, 4095, 2, TILE) == ("span", 8) and pf(9, 4096, 4096, 2, TILE) == ("tile2", 0) and pf(9, 4097, 4097, 2, TILE) == ("element_scalar", 0)
    assert pf(9, 4100, 4100, 2, TILE) == ("element_vec", 0) and pf(9, 2047, 2047, 2, TILE) == ("span", 8) and pf(9, 2049, 2049, 2, TILE) == ("span", 8)
    assert pf(9, 147, 147, 2, TILE) == ("span", 24) and pf(9, 147, 148, 2, TILE) == ("element_vec", 0) and pf(9, 147, 147, 4, TILE) == ("element_scalar", 0)
    # k % 8 and ld % 8 (16-bit), ld % 4
    assert pf(9, 72, 72, 2, TILE)[0] == "tile2" and pf(9, 72, 80, 2, TILE)[0] == "tile2" and pf(9, 72, 76, 2, TILE)[0] == "element_vec"
    assert pf(9, 76, 80, 2, TILE)[0] == "element_vec" and pf(9, 76, 78, 2, TILE)[0] == "element_scalar" and pf(9, 76, 76, 2, TILE)[0] == "span"
    assert pf(9, 72, 72, 4, TILE)[0] == "element_vec" and pf(9, 72, 74, 4, TILE)[0] == "element_scalar" and pf(9, 75, 76, 4, TILE)[0] == "element_vec"
    for elt, per16 in ((2, 8), (4, 4)):
        assert pf(9, 72, 72, elt, STRIP)[0] == "strip_flat_vec" and pf(9, 72, 72 + per16, elt, STRIP)[0] == "strip_vec"
        assert pf(9, 72, 72 + per16 // 2, elt, STRIP)[0] == "strip_scalar" and pf(9, 76, 76, elt, STRIP)[0] == ("strip_scalar" if elt == 2 else "strip_vec")
        assert pf(9, 70, 72, elt, STRIP)[0] == "strip_vec" and pf(9, 75, 75, elt, STRIP)[0] == "strip_scalar"
    # pointer offsets of 0, 2, 4, 8 and 16 bytes, on either operand
    tile16 = {0: "tile2", 2: "element_scalar", 4: "element_scalar", 8: "element_vec", 16: "tile2"}
    span16 = {0: "span", 2: "element_scalar", 4: "element_scalar", 8: "element_vec", 16: "span"}
    strip = {0: "strip_flat_vec", 2: "strip_flat_scalar", 4: "strip_flat_scalar", 8: "strip_flat_scalar", 16: "strip_flat_vec"}
    tile32 = {0: "element_vec", 4: "element_scalar", 8: "element_scalar", 16: "element_vec"}
    for d in (0, 2, 4, 8, 16):
        for a, o in ((A + d, O), (A, O + d), (A + d, O + d)):
            assert pf(9, 72, 72, 2, TILE, a, o)[0] == tile16[d] and pf(9, 76, 76, 2, TILE, a, o)[0] == span16[d]
            assert pf(9, 72, 72, 2, STRIP, a, o)[0] == strip[d]
            if d != 2:
                assert pf(9, 72, 72, 4, TILE, a, o)[0] == tile32[d] and pf(9, 72, 72, 4, STRIP, a, o)[0] == strip[d]
        assert pkg.prune24_check_form(A + d, FLAG, 9, 72, 72, 2) == strip[d] and pkg.prune24_check_form(A, FLAG + 4, 9, 72, 72, 2) == "strip_flat_vec"


def test_thresholds_of_compress_and_decompress(pkg):
    cf = lambda m, k, ld, batch, stride, elt, a=A, b=BLOB: pkg.compress24_form(a, b, m, k, ld, batch, stride, elt)
    df = lambda m, k, ld, batch, stride, elt, a=A: pkg.decompress24_form(BLOB, a, m, k, ld, batch, stride, elt)
    # the rowspan form: ld 767 | 768
    assert cf(5, 147, 767, 1, 5 * 767, 2) == "rowspan" and cf(5, 147, 768, 1, 5 * 768, 2) == "general_vec" and cf(5, 767, 767, 1, 5 * 767, 2) == "rowspan"
    assert cf(5, 768, 768, 1, 5 * 768, 2) == "flat" and cf(5, 147, 767, 1, 5 * 767, 4) == "general_scalar"
    # k % 64, ld == k, ld % 8 (% 4)
    assert cf(9, 128, 128, 2, 9 * 128, 2) == "flat" and cf(9, 120, 120, 2, 9 * 120, 2) == "rowspan" and cf(9, 128, 136, 2, 9 * 136, 2) == "rowspan"
    assert cf(9, 128, 128, 2, 9 * 128, 4) == "flat" and cf(9, 120, 120, 2, 9 * 120, 4) == "general_vec" and cf(9, 128, 132, 2, 9 * 132, 4) == "general_vec"
    assert cf(9, 128, 130, 2, 9 * 130, 4) == "general_scalar" and cf(9, 128, 129, 1, 9 * 129, 2) == "rowspan"
    # strideA == m * ld against + 8 and + 1
    assert cf(9, 128, 128, 2, 9 * 128 + 8, 2) == "general_vec" and cf(9, 128, 128, 2, 9 * 128 + 1, 2) == "general_scalar"
    assert cf(9, 147, 147, 2, 9 * 147, 2) == "rowspan" and cf(9, 147, 147, 2, 9 * 147 + 8, 2) == "general_scalar" and cf(9, 147, 152, 2, 9 * 152 + 8, 2) == "general_vec"
    assert cf(9, 128, 128, 2, 9 * 128 + 4, 4) == "general_vec" and cf(9, 128, 128, 2, 9 * 128 + 1, 4) == "general_scalar"
    assert cf(9, 128, 128, 1, 9 * 128 + 1, 2) == "rowspan"      # one batch: the stride still decides the vector flag, not the form's contiguity
    # pointer offsets
    for d, want in ((0, "flat"), (2, "general_scalar"), (4, "general_scalar"), (8, "general_scalar"), (16, "flat")):
        assert cf(9, 128, 128, 2, 9 * 128, 2, A + d) == want
        assert df(9, 128, 128, 2, 9 * 128, 2, A + d) == ("vec" if want == "flat" else "scalar")
        if d != 2:
            assert cf(9, 128, 128, 2, 9 * 128, 4, A + d) == want
        assert cf(9, 128, 128, 2, 9 * 128, 2, A, BLOB + d) == ("flat" if d in (0, 16) else "invalid")
    assert df(9, 75, 80, 2, 9 * 80, 2) == "vec" and df(9, 75, 76, 2, 9 * 76, 2) == "scalar" and df(9, 75, 76, 2, 9 * 76, 4) == "vec"
    assert df(9, 75, 80, 2, 9 * 80 + 4, 2) == "scalar" and df(9, 75, 80, 2, 9 * 80 + 4, 4) == "vec" and df(9, 75, 80, 2, 9 * 80 + 1, 4) == "scalar"


def test_thresholds_of_the_onepass_kernel(pkg):
    def of(m, k, ld, batch, stride, elt, alg=TILE, a=A, o=O, blob=BLOB, cus=256):
        return pkg.prune24_compress24_form(a, o, m, k, ld, batch, stride, blob, elt, alg, cus=cus)
    for elt, per16 in ((2, 8), (4, 4)):
        # k % 64; ld and strideA multiples of 16 bytes
        assert of(36, 128, 128, 2, 36 * 128, elt)[0] == "onepass_tile" and of(36, 120, 120, 2, 36 * 120, elt)[0] == ("fallback_tall_span" if elt == 2 else "fallback_tall")
        assert of(36, 128, 128 + per16, 2, 36 * (128 + per16), elt)[0] == "onepass_tile" and of(36, 128, 128 + per16 // 2, 2, 36 * (128 + per16 // 2), elt)[0] == "fallback_tall"
        # strideA == m * ld against + 8 and + 1; m % 4 for FLAT
        assert of(36, 128, 128, 2, 36 * 128, elt)[1]["flat"] and not of(36, 128, 128, 2, 36 * 128 + 8, elt)[1]["flat"]
        assert of(36, 128, 128, 2, 36 * 128 + 1, elt)[0] == "fallback_per_batch"
        assert not of(38, 128, 128, 2, 38 * 128, elt)[1]["flat"] and of(38, 128, 128, 1, 38 * 128, elt)[1]["flat"]
        # m % 4 for `tall`: TILE only
        assert of(20, 147, 152, 2, 20 * 152, elt)[0] == "fallback_tall" and of(21, 147, 152, 2, 21 * 152, elt)[0] == "fallback_per_batch"
        assert of(21, 147, 152, 2, 21 * 152, elt, STRIP)[0] == "fallback_tall" and of(21, 147, 152, 2, 21 * 152 + 8, elt, STRIP)[0] == "fallback_per_batch"
        assert of(21, 147, 152, 1, 0, elt)[0] == "fallback_tall"
        # pointer offsets of A_in and A_out (a null A_out asks nothing), the blob's alignment
        for d in (0, 4, 8, 16) + ((2,) if elt == 2 else ()):
            want = "onepass_tile" if d in (0, 16) else "fallback_tall"
            assert of(36, 128, 128, 2, 36 * 128, elt, a=A + d)[0] == want and of(36, 128, 128, 2, 36 * 128, elt, o=O + d)[0] == want
            assert of(36, 128, 128, 2, 36 * 128, elt, blob=BLOB + d)[0] == ("onepass_tile" if d in (0, 16) else "invalid")
        assert of(36, 128, 128, 2, 36 * 128, elt, o=None)[0] == "onepass_tile" and of(36, 120, 120, 2, 36 * 120, elt, o=None)[0] == "not_supported"
        assert of(36, 120, 120, 2, 36 * 120, elt, STRIP, o=None)[0] == "fallback_tall" and of(36, 120, 120, 2, 36 * 120, elt, o=None, blob=None)[0] == "fallback_tall"
        # each lpr_log2, nj 1 against more
        for k, lpr, nj in ((64, 3, 1), (128, 4, 1), (256, 5, 1), (512, 6, 1), (192, 3, 3), (320, 3, 5), (384, 4, 3), (768, 5, 3), (1024, 6, 2), (1152, 4, 9)):
            p = of(36, k, k, 2, 36 * k, elt)[1]
            assert (p["lpr_log2"], p["nj"]) == (lpr, nj), k
            # the grid: one wave per 64 >> lpr tile rows, four waves per workgroup
            assert p["grid"] == -(-(-(-18 // (64 >> lpr))) // 4) and not p["capped"]
        # the grid just below and just above the cap of 8 workgroups per CU
        for cus in (256, 64, 304):
            m = pc.capped_rows(cus)
            below, above = of(m - 1, 512, 512, 1, 0, elt, cus=cus)[1], of(m, 512, 512, 1, 0, elt, cus=cus)[1]
            assert (below["grid"], below["capped"]) == (8 * cus, False) and (above["grid"], above["capped"]) == (8 * cus, True)
            assert of(m - 17, 512, 512, 1, 0, elt, cus=cus)[1]["grid"] == 8 * cus - 1     # (four tile rows fewer: one workgroup fewer)
    # the span form inside the fallback: 16-bit TILE with A_out on one tall contiguous matrix
    assert of(20, 147, 147, 2, 20 * 147, 2)[0] == "fallback_tall_span" and of(20, 147, 147, 2, 20 * 147, 4)[0] == "fallback_tall"
    assert of(20, 147, 147, 2, 20 * 147, 2, STRIP)[0] == "fallback_tall" and of(20, 147, 147, 2, 20 * 147, 2, blob=None, o=None)[0] == "fallback_tall"
    assert of(20, 4095, 4095, 1, 0, 2)[0] == "fallback_tall_span" and of(20, 4097, 4097, 1, 0, 2)[0] == "fallback_tall"
    assert of(20, 147, 147, 2, 20 * 147, 2, a=A + 8)[0] == "fallback_tall" and of(21, 147, 147, 2, 21 * 147, 2)[0] == "fallback_per_batch"
    assert of(36, 128, 128, 2, 36 * 128, 2, blob=None)[0] == "onepass_tile_noblob" and of(36, 128, 128, 2, 36 * 128, 4, blob=None)[0] == "onepass_tile"
    assert of(36, 128, 128, 2, 36 * 128, 2, STRIP, blob=None)[0] == "onepass_strip"


# ---------------------------------------------------------------------------------------------
# refusals, decided before any device call: dummy non-null pointers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", pc.TYPES)
@pytest.mark.parametrize("name", list(pc.REFUSALS))
def test_refusal_status_and_message(pkg, ty, name):
    rc, msg = pc.refused_call(pkg.lib(), ty, name, ORIGIN_IN, ORIGIN_OUT, BLOB, FLAG)
    assert rc == pc.REFUSALS[name][2], (rc, msg)
    assert pc.refusal_text(name, ty) in msg, msg


def test_refusals_cover_what_the_issue_lists():
    entries = {}
    for name, (entry, over, status, _) in pc.REFUSALS.items():
        entries.setdefault(entry, set()).add(("null" if None in over.values() and status == pc.INVALID else
                                              "ld<k" if "ld" in over else "alg" if "alg" in over and status == pc.INVALID else
                                              "blob" if "blob_off" in over else "not_supported"))
    assert entries["prune"] == {"null", "ld<k", "alg"} and entries["check"] == {"null", "ld<k"}
    assert entries["compress"] == {"null", "ld<k", "blob"} and entries["decompress"] == {"null", "ld<k"}
    assert entries["onepass"] == {"null", "ld<k", "alg", "blob", "not_supported"}


# ---------------------------------------------------------------------------------------------
# the references and the instruments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ty", pc.TYPES)
def test_numpy_strip_agrees_with_the_oracle_on_the_pool(orc, ty):
    """All 14^4 = 38 416 strips of the 14 special patterns: the restatement (sign-cleared bits as keys, top two, ties to the lower index,
    pruned positions +0) and the oracle agree bit for bit; so do the check's verdicts, strip by strip."""
    pool = pc.POOL[ty]
    assert len(pool) == len(set(pool)) == 14
    data = pc.pool_strips(ty)
    assert data.size == 4 * 38416 == pc.POOL_M * pc.POOL_K and np.unique(data.reshape(-1, 4), axis=0).shape[0] == 38416
    got = pc.np_strip_prune(data, pc.POOL_M, pc.POOL_K, ty)
    want = orc.prune24(data, pc.POOL_M, pc.POOL_K, pc.POOL_K, orc.STRIP, bf16=ty == "bf16")
    assert np.array_equal(got, want)
    # the same strips under another row length (ragged rows do not cut a strip here: 28 % 4 == 0)
    assert np.array_equal(orc.prune24(data, 5488, 28, 28, orc.STRIP, bf16=ty == "bf16"), want)
    dense = pc.np_strip_nnz_gt2(data, 38416, 4, ty)
    for i in list(range(0, 38416, 97)) + [38415]:
        assert orc.prune24_check(np.ascontiguousarray(data[4 * i:4 * i + 4]), 1, 4, 4) == int(dense[i])
    assert orc.prune24_check(want, pc.POOL_M, pc.POOL_K, pc.POOL_K) == 0 and not pc.np_strip_nnz_gt2(want, pc.POOL_M, pc.POOL_K, ty).any()
    # ragged k: the last strip is completed with zeros
    rng = np.random.default_rng(5)
    for k in (1, 2, 3, 5, 7, 75):
        d = pc.rand_bits(rng, 6 * k, ty, ties=True)
        assert np.array_equal(pc.np_strip_prune(d, 6, k, ty), orc.prune24(d, 6, k, k, orc.STRIP, bf16=ty == "bf16")), k


@pytest.mark.filterwarnings("ignore:invalid value encountered in cast")     # (signalling NaNs of the pool, converted to fp64)
def test_pool_patterns_are_what_their_names_say():
    f16 = np.array(pc.POOL["f16"], dtype=np.uint16).view(np.float16).astype(np.float64)
    f32 = np.array(pc.POOL["f32"], dtype=np.uint32).view(np.float32).astype(np.float64)
    bf = (np.array(pc.POOL["bf16"], dtype=np.uint32) << 16).view(np.float32).astype(np.float64)
    for v, tiny, sub, nrm, big in ((f16, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 65504.0),
                                   (bf, 2.0 ** -133, 2.0 ** -126 - 2.0 ** -133, 2.0 ** -126, float(np.float32(3.3895313892515355e38))),
                                   (f32, 2.0 ** -149, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126, float(np.finfo(np.float32).max))):
        assert list(v[:11]) == [0.0, 0.0, tiny, -tiny, sub, nrm, 1.0, -1.0, big, np.inf, -np.inf] and np.signbit(v[1]) and not np.signbit(v[0])
        assert np.isnan(v[11:]).all() and np.signbit(v[12])
    for ty in pc.TYPES:
        assert pc.POOL[ty][12] == (1 << (8 * pc.ELT[ty])) - 1 and pc.POOL[ty][11] == pc.QNAN[ty]
        q = np.array([pc.QNAN[ty], pc.SENT[ty]], dtype=pc.NP[ty])
        v = q.view(np.float16).astype(np.float64) if ty == "f16" else (q.astype(np.uint32) << (16 if ty == "bf16" else 0)).view(np.float32).astype(np.float64)
        assert np.isnan(v[0]) and np.isfinite(v[1])


@pytest.mark.parametrize("ty", pc.TYPES)
def test_pad_builder(ty):
    rng = np.random.default_rng(7)
    for (m, k, ld_pad, batch, gap, off, fill) in ((5, 7, 3, 2, 5, 1, "nan"), (4, 8, 0, 1, 0, 0, "sent"), (3, 147, 620, 1, 0, 4, "nan")):
        data = pc.rand_bits(rng, batch * m * k, ty)
        p = pc.Pad(ty, m, k, ld_pad, batch, gap, off, fill=fill, data=data)
        assert np.unique(p.idx).size == p.idx.size == batch * m * k and np.array_equal(p.h[p.idx], data)
        assert p.idx[0] == pc.GUARD + off and p.idx[-1] == pc.GUARD + off + (batch - 1) * (m * (k + ld_pad) + gap) + (m - 1) * (k + ld_pad) + k - 1
        out = np.ones(p.h.size, dtype=bool)
        out[p.idx] = False
        assert (p.h[out] == (pc.QNAN[ty] if fill == "nan" else pc.SENT[ty])).all() and out[:pc.GUARD].all()
        # the buffer ends GUARD elements behind the last logical one: no room for a whole last row of ld
        assert p.h.size - 1 - p.idx[-1] == pc.GUARD
        assert p.addr(ORIGIN_IN) % 16 == (off * pc.ELT[ty]) % 16 and (pc.GUARD * pc.ELT[ty]) % 16 == 0
    assert not np.isnan(pc.rand_bits(rng, 1000, ty).astype(np.uint32).view(np.float32) if ty == "f32" else np.zeros(1)).any()
