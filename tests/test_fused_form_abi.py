"""sm_spmma_fused_form -- the dispatch rule of the fused 16-bit 2:4 matmul as a host-side query -- without a GPU: the symbol, its
arity and every status; the form of every shape tests/test_gpu_strided16.py runs and of every shape an existing test attributes to
a form, PINNED at 256 compute units (the MI355X); and threshold pairs around each boundary of the rule.  A dispatch constant that
moves makes this file fail instead of silently leaving a kernel without coverage."""
import ctypes
import os

import pytest

import test_gpu_parity as tp
import test_gpu_strided16 as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
CUS = 256


def form(pkg, m, n, k, batch=1, cus=CUS, **kw):
    return pkg.spmma_fused_form(m, n, k, batch=batch, cus=cus, **kw)


def test_symbol_exported_declared_and_bound(pkg):
    pkg.build()
    header = open(os.path.join(ROOT, "include", "sparsifyme.h")).read()
    L = ctypes.CDLL(pkg.LIB_PATH)
    assert "sm_spmma_fused_form(" in header and "sm_spmma_fused_form" in pkg.EXPORTED_SYMBOLS and hasattr(L, "sm_spmma_fused_form")
    # m, n, k, lda, batch, count, strideA, strideB, strideC, beta, flags, cus, form
    sig = pkg._SIGS["sm_spmma_fused_form"]
    assert len(sig) == 13 and sig[:9] == [ctypes.c_size_t] * 9 and sig[9] == ctypes.c_float and sig[10] == ctypes.c_uint and sig[11] == ctypes.c_size_t
    # the header's SM_FUSED_FORM_* values are the binding's names, in order
    for value, name in enumerate(pkg.FUSED_FORMS):
        assert "#define SM_FUSED_FORM_%s %d" % (name.upper(), value) in header
    for name, value in (("A_ALIGNED", 1), ("B_ALIGNED", 2), ("C_ALIGNED", 4), ("WORKSPACE", 8), ("EPILOGUE", 16)):
        assert "#define SM_FUSED_FLAG_%s %du" % (name, value) in header and getattr(pkg, "FUSED_FLAG_" + name) == value


def test_statuses(pkg):
    fn = pkg.lib().sm_spmma_fused_form
    out = ctypes.c_int(-1)
    ok = (128, 64, 64, 64, 1, 1, 128 * 64, 0, 128 * 64, 0.0, 7, CUS)
    assert fn(*ok, ctypes.byref(out)) == 0 and pkg.FUSED_FORMS[out.value] == "direct64"
    assert fn(*ok, None) == INVALID                                                   # form == NULL
    assert fn(128, 64, 64, 63, 1, 1, 0, 0, 0, 0.0, 7, CUS, ctypes.byref(out)) == INVALID     # lda < k
    assert fn(128, 64, 64, 64, 1, 9, 0, 0, 0, 0.0, 7, CUS, ctypes.byref(out)) == INVALID     # more problems than one launch takes
    assert fn(128, 64, 64, 64, 1, 1, 0, 0, 0, 0.0, 32, CUS, ctypes.byref(out)) == INVALID    # an unknown flag
    assert fn(128, 64, 64, 64, 1, 1, 0, 0, 0, 0.0, 7 | 8 | 16, CUS, ctypes.byref(out)) == INVALID   # workspace and epilogue
    assert b"sm_spmma_fused_form" in pkg.lib().sm_last_error()
    # cus == 0 asks the device; without one the rule answers for 256 compute units
    assert fn(*ok[:-1], 0, ctypes.byref(out)) == 0 and pkg.FUSED_FORMS[out.value] == "direct64"
    # nothing to do
    for kw in (dict(count=0), dict(batch=0)):
        assert form(pkg, 128, 64, 64, **kw) == "empty"
    assert form(pkg, 0, 64, 64) == "empty" and form(pkg, 128, 0, 64) == "empty"


def _query(pkg, m, n, k, lay, cus=CUS, **kw):
    """The query for a test_gpu_strided16 layout (what Problem.form asks on the device, from the layout alone)."""
    L = ts.Layout(**lay)
    lda = k + L.lda_pad
    return pkg.spmma_fused_form(m, n, k, lda, L.batch, kw.pop("count", 1), m * lda + L.gapA, 0 if L.gapB is None else k * n + L.gapB, m * n + L.gapC,
                                kw.pop("beta", L.beta), a_aligned=L.offA % 8 == 0, b_aligned=L.offB % 8 == 0, c_aligned=L.offC % 8 == 0, cus=cus, **kw)


def test_pinned_forms_of_the_strided_cases(pkg):
    """Every case of tests/test_gpu_strided16.py reaches the form it is pinned to; together they reach every form."""
    seen = set()
    for f, shape_of, lname in ts.FUSED_CASES:
        assert _query(pkg, *ts.FORM_SHAPES[shape_of], ts.LAYOUTS[lname]) == f, (shape_of, lname)
        seen.add(f)
    for f, shape_of, lname in ts.TALL_CASES:
        assert _query(pkg, *ts.TALL_SHAPES[shape_of], ts.TALL_LAYOUTS[lname]) == f, (shape_of, lname)
        seen.add(f)
    for f, shape in ts.FORM_SHAPES.items():   # the grouped and the integer-exact cases
        for count in (1, 3):
            assert _query(pkg, *shape, dict(lda_pad=8, gapA=64, gapB=8, gapC=8), count=count) == f, (f, count)
    for f, shape in ts.TALL_SHAPES.items():
        assert _query(pkg, *shape, dict(batch=1, offA=8, offB=8, offC=8)) == f
    for name, (shape, lay) in ts.REFUSALS.items():
        assert _query(pkg, *shape, lay) == "not_taken", name
    m, n, k, batch = ts.STREAMK_SHAPE
    for beta in (0.0, -2.0):
        lay = dict(lda_pad=8, gapA=64, gapC=8, batch=batch)
        assert _query(pkg, m, n, k, lay, beta=beta, workspace=True) == "streamk" and _query(pkg, m, n, k, lay, beta=beta) == "big"
    lay = dict(lda_pad=8, gapA=64, gapB=8, gapC=8, batch=batch)   # the integer-exact case: per-batch B
    assert _query(pkg, m, n, k, lay, workspace=True) == "streamk" and _query(pkg, m, n, k, lay) == "big"
    seen.add("streamk")
    for f, shape in ts.EX_SHAPES.items():
        assert _query(pkg, *shape, dict(lda_pad=8, gapA=64, gapB=8, gapC=8), beta=-2.0, epilogue=True) == f
    assert seen == set(pkg.FUSED_FORMS) - {"not_taken", "empty"}, "a form has no strided case"


def test_pinned_forms_of_the_named_parity_tests(pkg):
    """The shapes tests/test_gpu_parity.py attributes to a form by name, docstring or comment."""
    for shape, f in tp.FUSED_ROW_FORMS.items():                  # test_fused_equals_staged
        m, n, k, batch = shape
        for sB in (0, k * n):
            assert form(pkg, m, n, k, batch, strideB=sB) == f, shape
    assert set(tp.FUSED_ROW_FORMS.values()) >= {"direct64", "direct128", "direct128_nt", "astat", "widep", "wide", "big"}
    for m, n, k, batch in [(2045, 256, 128, 32), (2045, 264, 576, 32), (2048, 512, 576, 32), (128, 256, 128, 1), (100, 264, 576, 1)]:   # test_fused_big_form_equals_staged
        for kw in (dict(), dict(strideB=k * n), dict(beta=-2.0), dict(count=3)):
            assert form(pkg, m, n, k, batch, **kw) == "big", (m, n, k, batch, kw)
    for m, n, k, batch in [(3136, 512, 128, 24), (2100, 264, 256, 32), (4096, 384, 64, 17), (2049, 520, 192, 32)]:   # test_fused_astat_many_panels_equals_staged
        assert form(pkg, m, n, k, batch) == "astat" and form(pkg, m, n, k, batch, count=2) == "astat"
    for m, n, k, batch in [(12544, 64, 147, 2), (196, 64, 147, 3), (196, 64, 147, 4), (130, 128, 72, 2), (77, 24, 8, 4), (300, 72, 200, 1), (513, 64, 100, 1),
                           (520, 64, 100, 1), (128, 64, 333, 2), (40, 128, 190, 2)]:   # test_fused_span_form_equals_staged
        want = "not_taken" if (batch * m * k) % 8 else "span"    # an operand that does not end on a 16-byte boundary is declined
        assert form(pkg, m, n, k, batch) == want and form(pkg, m, n, k, batch, count=3) == want
    for m, n, k, batch in [(196, 1, 9, 64), (49, 1, 25, 96), (784, 1, 9, 33), (100, 3, 18, 8), (64, 7, 64, 4), (3136, 1, 9, 512), (8, 1, 8, 1)]:   # test_fused_thin_vs_oracle
        assert form(pkg, m, n, k, batch) == "thin" and form(pkg, m, n, k, batch, beta=-2.0) == "thin"
    for m, n, k, batch in [(196, 512, 2048, 4), (100, 264, 2304, 3), (300, 256, 2304, 2), (64, 136, 4608, 1), (600, 512, 3072, 5)]:   # test_fused_streamk_vs_oracle
        for beta in (0.0, -2.0):
            assert form(pkg, m, n, k, batch, beta=beta, workspace=True) == "streamk"
            assert form(pkg, m, n, k, batch, beta=beta) != "streamk"


def test_threshold_pairs(pkg):
    """Both sides of every boundary of the rule, at 256 compute units (m = 200, one batch unless said)."""
    # n: 64 / 72, 128 / 136, 256 / 264
    assert [form(pkg, 200, n, 192) for n in (64, 72)] == ["direct64", "direct128"]
    assert [form(pkg, 200, n, 192) for n in (128, 136)] == ["direct128", "widep"]
    assert [form(pkg, 200, n, 64) for n in (128, 136, 256, 264)] == ["direct128", "direct128", "direct128", "astat"]   # a single stage: direct up to n = 256
    assert [form(pkg, 200, n, 192) for n in (256, 264)] == ["widep", "astat"]
    assert [form(pkg, 200, n, 1088) for n in (256, 264)] == ["wide_nt", "wide"]
    assert [form(pkg, 100, n, 192) for n in (128, 136)] == ["direct128", "big"]      # one 128-row tile: the 256-row form fills the rounds as well
    # k: 64 / 128, 512 / 576, 1024 / 1088
    assert [form(pkg, 200, 200, k) for k in (64, 128)] == ["direct128", "widep"]
    assert [form(pkg, 200, 104, k) for k in (448, 512, 576)] == ["direct128", "direct128_nt", "direct128_nt"]
    assert [form(pkg, 200, 264, k) for k in (512, 576)] == ["astat", "widep"]
    assert [form(pkg, 200, 264, k) for k in (1024, 1088)] == ["widep", "wide"]
    assert [form(pkg, 200, 200, k) for k in (1024, 1088)] == ["widep", "wide_nt"]
    assert [form(pkg, 200, 40, k) for k in (64, 576, 1088)] == ["direct64"] * 3
    # the A-stationary form: beta == 0, an aligned C with strideC % 8 == 0, no epilogue
    assert form(pkg, 200, 264, 128) == "astat"
    assert form(pkg, 200, 264, 128, beta=-2.0) == "widep"
    assert form(pkg, 200, 264, 128, c_aligned=False) == "widep"
    assert form(pkg, 200, 264, 128, batch=2, strideC=200 * 264 + 3) == "widep" and form(pkg, 200, 264, 128, batch=2, strideC=200 * 264 + 8) == "astat"
    assert form(pkg, 200, 264, 128, epilogue=True) == "wide"
    # persistent wide: no epilogue
    assert form(pkg, 200, 200, 128) == "widep" and form(pkg, 200, 200, 128, epilogue=True) == "wide_nt"
    # stream-K: a workspace, and not on the A-stationary shapes
    assert form(pkg, 196, 512, 4608, batch=3, workspace=True) == "streamk" and form(pkg, 196, 512, 4608, batch=3) != "streamk"
    assert form(pkg, 196, 512, 512, batch=3, workspace=True) == form(pkg, 196, 512, 512, batch=3) == "astat"
    assert form(pkg, 200, 104, 4608, workspace=True) == "direct128_nt"              # n <= 128: never
    # the big form against the 128-row kernels: round efficiencies at THIS many compute units
    assert form(pkg, 2045, 256, 128, batch=32) == "big" and form(pkg, 200, 256, 128) == "widep"
    assert form(pkg, 3190, 256, 192, batch=24, cus=256) == "widep" and form(pkg, 3190, 256, 192, batch=24, cus=304) == "big"
    # thin and span: one tall contiguous A
    assert form(pkg, 200, 3, 18) == "thin" and form(pkg, 200, 3, 18, lda=24) == "not_taken" and form(pkg, 200, 3, 18, epilogue=True) == "not_taken"
    assert form(pkg, 200, 3, 18, a_aligned=False) == "not_taken" and form(pkg, 200, 3, 18, b_aligned=False, c_aligned=False) == "thin"
    assert form(pkg, 3, 3, 18) == "not_taken"                                         # 108 bytes of A: not whole 16-byte pieces
    assert form(pkg, 200, 72, 200) == "span" and form(pkg, 200, 136, 200) == "not_taken" and form(pkg, 200, 72, 200, lda=208) == "not_taken"
    assert form(pkg, 200, 72, 200, batch=2, strideA=200 * 200 + 8) == "not_taken" and form(pkg, 200, 72, 200, c_aligned=False) == "not_taken"
    # what no form takes
    for kw in (dict(lda=196), dict(batch=2, strideA=200 * 192 + 4), dict(batch=2, strideB=192 * 104 + 4), dict(a_aligned=False), dict(b_aligned=False)):
        assert form(pkg, 200, 104, 192, **kw) == "not_taken", kw
    assert form(pkg, 200, 100, 192) == "not_taken"                                    # n % 8
    assert form(pkg, 200, 104, 192, count=3, c_aligned=False) == "not_taken" and form(pkg, 200, 104, 192, c_aligned=False) == "direct128"
    assert form(pkg, 1 << 31, 104, 192) == "not_taken"


def test_taken_or_not_is_independent_of_the_cu_count(pkg):
    """sm::spmma_fused16_takes_exact (asked by sm_prune24_spmma_* before it touches A) is the same rule with no workspace and no
    epilogue at a fixed CU count: whether a call is taken must therefore not depend on the CU count -- over a grid of small shapes."""
    for m in (4, 130):
        for n in (3, 8, 72, 136, 264):
            for k in (8, 18, 64, 100, 192):
                for lda in (k, k + 8):
                    for batch, gapA in ((1, 0), (2, 0), (2, 8), (2, 4)):
                        for al in (True, False):
                            got = {form(pkg, m, n, k, batch, cus=c, lda=lda, strideA=m * lda + gapA, a_aligned=al) in ("not_taken", "empty") for c in (8, 64, 256, 304)}
                            assert len(got) == 1, (m, n, k, lda, batch, gapA, al)
