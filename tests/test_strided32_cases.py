"""The instruments of tests/test_gpu_strided32.py, checked without a GPU: for every case the layout builder's gather is the inverse of its
scatter, every word outside the logical operands is poison or sentinel, bases and strides meet (or by design break) the alignment
conditions the case's launch class needs (CLASS_NEEDS), the `ties` premise holds for the reference alone, the oracle-pruned A has at most
two non-zeros per strip, every launch class of the docstring table has a case of each data kind, and every REFUSALS entry returns its
status from a call with dummy non-null pointers (each is decided before any device call)."""
import ctypes

import numpy as np
import pytest

import test_gpu_strided32 as s32   # (as a module: its test functions must not be collected here)

CASES = s32.ALL_CASES
_cid = s32._cid


def _family(cls):
    return "staged" if cls.startswith("staged") else "split" if cls.startswith(("split", "span")) else "mm"


def test_every_class_of_the_table_has_cases():
    have = {c.cls for c in CASES} | {"generic<128,64>"}     # the latter: test_dense_generic_128x64_tiles, sized on the device
    assert have == set(s32.CLASS_NEEDS)
    for cls in s32.CLASS_NEEDS:
        for part in cls.split(", "):
            assert part in s32.__doc__, f"{cls} is missing from the docstring table"
    assert len(set(CASES)) == len(CASES)
    # both batch modes per family of classes, and every layout the families are asked to run
    for fam, names in (("mm", s32.FOLDING + s32.PER_BATCH), ("staged", s32.STAGED_LAYOUTS), ("split", s32.SPLIT_LAYOUTS)):
        assert set(names) <= {c.lname for c in CASES if c.fam == fam}
    for cls in s32.CLASS_NEEDS:
        folds = {s32.case_facts(c)["fold"] for c in CASES if c.cls == cls}
        if cls in ("dma<64,64>", "dma<64,128>"):
            assert folds == {False}          # a fold makes M > 64: these classes are the witness that no fold fired
        elif cls.startswith("span"):
            assert folds == {True}
        elif cls != "generic<128,64>":
            assert folds == {False, True}, cls


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_case_meets_the_conditions_of_its_class(case):
    f = s32.case_facts(case)
    assert s32.CLASS_NEEDS[case.cls](f), f
    others = [cls for cls, need in s32.CLASS_NEEDS.items() if cls != case.cls and _family(cls) == case.fam and need(f)]
    assert not others, f"the case also meets {others}"
    lay = s32.layout_of(case.fam, case.lname)
    if case.lname in s32.PER_BATCH:
        assert not f["fold"]
    if case.lname in s32.FOLDING:
        assert f["fold"]
    if case.lname == "sC+3":      # batch 0 on the vector store, batch 1 off it
        assert lay.offC % 4 == 0 and (case.m * case.n + lay.gapC) % 4 != 0
    assert case.k <= 256 and case.m % 128 != 0


def test_big_generic_shape_reaches_its_class_at_any_cu_count():
    for cus in (64, 104, 256, 304):
        for per_batch in (False, True):
            m, n, k, lname = s32.big_generic_shape(cus, per_batch)
            f = s32.facts("mm", m, n, k, s32.layout_of("mm", lname))
            assert not f["dma"] and f["fold"] != per_batch and f["small_tiles"] >= 32 * cus and n % 64 != 0
            if cus == 256:
                assert s32.CLASS_NEEDS["generic<128,64>"](f)
                lay = s32.layout_of("mm", lname)
                assert 4 * (lay.batch * (m * k + lay.gapA) + k * n + lay.batch * m * n + 6 * s32.GUARD) < 150e6


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_layout_builder_and_references(orc, case):
    for p in s32.problems(case):
        lay = p.lay
        a, b, c0 = s32.draw(np.random.default_rng(s32._seed(p.kind, *(x for x in case if x is not None))), p.kind, p.batch, p.nb, p.m, p.n, p.k)
        # gather is the inverse of scatter; the logical operands do not overlap and lie inside the guards
        for buf, idx, want in ((p.A, p.iA, a), (p.B, p.iB, b)):
            assert np.array_equal(buf[idx], s32.bits(want).reshape(-1)) and np.unique(idx).size == idx.size
            assert idx.min() >= s32.GUARD and idx.max() < buf.size - s32.GUARD + 1
            out = np.ones(buf.size, dtype=bool)
            out[idx] = False
            assert (buf[out] == s32.QNAN).all() and np.isnan(buf[out].view(np.float32)).all() and out[: s32.GUARD].all() and out[-s32.GUARD + 1:].all()
            assert not np.isnan(buf[idx].view(np.float32)).any()
        assert np.unique(p.iC).size == p.iC.size and p.iC.min() >= s32.GUARD and p.iC.max() < p.C.size - s32.GUARD + 1
        assert (p.C[p.outC] == s32.SENT).all() and p.outC[: s32.GUARD].all() and p.outC[-s32.GUARD + 1:].all() and p.outC.sum() == p.C.size - p.iC.size
        if p.reads_c:
            assert np.array_equal(p.C[p.iC], s32.bits(c0).reshape(-1))
        else:
            assert (p.C == s32.SENT).all()
        # strides and bases as the call passes them
        assert p.iA[0] == p.baseA and p.iA[-1] == p.baseA + (p.batch - 1) * p.sA + (p.m - 1) * p.lda + p.k - 1
        assert p.iC[-1] == p.baseC + (p.batch - 1) * p.sC + p.m * p.n - 1 and p.iB[-1] == p.baseB + (p.nb - 1) * (p.k * p.n + (lay.gapB or 0)) + p.k * p.n - 1
        assert (p.baseA % 4, p.baseB % 4, p.baseC % 4) == (lay.offA % 4, lay.offB % 4, lay.offC % 4)
        # the oracle-pruned A: at most two non-zeros per strip (ragged k: the last strip is shorter), a subset of A
        pr = p.pruned_bits(orc).view(np.float32).reshape(p.batch * p.m, p.k)
        kc = (p.k + 3) // 4 * 4
        strips = np.zeros((p.batch * p.m, kc), dtype=np.float32)
        strips[:, : p.k] = pr
        assert ((strips.reshape(-1, 4) != 0).sum(axis=1) <= 2).all()
        full = p.a_compact().view(np.float32).reshape(p.batch * p.m, p.k)
        assert ((pr == full) | (pr == 0)).all()
        if p.kind == "ties":
            p.assert_ties_premise(orc)
            for pruned in (False, True):
                ref, _ = p.reference(orc, pruned)
                assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref) and np.abs(ref).max() < 2.0 ** 24
        else:
            ref, scale = p.reference(orc, True)
            assert np.isfinite(ref).all() and (scale >= np.abs(ref) - 1e-12).all()


def test_threshold_cases_sit_on_both_sides():
    for fam, ext, vals, fixed, k, crosses in s32.THRESHOLDS:
        lay = s32.layout_of(fam, "all")
        cls = []
        for v in vals:
            d = dict(fixed, **{ext: v})
            c = s32.Case(fam, None, d["m"], d["n"], k, "all")
            f = s32.case_facts(c)
            cls.append([name for name, need in s32.CLASS_NEEDS.items() if need(f) and _family(name) == fam])
        assert len(cls[0]) == 1 and len(cls[1]) == 1 and (cls[0] != cls[1]) == crosses, (fam, ext, vals, cls)
        assert lay.batch == 2


# ---- the refusals, without a device: dummy non-null pointers that carry the layout's base offsets
BASE = 0x100000


@pytest.mark.parametrize("name", list(s32.REFUSALS))
def test_refusals_are_decided_before_any_device_call(pkg, name):
    entries, lname, over, k, status = s32.REFUSALS[name][:5]
    L = pkg.lib()
    m, n = s32.REFUSAL_MN[0], (s32.REFUSALS[name] + (s32.REFUSAL_MN[1],))[5]
    p = s32.Problem(m, n, k, s32.Layout(**s32.LAYOUTS[lname]), "ties", np.random.default_rng(0))
    A, B, C = (BASE * (i + 1) + 4 * getattr(p, "base" + w) for i, w in enumerate("ABC"))
    assert (BASE % 16, s32.GUARD % 4) == (0, 0)
    for entry in entries:
        assert entry != "staged"
        for planes in (2, 3):
            rc = s32.call_entry(L, entry, A, B, C, p, planes=planes, ws=BASE * 8, ws_bytes=1 << 40, **over)
            assert rc == status, f"{name} {entry} planes {planes}: status {rc}: {L.sm_last_error().decode()}"


def test_refusals_cover_what_the_header_states():
    R = s32.REFUSALS
    assert {n.split()[1] for n in R if n.startswith("fused")} == {"lda+1", "sA+2", "sB+2", "a_off1", "b_off1"}
    assert {n.split(" ", 1)[1] for n in R if n.startswith("split")} == {"sC+3", "c_off1", "sB+16", "ragged k lda+4", "ragged k sA+64", "span k=147 n=104"}
    assert R["lda<k"][0] == s32.TAKES_LDA and R["lda<k"][4] == s32.INVALID and R["lda<k"][2]["lda"] < R["lda<k"][3]
    assert all(v[4] == s32.NOT_SUPPORTED for n, v in R.items() if n != "lda<k")
    assert ctypes.sizeof(ctypes.c_float) == 4
