"""The instruments of tests/test_gpu_gemm_batched.py, checked without a GPU: every case meets CLASS_NEEDS of its class and of no other
class of its entry point (the CU-dependent ones at 64, 104, 256 and 304 CUs), every class of the docstring table has cases, the
placement builder's gather is the inverse of its scatter, every word outside the logical operands is poison or sentinel, the bases meet
the header's alignment precondition and no more (multiples of 16 bytes that are no multiples of 256; f64 `odd8`: 8 mod 16), the entries
lie at non-monotonic offsets with unequal gaps, the `ties` premise holds for the reference alone, every case's buffers stay under
CAP_BYTES, the mirror of the stream-K rule agrees with sm_spmma_fused_streamk_plan (which answers for 256 CUs without a device), and
every REFUSALS entry returns its status from a call with dummy non-null pointers (each is decided before any device call)."""
import collections
import re

import numpy as np
import pytest

import test_gpu_gemm_batched as gb   # (as a module: its test functions must not be collected here)

CASES = gb.ALL_CASES
_cid = gb._cid
CUS = (64, 104, 256, 304)
DEVICE_SIZED = {"f64 dma<128,128>", "f32 generic<128,64>"}   # test_f64_big_tiles, test_f32_generic_128x64
STAGE = {"f64": 16, "f32": 32, "f16": 64, "f16_ws": 64}
MATRIX_CORE = [cls for e in gb.ENTRIES for cls in gb.CLASS_NEEDS[e] if not any(w in cls for w in ("fma", "generic", "atr", "cfg"))]


def _tile(cls):
    """(rows of the row-major view = the call's n, columns = the call's m) of a matrix-core class's tile."""
    if "span" in cls:
        return 128, int(re.search(r"<(\d+)>", cls).group(1))
    if "big" in cls or "streamk" in cls:
        return 256, 256
    bm, bn = re.search(r"<(\d+),(\d+)>", cls).groups()
    return int(bm), int(bn)


def test_every_class_of_the_table_has_cases():
    names = [cls for e in gb.ENTRIES for cls in gb.CLASS_NEEDS[e]]
    assert len(set(names)) == len(names) and len(set(CASES)) == len(CASES)
    assert {c.cls for c in CASES} | DEVICE_SIZED == set(names)
    # the number of cases per class: a row deleted from (or added to) a case list shows here
    count = collections.Counter(c.cls for c in CASES)
    want = {"f64 dma<64,64>": 16, "f64 fma": 8, "f32 dma<64,64>": 3, "f32 dma<64,128>": 6, "f32 dma<128,64>": 6, "f32 dma<128,128>": 3,
            "f32 generic<64,64>": 4, "f32 T generic<64,64>": 3, "twin span<64>": 4, "twin span<128>": 4, "dma<128,64>": 4, "dma<64,128>": 4,
            "dma<128,128>": 4, "cfg<128,128,T> vec8": 4, "cfg<128,128,T> vec4->1": 6, "cfg<128,128,T> vec1": 3}
    assert {cls: count[cls] for cls in set(names) - DEVICE_SIZED} == {cls: want.get(cls, 2) for cls in set(names) - DEVICE_SIZED}
    assert len(CASES) == 118
    for cls in names:
        assert cls in gb.__doc__, f"{cls} is missing from the docstring table"
    for f in ("gemm_f32.hip", "gemm_f16.hip", "spmma_f16_fused.hip"):
        assert f in gb.__doc__
    # every case runs both data kinds (run_case), the device-sized tests are parametrised over them
    assert gb.KINDS == ("ties", "uniform") and gb.ABS == ((1.0, 0.0), (0.5, -2.0))
    for cls in set(names) - DEVICE_SIZED:
        mine = [c for c in CASES if c.cls == cls]
        assert {c.ab for c in mine} == {0, 1}, f"{cls}: both (alpha, beta)"
        assert all(c.entry == next(e for e in gb.ENTRIES if cls in gb.CLASS_NEEDS[e]) for c in mine)
    for entry in gb.ENTRIES:
        lays = [gb.LAYOUTS[c.lname] for c in CASES if c.entry == entry]
        assert any(l.sharedB for l in lays) and any(not l.sharedB for l in lays) and any(l.dupA for l in lays) and any(l.second for l in lays), entry
        assert all(not l.odd8 for l in lays) or entry == "f64"
    assert any(gb.LAYOUTS[c.lname].odd8 for c in CASES if c.cls == "f64 dma<64,64>") and gb.LAYOUTS[gb.F64_BIG_LAYOUT[16]].odd8
    # matrix-core classes: a ragged last tile in both m and n, at least two k stages, batch >= 2 -- in ONE case
    for cls in set(MATRIX_CORE) - DEVICE_SIZED:
        tn, tm = _tile(cls)
        mine = [c for c in CASES if c.cls == cls and c.batch >= 2]
        if cls == "f32 T dma<64,64>":     # ta = T needs m >= k and the class m <= 64: two 32-deep stages leave m = 64 only
            assert any(c.n % tn and c.m % tm for c in mine) and any(c.n % tn and c.k >= 64 for c in mine)
            continue
        assert any(c.n % tn and c.m % tm and c.k >= 2 * STAGE[c.entry] for c in mine), cls
    m, n, _ = gb.f64_big_shape(256)
    assert m % 128 and n % 128 and m > 128 and n > 128
    # what the issue names
    f64 = [c for c in CASES if c.cls == "f64 dma<64,64>"]
    assert {c.m for c in f64} == {2, 66, 130} and {c.n for c in f64} == {40, 64, 65, 200} and {c.k for c in f64} == {16, 32, 48}
    fma = [c for c in CASES if c.cls == "f64 fma"]
    assert {(c.ta, c.tb) for c in fma} == {(0, 0), (1, 0), (0, 1), (1, 1)} and {5, 24} <= {c.k for c in fma} and any(c.k == 16 and c.m % 2 for c in fma)
    span = [c for c in CASES if "span" in c.cls]
    assert {(c.m, c.k, c.batch) for c in span} == {(m, k, b) for m in (40, 104) for k in (72, 147) for b in (3, 11)} and 11 > gb.MAXG
    assert {(c.m, c.n, c.k) for c in CASES if c.cls == "twin big<256>"} == {(136, 250, 2048), (256, 250, 2048)}
    for t in ("128,64", "64,128", "128,128"):
        assert {c.m % 8 for c in CASES if c.cls == f"dma<{t}>"} >= ({0, 4} if t != "128,128" else {0, 4})
    for v in ("vec8", "vec4->1", "vec1"):
        assert {(c.ta, c.tb) for c in CASES if c.cls == f"cfg<128,128,T> {v}"} == {(1, 0), (0, 1), (1, 1)}
    assert {(c.k % 8 == 4, c.m % 8 == 4) for c in CASES if c.cls == "cfg<128,128,T> vec4->1"} == {(True, False), (False, True)}
    for cls in ("f32 atr<0>", "f32 atr<2>"):
        assert any(c.k % 16 and c.m % 64 and c.n % 64 and c.m > 64 and c.n > 64 for c in CASES if c.cls == cls)


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_case_meets_the_conditions_of_its_class(case):
    for cus in CUS:
        got = gb.classes_of(case.entry, case.m, case.n, case.k, case.batch, case.ta, case.tb, cus)
        if case.entry == "f16_ws" and cus != 256:     # the plan's answer depends on the CU count: both outcomes are cases
            assert len(got) == 1 and got[0] in gb.CLASS_NEEDS["f16_ws"], (cus, got)
        else:
            assert got == [case.cls], (cus, got)
    # the call is one the entry point accepts
    assert (not case.ta or case.m >= case.k) and (not case.tb or case.k >= case.n) and case.batch >= 2
    assert case.lname in gb.LAYOUTS and (case.entry == "f64" or not gb.LAYOUTS[case.lname].odd8)


def test_device_sized_shapes_reach_their_class_at_any_cu_count():
    for cus in CUS:
        m, n, batch = gb.f64_big_shape(cus)
        for k in (16, 48):
            assert gb.classes_of("f64", m, n, k, batch, 0, 0, cus) == ["f64 dma<128,128>"]
            assert gb.classes_of("f64", m, n, k, batch - 1, 0, 0, cus) == ["f64 dma<64,64>"]
            assert 8 * (batch * m * n + 3 * m * k + 2 * k * n) < gb.CAP_BYTES * max(1.0, cus / 256.0) and batch <= 65535
        m, n, k, batch = gb.f32_generic_big_shape(cus)
        assert gb.classes_of("f32", m, n, k, batch, 0, 0, cus) == ["f32 generic<128,64>"] and k % 32 and k > 32 and n % 128 and m % 64 and n > 128
        assert gb.classes_of("f32", m, n, k, batch - 3, 0, 0, cus) == ["f32 generic<64,64>"]
        assert 4 * batch * (m * n + 32) < gb.CAP_BYTES * max(1.0, cus / 256.0)
    assert gb.f64_big_shape(256)[2] == 48


def test_every_tile_and_vector_width_of_the_register_staged_kernel_is_reachable():
    """The docstring's statement, by enumeration over sm_gemm_batched_f16 calls with non-transposed operands."""
    seen = set()
    for m in range(8, 300):
        for n in (35, 40, 200, 201):
            for k in (72, 76, 147, 200, 440):
                seen.update(cls for cls in gb.classes_of("f16", m, n, k, 2, 0, 0) if cls.startswith("cfg"))
    assert seen == {f"cfg<{t}> vec{v}" for t in ("128,64", "64,128", "128,128") for v in (8, 4, 1)}
    # vec 8 with m <= 64 only where the span form's LDS bound declines
    for k in range(8, 1024, 8):
        for m in range(8, 65, 8):
            got = gb.classes_of("f16", m, 200, k, 2, 0, 0)
            assert (got == ["cfg<128,64> vec8"]) == (k % 64 != 0 and not gb.span_lds_fits(m, k)), (m, k, got)


def test_stream_k_mirror_agrees_with_the_library_at_256_cus(pkg):
    """Without a device the library's plan is the one for 256 CUs."""
    for rows in (100, 250, 300, 784):
        for cols in (136, 256, 264, 512):
            for k in (128, 1024, 2048, 2304, 4608):
                for problems in (1, 2, 3, 5, 8, 16, 40):
                    takes, plan = pkg.spmma_fused_streamk_plan(rows, cols, k, problems)
                    mine, need = gb.sk_takes(rows, problems, cols, k, 256)
                    assert mine == takes, (rows, cols, k, problems)
                    assert not takes or need == 4096 + plan["slots"] * ((cols + 255) // 256) * 256 * 256 * 4
    # the workspace cases at 256 CUs: every batch below SK_DECLINED is taken, the next ones are not
    for m in (136, 256):
        taken = [b for b in range(1, gb.SK_DECLINED + 8) if gb.sk_takes(250, b, m, 2048, 256)[0]]
        assert taken == list(range(1, gb.SK_DECLINED)), taken
    assert 2 <= gb.SK_BATCH < gb.SK_DECLINED


@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_placement_builder_and_references(case):
    cap = 0
    for kind in gb.KINDS:
        p = gb.problem_of(case, kind)
        d, es = p.d, np.dtype(p.d["u"]).itemsize
        nan_of = lambda a: np.isnan(a.view(d["np"]))
        assert nan_of(np.array([d["qnan"], d["sent"]], dtype=d["u"])).all()
        for pool, idx, vals, fill in ((p.pA, p.iA, p.Av, d["qnan"]), (p.pB, p.iB, p.Bv, d["qnan"]), (p.pC, p.iC, p.C0v, d["sent"])):
            assert np.unique(idx).size == idx.size and idx.min() == 0 and idx.max() + 1 == pool.extent
            lo = [[], []]
            for i in range(pool.nmat):
                if pool is not p.pC or p.reads_c:    # gather is the inverse of scatter
                    assert np.array_equal(pool.gather(i, idx), gb.bits(vals[i]))
                lo[pool.alloc[i]].append((pool.base[i], pool.base[i] + pool.extent))
                # the header's precondition and no more
                byte = pool.base[i] * es
                assert byte % 256 != 0 and byte % 16 == (8 if p.lay.odd8 else 0), (i, byte)
            for a, buf in enumerate(pool.buf):        # guards at both ends, a gap behind every matrix, nothing overlaps
                spans = sorted(lo[a])
                assert not spans or (spans[0][0] * es >= gb.GUARD_BYTES and (buf.size - spans[-1][1]) * es >= gb.GUARD_BYTES)
                assert all(y[0] - x[1] >= 16 // es for x, y in zip(spans, spans[1:]))
                assert (buf[~pool.logical[a]] == fill).all() and pool.logical[a].sum() == len(spans) * idx.size
                if pool is not p.pC or p.reads_c:
                    assert not nan_of(buf[pool.logical[a]]).any()
                else:
                    assert (buf == d["sent"]).all()                  # beta == 0: C holds nothing but the sentinel, a NaN
            assert (not p.lay.second or pool.nmat < 2) == (pool.buf[1].size == 0)
        # the tables: the stated sharing, and no stride describes the entries
        assert len(set(p.bmap)) == (1 if p.lay.sharedB else p.batch)
        assert (p.amap[-1] == p.amap[0]) == p.lay.dupA and len(set(p.amap)) == p.batch - p.lay.dupA
        off = [p.pC.base[e] * es + (1 << 40) * p.pC.alloc[e] for e in range(p.batch)]
        steps = np.diff(off)
        assert steps[0] < 0 or p.pC.alloc[1] == 1, "entry 1 lies in front of entry 0, or in the other allocation"
        if p.batch >= 3:
            assert len(set(steps.tolist())) > 1 and (steps < 0).any() and (steps > 0).any()
        # references
        ref, scale = p.reference()
        assert ref.dtype == d["wide"] and ref.shape == (p.batch, p.n, p.m) and np.isfinite(ref.astype(np.float64)).all()
        assert (scale >= np.abs(ref) * (1 - 1e-12)).all()
        e = p.batch - 1
        Bm = p.Bv[p.bmap[e]].astype(d["wide"])
        Am = p.Av[p.amap[e]].astype(d["wide"])
        one = sum(Bm[p.n - 1, l] * Am[l, 0] for l in range(p.k)) * d["wide"](p.alpha) + (d["wide"](p.beta) * p.C0v[e, p.n - 1, 0].astype(d["wide"]) if p.reads_c else 0)
        assert abs(one - ref[e, p.n - 1, 0]) <= 1e-12 * max(1.0, float(scale[e, p.n - 1, 0]))
        if kind == "ties":
            p.assert_ties_premise()
        cap = max(cap, p.nbytes())
    assert cap < gb.CAP_BYTES


def test_column_major_index_maps():
    """The stored forms the header states: lda = m, ldb = k, ldc = m whatever the flags."""
    m, n, k = 7, 3, 5
    for ta in (0, 1):
        for tb in (0, 1):
            p = gb.Problem("f32", m, n, k, 2, ta, tb, kind="uniform", rng=np.random.default_rng(1))
            for i in range(m):
                for l in range(k):
                    assert p.iA[l, i] == (i * m + l if ta else l * m + i)      # op(A)[i][l]
            for l in range(k):
                for j in range(n):
                    assert p.iB[j, l] == (l * k + j if tb else j * k + l)      # op(B)[l][j]
            assert all(p.iC[j, i] == j * m + i for i in range(m) for j in range(n))


# ---- the refusals, without a device: one dummy non-null address for every pointer array
@pytest.mark.parametrize("name", list(gb.REFUSALS))
def test_refusals_are_decided_before_any_device_call(pkg, name):
    entries, _, _, status = gb.REFUSALS[name]
    for entry in entries:
        L = pkg.lib()
        rc = gb.refusal_status(L, entry, name, 0x100000)
        assert rc == status, f"{name} {entry}: status {rc}: {L.sm_last_error().decode()}"


def test_refusals_cover_what_the_header_states():
    R = gb.REFUSALS
    assert set(R) == {"null tables", "operation 2", "operation -1", "ta = T, m < k", "tb = T, k < n", "f64 batch 65536", "m = 2^31", "n = 2^31", "k = 2^31",
                      "empty m", "empty n", "empty batch"}
    assert all(v[0] == gb.ENTRIES for nme, v in R.items() if nme != "f64 batch 65536") and R["f64 batch 65536"][0] == ("f64",)
    assert R["ta = T, m < k"][1][0] < R["ta = T, m < k"][1][2] and R["tb = T, k < n"][1][2] < R["tb = T, k < n"][1][1]
    assert all(v[3] == 0 for nme, v in R.items() if nme.startswith("empty")) and gb.BIG == 2 ** 31
