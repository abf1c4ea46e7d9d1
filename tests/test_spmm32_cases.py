"""The instruments of tests/test_gpu_spmm32.py, checked without a GPU.  This file restates the dispatch rules of csrc/spmm.hip and of
dispatch32<2> (csrc/gemm_f32.hip) in Python -- the expand / scatter rule, the GEMM's launch class, the vectors per workgroup of both COO forms, the
row split and the packed form's `can` condition -- and holds every case of the GPU file against the class it is named for: every class has a case,
every threshold a case on each side.  On every case the numpy fp64 reference agrees with the oracle (orc.spmm_bell / orc.spmm_coo: a second opinion),
exactly on integers and within one fp32 rounding of the oracle's output on uniform data, and the integer cases' partial sums stay below 2^24.  Every
refusal returns the status include/sparsifyme.h states from a call with dummy non-null pointers: each is decided before any device call."""
import ctypes
import os

import numpy as np
import pytest

import test_gpu_spmm32 as s32   # (as a module: its test functions must not be collected here)

CUS = (64, 104, 256, 304, 512)


# ---------------------------------------------------------------------------------------------
# the rules, restated
# ---------------------------------------------------------------------------------------------
def bell_route(cols, ws_off):
    """launch_bell_expand: a dense row in LDS while cols * 4 bytes <= 48 KiB; its 16-byte stores need cols % 4 == 0 and an aligned row."""
    if cols * 4 > 48 * 1024:
        return "scatter"
    return "expand-vec" if cols % 4 == 0 and ws_off % 16 == 0 else "expand-elem"


def gemm_class(n, rows, cols, batch, b_off, ws_off, cus):
    """dispatch32<2> on (M, N, K) = (n, rows, cols): operand A is the caller's B (lda = cols), operand B the dense workspace (ldb = cols,
    batch stride rows * cols)."""
    M, N, K = n, rows, cols
    a_ok = cols % 4 == 0 and b_off % 4 == 0
    b_ok = cols % 4 == 0 and (rows * cols) % 4 == 0 and ws_off % 16 == 0
    if K % 32 == 0 and K >= 32 and a_ok and b_ok:
        if M <= 64:
            return "dma<64,64>" if N <= 64 else "dma<64,128>"
        return "dma<128,64>" if N <= 128 else "dma<128,128>"
    small_tiles = -(-M // 64) * -(-N // 64) * batch
    return "generic<128,64>" if small_tiles / cus >= 32.0 else "generic<64,64>"


def ws_class(k):
    """launch_csr_and_fallback: as many vectors per workgroup as keep two workgroups on a CU, then what fits 144 KiB; else thread-per-row."""
    cb = 4 * k
    J = 32 if cb * 32 <= 72 * 1024 else 16 if cb * 16 <= 144 * 1024 else 8
    return f"ws J{J}" if cb * J <= 144 * 1024 else "ws row"


def packed_class(m, k, nnz, nv, ws_bytes, ws_off):
    """sm_spmm_coo_f32_packed: J and `can`."""
    rb = 4 * (k + 1)
    J = 32 if rb * 32 <= 80 * 1024 else 16
    can = (ws_bytes >= s32.pk_bytes(m, nnz) and nnz > 0 and ws_off % 16 == 0 and rb * J <= 160 * 1024 and nnz + 32 * (m + 2) <= 2 ** 31 - 1
           and m <= 0x7ffffff0 and -(-nv // J) <= 2 ** 31 - 1)
    return f"packed J{J}" if can else "packed->ws"


def reported_packed_bytes(L, m, nnz):
    need = ctypes.c_size_t(0)
    assert L.sm_spmm_coo_packed_workspace_size(m, nnz, ctypes.byref(need)) == 0
    return need.value


# ---------------------------------------------------------------------------------------------
# Blocked-ELL
# ---------------------------------------------------------------------------------------------
def test_bell_every_class_and_structure_has_a_case():
    named = {(c.route, c.gemm) for c in s32.BELL_CASES if c.route}
    assert {r for r, _ in named} == {"expand-vec", "expand-elem", "scatter"}
    assert {g for _, g in named} == {"dma<64,64>", "dma<64,128>", "dma<128,64>", "dma<128,128>", "generic<64,64>"}   # generic<128,64>: sized on the device
    assert {("scatter", "dma<64,64>"), ("scatter", "generic<64,64>"), ("expand-elem", "generic<64,64>")} <= named
    for cls in ("dma<64,64>", "dma<64,128>", "dma<128,64>", "dma<128,128>"):
        assert {32, 64, 160} <= {c.cols for c in s32.BELL_CASES if c.gemm == cls}
        assert cls in s32.__doc__
    C = s32.BELL_CASES
    assert len({c.name for c in C}) == len(C)
    assert {c.bs for c in C} >= {1, 2, 3, 4, 8} and {c.n for c in C} >= {1, 8, 9} and {c.rows for c in C} >= {255, 256, 257}
    assert set(s32.PATTERNS) == {c.pattern for c in C}
    assert any(c.rows % c.bs for c in C) and any(c.cols % c.bs for c in C) and any(c.cols % 4 and c.cols * 4 <= 48 * 1024 for c in C)
    assert any(c.nblk == 0 and bell_route(c.cols, 0) == "scatter" for c in C) and any(c.nblk == 0 and bell_route(c.cols, 0) != "scatter" for c in C)
    assert {12288, 12320, 12292} <= {c.cols for c in C} and bell_route(12288, 0) == "expand-vec" and bell_route(12289, 0) == "scatter"
    assert all(6 <= c.rows <= 40 for c in C if c.cols > 10000)
    assert any(c.ws_off == 4 for c in C) and any(c.b_off == 1 for c in C)
    # the store branches, under each kernel family: C + one float, odd rows, and the aligned C with rows % 4 == 0
    for fam in ("dma", "generic"):
        mine = [c for c in C if c.gemm and c.gemm.startswith(fam)]
        assert any(c.c_off == 1 for c in mine) and any(c.rows % 4 for c in mine) and any(c.c_off == 0 and c.rows % 4 == 0 for c in mine)
    # every structure case runs through the three entry points
    assert all(c.entries == s32.BELL_ENTRIES for c in s32.BELL_STRUCTURE) and s32.BATCH == 3


@pytest.mark.parametrize("case", [c for c in s32.BELL_CASES if c.route], ids=lambda c: c.name)
def test_bell_case_meets_the_conditions_of_its_class(case):
    assert bell_route(case.cols, case.ws_off) == case.route
    for cus in CUS:
        for batch in (1, s32.BATCH):
            assert gemm_class(case.n, case.rows, case.cols, batch, case.b_off, case.ws_off, cus) == case.gemm
    assert case.ws_off == 0 or "batched" not in case.entries


def test_bell_thresholds_have_a_case_on_each_side():
    by = {c.name: c for c in s32.BELL_CASES}
    pairs = [("n64-rows40", "n68-rows40", "n"), ("n64-rows200", "n68-rows200", "n"), ("rows64-n40", "rows68-n40", "rows"), ("rows128-n72", "rows132-n72", "rows")]
    for lo, hi, ext in pairs:
        a, b = by[lo], by[hi]
        assert a.gemm != b.gemm and a._replace(name="", gemm="", **{ext: getattr(b, ext)}) == b._replace(name="", gemm="")
        assert (getattr(a, ext), getattr(b, ext)) in ((64, 68), (128, 132))
    assert by["cols12288"].cols * 4 == 48 * 1024 and by["cols12320"].cols * 4 > 48 * 1024 and by["cols12320"].cols % 32 == 0 and by["cols12292"].cols % 32


def test_big_generic_shape_reaches_its_class_at_any_cu_count():
    for cus in CUS:
        rows, cols, n, batch = s32.big_generic_shape(cus)
        assert gemm_class(n, rows, cols, batch, 0, 0, cus) == "generic<128,64>" and bell_route(cols, 0) == "expand-vec"
        assert -(-n // 64) * -(-rows // 64) * batch >= 32 * cus and cols == 24 and rows % 64 and batch <= 65535
        assert 4 * batch * rows * (cols + n + cols // 2) < 150e6 * max(1.0, cus / 256.0)      # workspace + C + values


@pytest.mark.parametrize("case", s32.BELL_CASES, ids=lambda c: c.name)
def test_bell_reference_and_oracle_agree(orc, case):
    for kind in s32.KINDS:
        p = s32.BellProblem(case, kind)
        for b in range(p.batch):
            ci, vals = p.ci[b], p.vals[b]
            nbr = -(-case.rows // case.bs)
            assert ci.shape == (nbr, case.nblk) and vals.shape == (case.rows, p.ell_cols)
            live = ci[ci < p.nbc]
            for row in ci:      # a block column at most once per block row
                assert np.unique(row[row < p.nbc]).size == (row < p.nbc).sum()
            if case.pattern == "empties":
                assert (ci == s32.ALL1).any() and (ci == p.nbc).any() and live.size
                assert all({int(ci[br, case.nblk // 2]), int(ci[br, -1])} == {int(s32.ALL1), p.nbc} for br in range(nbr) if br % 5 != 4)
                assert np.isnan(vals).any()
            elif case.nblk:
                assert live.size == ci.size and not np.isnan(vals).any()
                d = np.diff(ci.astype(np.int64), axis=1)
                assert {"asc": (d > 0).all(), "desc": (d < 0).all(), "shuf": (d > 0).any() and (d < 0).any()}[case.pattern]
            for ab in s32.ABS:
                ref, scale = p.reference(b, ab)
                want = p.C0[b].copy()
                orc.spmm_bell(np.ascontiguousarray(vals).reshape(-1), np.ascontiguousarray(ci).reshape(-1), case.rows, case.cols, case.bs, p.ell_cols, p.B, want,
                              case.n, ab[0], ab[1])
                if kind == "ties":
                    s32.assert_ties_premise(ref, scale)
                    assert np.array_equal(want, ref.astype(np.float32))
                else:
                    assert (np.abs(ref - want) <= 2.0 ** -24 * np.abs(want) * (1 + 1e-6) + 1e-13 * scale + 2.0 ** -149).all()
                    assert (scale >= np.abs(ref) - 1e-12).all()
            if case.nblk == 0:
                ref, _ = p.reference(b, s32.ABS[1])
                assert np.array_equal(ref, -2.0 * p.C0[b].astype(np.float64)) and not p.reference(b, s32.ABS[0])[0].any()


def test_guarded_buffers_hold_poison_around_the_payload():
    x = np.arange(10, dtype=np.float32)
    b = s32.Buf(x, s32.QNAN, off=1)
    assert b.base == s32.GUARD + 1 and np.array_equal(b.host[b.base:b.base + 10].view(np.float32), x)
    assert np.isnan(b.host[:b.base].view(np.float32)).all() and np.isnan(b.host[b.base + 10:].view(np.float32)).all() and b.host.size == 10 + 2 * s32.GUARD + 1
    i = s32.Buf(np.arange(5, dtype=np.uint64), s32.ALL1)
    assert (i.host[:s32.GUARD] == s32.ALL1).all() and (i.host[-s32.GUARD:] == s32.ALL1).all() and i.host.dtype == np.uint64
    pay = [np.full(7 + b_, b_, dtype=np.uint32) for b_ in range(3)]
    c = s32.CBuf(pay, off=1, order=[2, 0, 1])
    assert c.start[2] == s32.GUARD + 1 and c.start[2] < c.start[0] < c.start[1]
    gaps = [c.start[0] - (c.start[2] + 9), c.start[1] - (c.start[0] + 7), c.host.size - (c.start[1] + 8)]
    assert min(gaps) >= s32.GUARD and len(set(gaps)) == 3
    assert (c.host[c.outside] == s32.SENT).all() and c.outside.sum() == c.host.size - 24 and all((c.host[s:s + 7 + b_] == b_).all() for b_, s in enumerate(c.start))


# ---------------------------------------------------------------------------------------------
# COO
# ---------------------------------------------------------------------------------------------
def test_coo_rules_at_their_thresholds():
    assert [ws_class(k) for k in (576, 577, 2304, 2305, 4608, 4609)] == ["ws J32", "ws J16", "ws J16", "ws J8", "ws J8", "ws row"]
    big = 1 << 40
    assert [packed_class(50, k, 100, 5, big, 0) for k in (639, 640, 2559, 2560)] == ["packed J32", "packed J16", "packed J16", "packed->ws"]
    assert [s32.row_split(m, 1) for m in (511, 512, 520, 1025, 1030)] == [1, 2, 2, 4, 4]


def test_coo_every_class_has_cases_on_both_sides_of_its_thresholds():
    C = s32.COO_CASES
    assert len({c.name for c in C}) == len(C) and {c.cls for c in C} == set(s32.COO_CLASSES)
    for cls in s32.COO_CLASSES:
        assert cls in s32.__doc__ or cls.split()[0] in s32.__doc__
        mine = [c for c in C if c.cls == cls]
        ks = {c.k for c in mine}
        assert set(s32.THRESHOLD_COLS[cls]) <= ks
        J = s32.GROUP[cls]
        nvs = {(c.n if cls == "ws row" else c.n * c.batches) for c in mine}
        assert {1, 5, J - 1, J, J + 1} <= nvs and {c.batches for c in mine} >= {1, 3}
        assert {"sorted", "colshuf", "shuffled", "dups"} <= {c.order for c in mine} and "col" in {c.oob for c in mine}
    allk = {(s32.entry_of(c.cls), c.k) for c in C}
    assert {("ws", k) for k in (576, 577, 2304, 2305, 4608, 4609)} | {("packed", k) for k in (639, 640, 2559, 2560)} <= allk
    for entry in ("ws", "packed"):
        mine = [c for c in C if s32.entry_of(c.cls) == entry]
        assert {"rowhi", "rowneg"} <= {c.oob for c in mine}
        assert {511, 512, 520, 1030} <= {c.m for c in mine if c.matrix == "split"}
    assert any(c.m == 1025 and c.cls == "packed J32" for c in C)
    assert set(s32.PACKED_ROUTING) == {"nnz0", "one-byte-short", "below-rowptr", "unaligned"}


@pytest.mark.parametrize("case", s32.COO_CASES, ids=lambda c: c.name)
def test_coo_case_meets_the_conditions_of_its_class(pkg, case):
    entry = s32.entry_of(case.cls)
    p = s32.CooProblem(case, "ties")
    nv = case.n * case.batches
    if entry == "ws":
        assert ws_class(case.k) == case.cls
    else:
        assert packed_class(case.m, case.k, p.nnz, nv, reported_packed_bytes(pkg.lib(), case.m, p.nnz), 0) == case.cls
        if case.cls == "packed->ws":
            assert ws_class(case.k) == "ws J8"
    assert entry in ("ws", "packed") and p.nnz > 0
    r = p.r.astype(np.int64)
    rows_sorted = bool((np.diff(r) >= 0).all())
    in_range = bool(((r >= 0) & (r < case.m)).all())
    assert s32.expected_flag(case) == (1 if not (rows_sorted and in_range) else 4 if case.cls in ("packed J32", "packed J16") else 0)
    assert rows_sorted == (case.order != "shuffled") and in_range == (case.oob not in ("rowhi", "rowneg"))
    ok = p.valid()
    assert (~ok).sum() == {None: 0, "col": 6, "rowhi": 1, "rowneg": 1}[case.oob]
    c = p.c.astype(np.int64)
    same_row = np.diff(r) == 0
    if case.order == "sorted" and case.oob is None:
        assert (np.diff(c)[same_row] > 0).all()
    if case.order in ("colshuf", "dups"):
        assert (np.diff(c)[same_row] < 0).any()
    key = r[ok] * case.k + c[ok]
    assert (np.unique(key).size < key.size) == (case.order == "dups")
    lens = np.bincount(r[(r >= 0) & (r < case.m)], minlength=case.m)
    if case.matrix == "lens":
        R = s32.ROUND_ENTRIES[case.cls]
        # the entries per round: 256 / J of the LDS-CSR kernel (packed->ws is served by its J = 8 form), the 32-entry pad unit of the packed one
        assert R == {"ws J32": 32, "ws J16": 64, "ws J8": 128, "ws row": 32, "packed J32": 32, "packed J16": 32, "packed->ws": 128}[case.cls]
        assert 37 <= case.m <= 70 and case.m % 8 != 0
        if case.order != "dups" and case.oob in (None, "col"):
            assert {0, 1, R - 1, R, R + 1, 2 * R + 3} <= set(lens.tolist()) and lens[0] == 0 and lens[-1] == 0
            assert any((lens[i:i + 3] == 0).all() for i in range(1, case.m - 3))
    else:
        s = s32.row_split(case.m, -(-nv // s32.GROUP[case.cls]))
        assert s == {511: 1, 512: 2, 520: 2, 1025: 4, 1030: 4}[case.m] and nv <= 6
        per = -(-case.m // s)
        assert all(lens[min((y + 1) * per, case.m) - 1] > 0 for y in range(s)) and (lens[100:110] == 0).all()
    if case.m == 1025:      # pk_scan_kernel: runs of two rows, most of the 1024 threads without one
        assert (case.m + 1023) // 1024 == 2


@pytest.mark.parametrize("case", s32.COO_CASES + [s32.ROUTING_CASE], ids=lambda c: c.name)
def test_coo_reference_and_oracle_agree(orc, case):
    for kind in s32.KINDS:
        p = s32.CooProblem(case, kind)
        ok = p.valid()          # the oracle refuses a coordinate out of range: it gets the entries the definition keeps
        r, c, v = (np.ascontiguousarray(a[ok]) for a in (p.r, p.c, p.v))
        for ab in s32.ABS:
            ref, scale = p.reference(ab)
            want = p.C0.copy()
            orc.spmm_coo(case.m, case.k, r.size, case.n, case.batches, r, c, v, p.B, want, ab[0], ab[1])
            if kind == "ties":
                s32.assert_ties_premise(ref, scale)
                assert np.array_equal(want, ref.astype(np.float32))
            else:
                assert (np.abs(ref - want) <= 2.0 ** -24 * np.abs(want) * (1 + 1e-6) + 1e-13 * scale + 2.0 ** -149).all()
        assert p.terms() == int(np.bincount(r, minlength=case.m).max())


def test_packed_workspace_size_and_routing_cases(pkg):
    L = pkg.lib()
    for m, nnz in ((1, 0), (37, 100), (53, 1234), (1030, 7001), (70, 0)):
        assert reported_packed_bytes(L, m, nnz) == (s32.pk_bytes(m, nnz) + 255) // 256 * 256
    case = s32.ROUTING_CASE
    small = ctypes.c_size_t(0)
    assert L.sm_spmm_coo_workspace_size(case.m, ctypes.byref(small)) == 0 and small.value == 4 * (case.m + 2)
    for mode in s32.PACKED_ROUTING:
        p, ws_bytes, ws_off, flag, untouched = s32.routing_setup(mode, "ties")
        nbytes = reported_packed_bytes(L, case.m, p.nnz) if ws_bytes is None else ws_bytes
        assert packed_class(case.m, case.k, p.nnz, p.nv, nbytes, ws_off) == "packed->ws" and ws_class(case.k) == "ws J32"
        assert packed_class(case.m, case.k, max(p.nnz, 1), p.nv, reported_packed_bytes(L, case.m, p.nnz), 0) == "packed J32"   # but for the one condition
        assert untouched == (nbytes < small.value) and (flag is None) == untouched
        assert (p.nnz == 0) == (mode == "nnz0")
        if mode == "one-byte-short":
            assert small.value <= nbytes == s32.pk_bytes(case.m, p.nnz) - 1
        lens = np.bincount(p.r, minlength=case.m)
        assert (lens == 0).any()


# ---------------------------------------------------------------------------------------------
# refusals, without a device: dummy non-null pointers
# ---------------------------------------------------------------------------------------------
BASE = 0x100000


@pytest.mark.parametrize("name", list(s32.REFUSALS))
def test_refusals_are_decided_before_any_device_call(pkg, name):
    fam, entries, over, status = s32.REFUSALS[name]
    L = pkg.lib()
    for entry in entries:
        I = BASE * 2 if fam == "bell" else (BASE * 2, BASE * 6)
        rc = s32.call_refusal(L, name, BASE, I, BASE * 3, BASE * 4, BASE * 5, entry)
        assert rc == status, f"{name} {entry}: status {rc}: {L.sm_last_error().decode()}"


def test_refusals_cover_what_the_header_states():
    R = s32.REFUSALS
    assert {n for n, v in R.items() if v[3] == s32.INVALID} == {n for n in R if "null" in n or "block_size" in n or "without a workspace" in n}
    assert all(v[3] in (s32.INVALID, s32.NOT_SUPPORTED) for v in R.values())
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsifyme.h")).read()
    text = " ".join(hdr.split())
    for phrase in ("sm_spmm_bell_f32, sm_spmm_bell_f32_ws and sm_spmm_bell_batched_f32 return SM_STATUS_INVALID_VALUE for a null pointer",
                   "n > 8 * 65535", "B_num_cols * num_batches > 65535", "A_nnz exceeds 2^31-1"):
        assert phrase in text, phrase
