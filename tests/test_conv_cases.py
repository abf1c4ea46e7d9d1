"""The instruments of tests/test_gpu_conv.py, checked without a GPU.  This file restates the dispatch rule of csrc/conv_spmma.hip in Python --
conv_geometry_plan and the class choice of conv_fused_rule -- and holds it against sm_conv_spmma_fused_plan field for field on every case and on a
sweep; holds every case of the GPU file against the class it is named for (every class has a case, every threshold a case on each side); models
the activation patch from the plan numbers the LIBRARY returns, as the kernel's comments define it, and gathers every (tile, stage, pixel, k)
through it: inside patch_bytes, table entries below 65536, the value orc.im2col has there -- a wrong RI / padl / patch_bytes shows here; checks the
promise of sm_conv_spmma_workspace; records which refusals a sweep can reach; and holds the numpy fp64 reference against the oracle chain
(orc.im2col + orc.compress24 + orc.spmma: a second opinion), exactly on integers and within one output rounding on uniform data."""
import ctypes
import itertools

import numpy as np
import pytest

import test_gpu_conv as cv   # (as a module: its test functions must not be collected here)

FIELDS = ("bn", "RI", "pitch", "padl", "rpi", "nch", "a_n", "patch_bytes", "lds", "tiles_m", "tiles_n")
GEO_MAX = 1 << 20


# ---------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------
def geometry_plan(N, Cin, H, W, kh, kw, stride, pad, dil, v16, bn):
    """conv_geometry_plan: (why it does not fit or None, the plan numbers as far as they were computed)."""
    a = dict.fromkeys(FIELDS[1:8], 0)
    if kh == 0 or kw == 0 or stride == 0 or dil == 0:
        return "invalid", a
    if N > 0x7fffffff or Cin > 0x7fffffff or max(H, W, kh, kw, stride, pad, dil) > GEO_MAX:
        return "32-bit", a
    sh, sw = dil * (kh - 1) + 1, dil * (kw - 1) + 1
    if H + 2 * pad < sh or W + 2 * pad < sw:
        return "window", a
    OH, OW = (H + 2 * pad - sh) // stride + 1, (W + 2 * pad - sw) // stride + 1
    L, K = OH * OW, Cin * kh * kw
    if v16 and W % 8:
        return "w%8", a
    epl = 8 if v16 else 2                                   # halves per lane of a patch DMA
    padl = max(pad, max(sw - 1 - pad, 0))
    padl = -(-padl // epl) * epl or epl
    pitch = padl + W
    if K == 0 or K % 64 or W % 2 or pitch // epl > 64 or kh * kw > 64 or H > 0x7fff or N * L > 0x7fffffff or K > 0x7fffffff:
        return "shape", a
    span = (L - 1) // OW if L < 128 else (127 + OW - 1) // OW
    a["RI"] = span * stride + sh
    a["pitch"], a["padl"] = pitch, padl
    a["rpi"] = 64 // (pitch // epl)
    a["nch"] = (kh * kw - 1 + 63) // (kh * kw) + 1
    a["a_n"] = -(-a["nch"] * a["RI"] // a["rpi"])
    a["patch_bytes"] = -(-((a["nch"] * a["RI"] * pitch + padl + 2 * (sw + pad)) * 2 + 256) // 16) * 16
    if a["a_n"] > (16 if v16 else 48):
        return "dma", a
    if (a["nch"] * a["RI"] * pitch + kw * dil) * 2 >= 65536:
        return "table", a
    if 2 * (a["patch_bytes"] + 64 * bn * 2) + kh * kw * 128 > 160 * 1024:
        return "lds", a
    return None, a


def fused_rule(geom, x_align=16, b_aligned=True):
    """conv_fused_rule: (form, plan, why) as sm_conv_spmma_fused_plan answers; why "invalid" / "window": the query's status is INVALID_VALUE."""
    N, Cin, H, W, kh, kw, stride, pad, dil, n_out = geom
    plan = dict.fromkeys(FIELDS, 0)
    if kh == 0 or kw == 0 or stride == 0 or dil == 0:
        return "not_taken", plan, "invalid"
    if max(H, W, pad, kh, kw, dil) <= GEO_MAX and (H + 2 * pad < dil * (kh - 1) + 1 or W + 2 * pad < dil * (kw - 1) + 1):
        return "not_taken", plan, "window"
    if N == 0 or Cin == 0 or n_out == 0:
        return "empty", plan, None
    if n_out % 8 or n_out > 0x7fffffff or not b_aligned or x_align % 4:
        return "not_taken", plan, "operands"
    bn = 64 if n_out <= 64 else 128
    plan["bn"] = bn
    v16 = W % 8 == 0 and x_align % 16 == 0
    why, a = geometry_plan(*geom[:9], True, bn) if v16 else ("", None)
    if why is not None:
        v16 = False
        why, a = geometry_plan(*geom[:9], False, bn)
    plan.update(a)
    if why is not None:
        return "not_taken", plan, why
    L = cv.dims(geom)[2]
    tiles_m, tiles_n = (L + 127) // 128, -(-n_out // bn)
    if tiles_m * tiles_n * N > 0x7fffffff:
        return "not_taken", plan, "grid"
    lds = max(2 * (a["patch_bytes"] + 64 * bn * 2) + kh * kw * 128, 128 * (bn * 2 + 16))
    if lds > 160 * 1024:
        return "not_taken", plan, "lds"
    plan.update(lds=lds, tiles_m=tiles_m, tiles_n=tiles_n)
    return ("v16" if v16 else "small4" if a["a_n"] <= 16 else "large4"), plan, None


REASON_WORDS = {"operands": "needs n % 8 == 0", "32-bit": "32-bit indexing", "shape": "needs C*kh*kw % 64 == 0", "dma": "too many DMA instructions",
                "table": "16-bit offset table", "lds": "does not fit LDS", "grid": "grid too large"}


def library_answer(pkg, geom, x_align=16, b_aligned=True):
    """(form, plan, why) from sm_conv_spmma_fused_plan; why from the words it leaves in sm_last_error()."""
    try:
        form, plan = pkg.conv_spmma_fused_plan(*geom, x_align=x_align, b_aligned=b_aligned)
    except pkg.SparsifymeError as e:
        assert "status 1" in str(e)
        return "not_taken", dict.fromkeys(FIELDS, 0), "window" if "window larger" in str(e) else "invalid"
    why = None
    if form == "not_taken":
        text = pkg.lib().sm_last_error().decode()
        hits = [k for k, w in REASON_WORDS.items() if w in text]
        assert len(hits) == 1 and text.startswith("sm_conv_spmma_fused"), text
        why = hits[0]
    return form, plan, why


def window_combos():
    """(kh, kw, stride, pad, dil) of the cases."""
    return sorted({c.geom[4:9] for c in cv.CONV_CASES})


def sweep(ws=range(2, 131, 2), hs=(4, 9, 16, 30, 57), cins=(1, 3, 4, 16, 48, 64)):
    for (kh, kw, s, p, d), Cin, H, W in itertools.product(window_combos(), cins, hs, ws):
        yield (1 + (H + W) % 3, Cin, H, W, kh, kw, s, p, d, 64 if W % 4 else 136)


FLAG_SETTINGS = ((16, True), (4, True), (2, True))      # X 16-byte aligned, 4-byte aligned only, neither; B aligned


# ---------------------------------------------------------------------------------------------
# the restatement against the library
# ---------------------------------------------------------------------------------------------
def test_restated_rule_equals_the_library_on_every_case_and_a_sweep(pkg):
    geoms = [c.geom for c in cv.CONV_CASES] + [g for _, (g, _, _, _) in cv.REFUSALS.items()]
    geoms += [(0,) + cv._GOOD[1:], cv._GOOD[:1] + (0,) + cv._GOOD[2:], cv._GOOD[:9] + (0,)]
    reached, forms, n = set(), set(), 0
    for geom in itertools.chain(geoms, sweep()):
        for xa, b_ok in FLAG_SETTINGS + ((16, False),):
            mine, lib = fused_rule(geom, xa, b_ok), library_answer(pkg, geom, xa, b_ok)
            assert mine == lib, f"{geom} X % {xa}, B aligned {b_ok}: restated {mine}, library {lib}"
            reached.add(lib[2])
            forms.add((lib[0], lib[1]["bn"]))
            n += 1
    assert n > 100000
    assert forms >= {(f, bn) for f in ("v16", "small4", "large4") for bn in (64, 128)} | {("empty", 0), ("not_taken", 0), ("not_taken", 64)}
    # the refusals a sweep of ordinary layers reaches.  "table" and "lds" are guards no geometry reaches: pitch / epl <= 64 bounds a row at 128
    # (4-byte) or 512 (16-byte) halves, rpi * pitch <= 64 * epl and a_n <= 48 / 16 bound nch * RI * pitch at 6144 / 8192 halves, and the border
    # padl >= (sw - 1) / 2 bounds kw * dil by about 2 * pitch: the largest offset stays below 2 * (8192 + 1024) < 65536 bytes and the LDS below
    # 2 * (24 KiB + 16 KiB) + 8 KiB.  (Pushing kw * dil up does not get there: the border it needs breaks the pitch limit first.)
    assert reached == {None, "invalid", "window", "operands", "shape", "dma"}
    for geom in ((1, 64, 8, 64, 1, 2, 1, 20000, 40000, 64), (1, 32, 4, 100, 1, 2, 1, 200, 400, 64)):
        assert library_answer(pkg, geom, 16)[2] == "shape" == fused_rule(geom)[2]
    assert library_answer(pkg, (1, 64, 8, 8, 3, 3, 1, 1, GEO_MAX + 1, 64))[2] == "32-bit" == fused_rule((1, 64, 8, 8, 3, 3, 1, 1, GEO_MAX + 1, 64))[2]


def test_plan_query_rejects_bad_arguments(pkg):
    L = pkg.lib()
    form, buf = ctypes.c_int(-1), (ctypes.c_uint * 11)()
    assert L.sm_conv_spmma_fused_plan(*cv._GOOD, 7, None, buf) == cv.INVALID
    assert L.sm_conv_spmma_fused_plan(*cv._GOOD, 8, ctypes.byref(form), buf) == cv.INVALID and form.value == -1      # an unknown flag
    assert L.sm_conv_spmma_fused_plan(*cv._GOOD, 7, ctypes.byref(form), None) == 0 and form.value == 2                # plan may be NULL
    assert L.sm_conv_spmma_fused_plan(*cv._GOOD, 5, ctypes.byref(form), buf) == 0 and form.value == 2 and buf[0] == 64  # X 16-byte aligned implies 4
    assert L.sm_conv_spmma_fused_plan(*cv._GOOD, 6, ctypes.byref(form), buf) == 0 and form.value == 3
    assert pkg.CONV_FORMS[2:4] == ("v16", "small4") and len(pkg.CONV_PLAN_FIELDS) == 11 and tuple(pkg.CONV_PLAN_FIELDS) == FIELDS


# ---------------------------------------------------------------------------------------------
# the case list
# ---------------------------------------------------------------------------------------------
def test_every_class_and_threshold_has_a_case(pkg):
    C = cv.CONV_CASES
    assert len({c.name for c in C}) == len(C) and cv.TYPES == ("f16", "bf16")      # (every case runs in both types)
    assert {c.cls for c in C} == set(cv.CLASSES) | {cv.DECLINED}
    for cls in cv.CLASSES:
        assert cls.split("-")[0] in cv.__doc__
    plan = {c.name: library_answer(pkg, c.geom, cv.x_align(c)) for c in C}
    for lo, hi, field, values in cv.THRESHOLDS:
        a, b = cv.BY_NAME[lo], cv.BY_NAME[hi]
        assert a.cls != b.cls, (lo, hi)
        if field:
            assert (plan[lo][1][field], plan[hi][1][field]) == values
    # partial column tiles: under each 64-column kernel an n_out in {8, 24, 56}, under each 128-column one an n_out in {72, 136, 200}
    for fam in ("V16", "SMALL", "LARGE"):
        assert any(c.cls == fam + "-64" and c.geom[9] in (8, 24, 56) for c in C) and any(c.cls == fam + "-128" and c.geom[9] in (72, 136, 200) for c in C)
        assert any(cv.BY_NAME[n].cls.startswith(fam) and cv.BY_NAME[n].geom[9] % 64 for n in cv.SPECIAL_CASES)
    assert {c.geom[9] for c in C} >= {8, 24, 56, 72, 136, 200}
    # the 16-byte form's own limit: 16 instructions taken, 17 handed to the 4-byte form
    assert geometry_plan(*cv.BY_NAME["v16-a_n16"].geom[:9], True, 128)[1]["a_n"] == 16
    why, a = geometry_plan(*cv.BY_NAME["v16-a_n17"].geom[:9], True, 64)
    assert (why, a["a_n"]) == ("dma", 17) and plan["v16-a_n17"][0] == "large4"
    # pitch / halves per lane: 64 taken, 65 not (W = 128 is for the 16-byte form alone)
    assert plan["w126"][1]["pitch"] // 2 == 64 and plan["w128+x4"][2] == "shape" and plan["w128"][0] == "v16"
    assert geometry_plan(*cv.BY_NAME["w128"].geom[:9], False, 64)[0] == "shape"
    assert plan["w120"][1]["pitch"] // 8 == 16 and plan["w122"][0] == "large4"
    # kh * kw: 64 taken, 65 not
    khkw = lambda n: cv.BY_NAME[n].geom[4] * cv.BY_NAME[n].geom[5]
    assert (khkw("cin1-8x8"), khkw("khkw65")) == (64, 65) and plan["khkw65"][2] == "shape" and 64 * 5 * 13 % 64 == 0
    # channel counts that are no multiple of 64; a stage that can touch more channels than exist
    assert {c.geom[1] for c in C} >= {1, 3, 4, 12, 16, 48} and plan["cin16-2x2"][1]["nch"] == 17 > 16
    # the windows, L at the tile edge, a tile that straddles 65 output rows
    assert {cv.dims(cv.BY_NAME[n].geom)[2] for n in ("L126", "L128", "L140")} == {126, 128, 140}
    assert cv.BY_NAME["L140-n3"].geom[0] == 3 and cv.dims(cv.BY_NAME["L140-n3"].geom)[2] % 128
    assert cv.dims(cv.BY_NAME["ow2"].geom)[1] == 2 and plan["ow2"][1]["RI"] == 67
    assert any(c.x_off == 2 and c.cls != cv.DECLINED for c in C) and sum(c.cls == cv.DECLINED for c in C) >= 5
    # small enough to stay quick: the largest im2col operand
    assert max(c.geom[0] * cv.dims(c.geom)[2] * cv.dims(c.geom)[3] for c in C) <= 3136 * 576


@pytest.mark.parametrize("case", cv.CONV_CASES, ids=lambda c: c.name)
def test_case_is_named_for_its_class(pkg, case):
    form, plan, why = library_answer(pkg, case.geom, cv.x_align(case))
    assert cv.class_of(form, plan) == case.cls and (why is not None) == (case.cls == cv.DECLINED)
    assert fused_rule(case.geom, cv.x_align(case)) == (form, plan, why)
    for k, v in (case.pins or {}).items():
        assert plan[k] == v, f"{case.name}: {k} = {plan[k]}, the case is there for {v}"
    assert 4.5 * cv.dims(case.geom)[3] + 6 < 2 ** 24 and case.x_off in (0, 2)
    if case.cls == cv.DECLINED:
        # the routed entry needs a workspace here, and the entry point leaves the query's words (under its own name) with status 2
        L = pkg.lib()
        assert pkg.conv_spmma_workspace(*case.geom[:9]) == pkg.compress24_size(*cv.dims(case.geom)[2:], 2, case.geom[0]) > 0
        said = L.sm_last_error().decode()
        for t in cv.TYPES:
            assert cv.call_fused(L, t, BASE + 2 * case.x_off, BASE * 2, BASE * 3, case.geom) == cv.NOT_SUPPORTED
            assert L.sm_last_error().decode() == said.replace("sm_conv_spmma_fused_plan", "sm_conv_spmma_fused_" + t)


# ---------------------------------------------------------------------------------------------
# plan sufficiency: the patch modelled from the library's numbers
# ---------------------------------------------------------------------------------------------
def check_plan_gathers_im2col(orc, geom, form, plan):
    N, Cin, H, W, kh, kw, s, p, d, n_out = geom
    OH, OW, L, K = cv.dims(geom)
    RI, pitch, padl, rpi, nch, a_n, patch_bytes = (plan[k] for k in FIELDS[1:8])
    epl = 8 if form == "v16" else 2
    khkw = kh * kw
    # the DMA plan: rpi rows of pitch / epl lanes per instruction, a_n instructions cover the nch * RI rows, 4 waves x 4 (12) slots hold them
    assert pitch == padl + W and pitch % epl == 0 and padl % epl == 0 and W % epl == 0 and rpi * (pitch // epl) <= 64 and rpi >= 1
    assert a_n * rpi >= nch * RI and a_n <= (48 if form == "large4" else 16) and patch_bytes % 16 == 0 and nch * RI * pitch * 2 <= patch_bytes
    X = (np.arange(Cin * H * W, dtype=np.int64) % 65535 + 1).astype(np.uint16)      # no zero inside the image
    A = orc.im2col(X, 1, Cin, H, W, kh, kw, s, p, d).reshape(L, K)
    Ximg = X.reshape(Cin, H, W)
    kk = np.arange(64)
    for tile in range((L + 127) // 128):
        m0 = tile * 128
        oh_first = m0 // OW
        ih_lo = oh_first * s - p                                   # patch row 0 is this input row
        px = np.minimum(m0 + np.arange(128), L - 1)
        oh, ow = px // OW, px % OW
        poff = (((oh - oh_first) * s) * pitch + ow * s + padl - p) * 2
        rows = ih_lo + np.arange(RI)
        live = (rows >= 0) & (rows < H)
        for kt in range(K // 64):
            cbase = 64 * kt // khkw
            # layout [channel][input row][padl + W], borders zero: a row's right border is the next row's left border
            patch = np.zeros(patch_bytes // 2, dtype=np.uint16)
            body = patch[:nch * RI * pitch].reshape(nch, RI, pitch)
            ch = min(nch, Cin - cbase)                             # the channel bound cbase + a_ch < Cin
            body[:ch, live, padl:] = Ximg[cbase:cbase + ch, rows[live], :]
            q = 64 * kt % khkw + kk
            c, rem = q // khkw, q % khkw
            table = ((c * RI + (rem // kw) * d) * pitch + (rem % kw) * d) * 2
            assert table.max() < 65536
            addr = poff[:, None] + table[None, :]
            assert addr.min() >= 0 and addr.max() + 2 <= patch_bytes, f"{geom} tile {tile} stage {kt}: a gather at {addr.min()} .. {addr.max()} of {patch_bytes}"
            got = patch[addr // 2]
            want = A[px, 64 * kt:64 * kt + 64]
            assert np.array_equal(got, want), f"{geom} tile {tile} stage {kt}: the modelled patch gathers {int((got != want).sum())} wrong values"


@pytest.mark.parametrize("case", [c for c in cv.CONV_CASES if c.cls != cv.DECLINED], ids=lambda c: c.name)
def test_plan_gathers_the_im2col_operand_on_the_cases(pkg, orc, case):
    form, plan, _ = library_answer(pkg, case.geom, cv.x_align(case))
    check_plan_gathers_im2col(orc, case.geom, form, plan)


# (case, what is taken off its plan): RI and padl are the rule's upper bounds -- a tile rarely straddles the most rows the formula allows for, the
# right border never needs more than `pad` -- so each is cut where the case needs all of it
OFF_BY_ONE = [("cin16-2x2", "RI"), ("1x1-small64", "RI"), ("v16-a_n16", "RI"), ("small128-n72", "padl"), ("L128", "padl"), ("v16-a_n16", "padl"),
              ("dil3-nopad", "patch_bytes"), ("ow2", "patch_bytes"), ("v16-a_n16", "patch_bytes")]


@pytest.mark.parametrize("name,field", OFF_BY_ONE)
def test_the_patch_model_notices_a_plan_that_is_off_by_one(pkg, orc, name, field):
    """The instrument itself: one row less per channel, a border one lane's piece narrower, a patch buffer one 16-byte piece short of its rows."""
    case = cv.BY_NAME[name]
    form, plan, _ = library_answer(pkg, case.geom, cv.x_align(case))
    check_plan_gathers_im2col(orc, case.geom, form, plan)
    epl = 8 if form == "v16" else 2
    wrong = {"RI": dict(RI=plan["RI"] - 1), "padl": dict(padl=plan["padl"] - epl, pitch=plan["pitch"] - epl),
             "patch_bytes": dict(patch_bytes=plan["nch"] * plan["RI"] * plan["pitch"] * 2 // 16 * 16 - 16)}[field]
    with pytest.raises(AssertionError):
        check_plan_gathers_im2col(orc, case.geom, form, dict(plan, **wrong))


def test_plan_gathers_the_im2col_operand_on_a_sweep(pkg, orc):
    n = 0
    for (kh, kw, s, p, d), H, W in itertools.product(window_combos(), (5, 20), range(2, 131, 10)):
        Cin = next(c for c in (1, 4, 16, 64) if c * kh * kw % 64 == 0)
        geom = (1, Cin, H, W, kh, kw, s, p, d, 64)
        for xa in (16, 4):
            form, plan, why = library_answer(pkg, geom, xa)
            if form in ("v16", "small4", "large4") and (xa == 16 or W % 8 == 0):
                check_plan_gathers_im2col(orc, geom, form, plan)
                n += 1
    assert n > 150


# ---------------------------------------------------------------------------------------------
# the workspace promise
# ---------------------------------------------------------------------------------------------
def test_workspace_zero_means_the_implicit_kernel_takes_any_4_byte_aligned_x(pkg):
    zero = sized = 0
    for geom in itertools.chain((c.geom for c in cv.CONV_CASES), sweep(ws=range(2, 131, 4), hs=(4, 16, 57))):
        try:
            need = pkg.conv_spmma_workspace(*geom[:9])
        except pkg.SparsifymeError:
            assert fused_rule(geom)[2] in ("window", "invalid")
            continue
        if need == 0:
            form, _, why = library_answer(pkg, geom[:9] + (128,), 4)
            assert form in ("small4", "large4"), f"{geom}: no workspace asked for, but a 4-byte aligned X is declined ({why})"
            zero += 1
        else:
            OH, OW, L, K = cv.dims(geom)
            assert need == pkg.compress24_size(L, K, 2, geom[0])
            assert (L <= 256 and K >= 2048) or library_answer(pkg, geom[:9] + (128,), 4)[0] == "not_taken"
            sized += 1
    assert zero > 1000 and sized > 1000


# ---------------------------------------------------------------------------------------------
# the reference against the oracle chain
# ---------------------------------------------------------------------------------------------
HALF_ULP = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}


@pytest.mark.parametrize("case", cv.CONV_CASES, ids=lambda c: c.name)
def test_reference_and_oracle_agree(orc, case):
    N, Cin, H, W, kh, kw, s, p, d, n_out = case.geom
    for t, kind in itertools.product(cv.TYPES, cv.KINDS):
        pr = cv.Problem(case, kind, t)
        A = orc.im2col(pr.X, N, Cin, H, W, kh, kw, s, p, d)
        assert np.array_equal(A, pr.A_bits.reshape(-1)), f"{case.name}: the window read by index arithmetic is not orc.im2col"
        blob = orc.compress24(A, pr.L, pr.K, pr.K, N)
        for ab in (cv.ABS if kind == "ties" else cv.ABS[1:]):
            ref, scale = pr.reference(ab)
            want = pr.C0.copy()
            orc.spmma(blob, pr.B, want, pr.L, n_out, pr.K, N, 0, None, ab[0], ab[1], bf16=(t == "bf16"))
            if kind == "ties":
                cv.assert_ties_premise(pr, ref, scale)
                assert np.array_equal(cv.canon(want), cv.canon(cv.round_once(ref, t))), f"{case.name} {t} {ab}"
            else:
                w = cv.bits_to_f64(want, t)
                assert (np.abs(ref - w) <= HALF_ULP[t] * np.abs(w) * (1 + 1e-3) + 1e-13 * scale + 2.0 ** -25).all(), f"{case.name} {t} {ab}"
                assert (scale >= np.abs(ref) - 1e-12).all()


def test_ties_data_is_the_same_in_both_types_and_exact():
    case = cv.BY_NAME["small128-n72"]
    a, b = cv.Problem(case, "ties", "f16"), cv.Problem(case, "ties", "bf16")
    for x, y in ((a.X, b.X), (a.B, b.B), (a.C0, b.C0)):
        assert np.array_equal(cv.bits_to_f64(x, "f16"), cv.bits_to_f64(y, "bf16")) and set(np.unique(cv.bits_to_f64(x, "f16"))) == set(range(-3, 4))
    # the strip rule: ties keep the lower k; the two largest magnitudes otherwise
    keep = cv.strip_keep(np.array([[1.0, -1.0, 1.0, 1.0, 0.0, 3.0, -2.0, 2.0, 0.0, 0.0, 0.0, 0.0, -1.0, 2.0, -3.0, 2.0]]))
    assert keep.astype(int).tolist() == [[1, 1, 0, 0, 0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1, 0]]
    # the conversions: round to nearest even, once
    assert cv.f32_to_bits(np.array([1.0, 1.00390625, 1.01171875, -2.0], dtype=np.float32), "bf16").tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC000]
    assert cv.round_once(np.array([2049.0, 2051.0, -0.0, 65520.0]), "f16").tolist() == [0x6800, 0x6802, 0x8000, 0x7C00]
    assert cv.canon(np.array([0x8000, 0x8001, 0], dtype=np.uint16)).tolist() == [0, 0x8001, 0]


@pytest.mark.parametrize("name", cv.SPECIAL_CASES)
def test_special_values_reach_every_kind_of_result(name):
    for t in cv.TYPES:
        pr = cv.Problem(cv.BY_NAME[name], "special", t)
        inf, big, sub = (0x7C00, 0x7BFF, 0x03FF) if t == "f16" else (0x7F80, 0x7F7F, 0x007F)
        mag = pr.X & 0x7FFF
        assert {0x0000, 0x8000, inf, 0x8000 | inf} <= set(pr.X.tolist()) and (mag == big).sum() >= pr.N and ((mag > 0) & (mag <= sub)).any()
        assert not cv.is_nan16(pr.X, t).any() and not cv.is_nan16(pr.B, t).any() and (np.abs(cv.bits_to_f64(pr.B, t)[np.isfinite(cv.bits_to_f64(pr.B, t))]) <= 1).all()
        ref = pr.reference_over_kept_terms()
        assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).any()
        # no window holds the largest finite value twice: no fp32 partial sum overflows where the fp64 sum is finite
        assert ((pr.A_bits & 0x7FFF) == big).sum(axis=1).max() <= 1


def test_guarded_buffers_hold_poison_around_the_payload():
    x = np.arange(10, dtype=np.uint16)
    b = cv.Buf16(x, cv.QNAN16["f16"], off=2)
    assert b.base == cv.GUARD + 2 and np.array_equal(b.host[b.base:b.base + 10], x) and b.host.size == 10 + 2 * cv.GUARD + 2
    assert cv.is_nan16(b.host[:b.base], "f16").all() and cv.is_nan16(b.host[b.base + 10:], "f16").all()
    assert cv.is_nan16(np.array([cv.QNAN16["bf16"]]), "bf16").all() and not cv.is_nan16(np.array([0x7F80, 0xFF80, 0x7C00], dtype=np.uint16), "bf16").any()
    c = cv.CBuf16(np.full(7, 3, dtype=np.uint16))
    assert (c.host[:cv.GUARD] == cv.SENT16).all() and (c.host[cv.GUARD + 7:] == cv.SENT16).all() and c.host.size == 7 + 2 * cv.GUARD + 8
    assert (2 * cv.GUARD) % 16 == 0


# ---------------------------------------------------------------------------------------------
# refusals, without a device: dummy non-null pointers
# ---------------------------------------------------------------------------------------------
BASE = 0x100000


@pytest.mark.parametrize("name", list(cv.REFUSALS))
def test_refusals_are_decided_before_any_device_call(pkg, name):
    geom, xo, bo, status = cv.REFUSALS[name]
    L = pkg.lib()
    for t in cv.TYPES:
        for routed in (False, True):
            rc = cv.call_refusal(L, name, t, BASE, BASE * 2, BASE * 3, routed)
            assert rc == status, f"{name} {t} routed={routed}: status {rc}: {L.sm_last_error().decode()}"
    form, _, why = library_answer(pkg, geom, 2 if xo else 16, bo == 0)
    assert form == "not_taken" and (why in ("invalid", "window")) == (status == cv.INVALID)
    for t in cv.TYPES:
        assert getattr(L, "sm_conv_spmma_fused_" + t)(None, BASE, BASE, *cv._GOOD, 1.0, 0.0, None) == cv.INVALID
