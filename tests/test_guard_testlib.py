"""The guard logic of tests/guard_testlib.py itself, without a device: a flipped element outside the logical region is reported with its
index wherever it lies, one inside is not; the index maps are what the layout says; the seed is the seed the cases were recorded with."""
import numpy as np
import pytest

from guard_testlib import BYTE, UNSIGNED, Guarded, Layout, Strided, bytes_outside_written, changed_outside, seed

M, N, K = 5, 8, 12
LAY = dict(lda_pad=4, gapA=8, gapB=8, gapC=3, offA=8, offB=8, offC=1, batch=2)
G = 4                                      # guard elements in front of and behind the buffers of this file
FILL = {1: 0x7F, 2: 0x7E00, 4: 0x7FC00000, 8: 0xFFFFFFFFFFFFFFFF}


def geometry():
    lay = Layout(**LAY)
    return Strided(M, N, K, lay, G + lay.offA, G + lay.offB, G + lay.offC)


def said(n, first):
    return f"flip: {n} elements outside the logical region were written, first at {first}"


def flipped(g, pos):
    """What a read-back would give had the device changed element pos alone."""
    got = g.host.copy()
    got[pos] ^= 1
    return got


def assert_reported(g, pos):
    got = flipped(g, pos)
    assert changed_outside(got, g.host, g.idx).tolist() == [pos]
    with pytest.raises(AssertionError, match=rf"1 elements outside .* first at \[{pos}\]"):
        g.assert_outside_kept(said, got)


def assert_not_reported(g, pos):
    got = flipped(g, pos)
    assert changed_outside(got, g.host, g.idx).size == 0
    assert g.result(said, got)[0 if pos == g.base else -1] == got[pos]      # (the positions tried are the first and the last logical element)


def test_index_maps_have_one_entry_per_logical_element():
    s, batch = geometry(), LAY["batch"]
    assert s.nb == batch and (s.lda, s.sA, s.sB, s.sC) == (K + 4, M * (K + 4) + 8, K * N + 8, M * N + 3)
    for idx, count in ((s.iA, batch * M * K), (s.iB, s.nb * K * N), (s.iC, batch * M * N)):
        assert idx.size == count == np.unique(idx).size
    assert (s.iA[0], s.iB[0], s.iC[0]) == (s.baseA, s.baseB, s.baseC) == (G + 8, G + 8, G + 1)
    shared = Strided(M, N, K, Layout(**dict(LAY, gapB=None)), 0, 0, 0)
    assert shared.nb == 1 and shared.sB == 0 and shared.iB.size == K * N == np.unique(shared.iB).size


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_a_flip_outside_the_strided_region_is_reported_and_one_inside_is_not(width):
    s = geometry()
    g = Guarded(s.baseA + LAY["batch"] * s.sA + G, FILL[width], UNSIGNED[width], s.baseA, s.iA)
    g.host[s.iA] = np.arange(s.iA.size, dtype=UNSIGNED[width])
    last = int(s.iA[-1])
    assert last + 1 < g.host.size - 1 and g.outside.sum() == g.host.size - s.iA.size
    for pos in (0,                         # the front guard
                s.baseA + K,               # the lda padding of the first row
                s.baseA + M * s.lda,       # the gap between the two batches
                last + 1,                  # directly behind the last logical element
                g.host.size - 1):          # the last guard element
        assert_reported(g, pos)
    for pos in (s.baseA, last):
        assert_not_reported(g, pos)
    assert changed_outside(g.host.copy(), g.host, g.idx).size == 0


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_a_flip_around_a_contiguous_payload_is_reported_and_one_inside_is_not(width):
    payload = np.arange(1, 11, dtype=UNSIGNED[width])
    g = Guarded.around(payload, FILL[width], G + 1, G)
    assert g.host.dtype == UNSIGNED[width] and g.base == G + 1 and g.host.size == 10 + 2 * G + 1 and np.array_equal(g.host[g.idx], payload)
    for pos in (0, g.base - 1, g.base + 10, g.host.size - 1):
        assert_reported(g, pos)
    for pos in (g.base, g.base + 9):
        assert_not_reported(g, pos)


def test_a_byte_outside_the_region_is_seen():
    h = np.full(16 + 40 + 32, BYTE, dtype=np.uint8)
    h[16:56] = 0
    assert not bytes_outside_written(h, 16, 40)
    for pos in (0, 15, 56, h.size - 1):
        w = h.copy()
        w[pos] = 0
        assert bytes_outside_written(w, 16, 40)


def test_the_seed_is_the_one_the_cases_were_recorded_with():
    assert seed(0x5718, "a", 3) == 861957950
    assert seed(0x5716, "a", 3) != seed(0x5718, "a", 3) != seed(0x2404, "a", 3)
