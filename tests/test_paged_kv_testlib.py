"""The paged-cache builder of tests/paged_kv_testlib.py itself, without a device: the index maps are what the layout says, the offsets an
unclamped kernel would form from the ids -1 and num_pages land in a guard page of the buffer (what the GPU tests of sm_attn_decode_* and
sm_rope_append_* rely on to SEE such a kernel instead of faulting), and the block table has the properties its cases name."""
import numpy as np
import pytest

from paged_kv_testlib import BAD32, CacheLayout, PageTable

# lens in P (the page size); absent: (sequence, column, "lo" | "hi"); shared: prefix columns of sequence 1 taken from sequence 0
TABLES = {
    "empty": dict(lens=["0"], max_pages=2),
    "one-token": dict(lens=["1"], max_pages=1),
    "page-edge": dict(lens=["P-1", "P+1"], max_pages=3),
    "shared-prefix": dict(lens=["3*P+1", "4*P", "2*P"], max_pages=5, shared=2, absent=[(0, 1, "lo"), (1, 3, "hi"), (2, 0, "hi")]),
}


def build(name, ps):
    t = TABLES[name]
    lens = [int(eval(x, {"P": ps})) for x in t["lens"]]
    return PageTable(lens, ps, t["max_pages"], np.random.default_rng(ps + len(name)), t.get("absent", ()), t.get("shared", 0)), t


@pytest.mark.parametrize("kv_width", [64, 256])
@pytest.mark.parametrize("ps", [16, 128])
@pytest.mark.parametrize("name", list(TABLES))
def test_the_cache_layout_keeps_an_unclamped_kernel_inside_its_guard_pages(name, ps, kv_width):
    pt, _ = build(name, ps)
    cl = CacheLayout(pt.num_pages, ps, kv_width, pt.seqs, pt.max_pages)
    # one entry per logical cache element, none twice; pitches above their extents
    assert cl.ikv.shape == (pt.num_pages, ps, kv_width) and np.unique(cl.ikv).size == cl.ikv.size == pt.num_pages * ps * kv_width
    assert cl.ldkv > kv_width and cl.page_stride > ps * cl.ldkv and cl.ldbt > pt.max_pages
    assert cl.ldkv % 8 == 0 and cl.page_stride % 8 == 0 and cl.kbase % 8 == 0, "the call needs 16-byte aligned token rows"
    assert cl.ikv.min() == cl.kbase and cl.ikv.max() < cl.n_kv and np.array_equal(cl.rows(np.arange(pt.num_pages), np.zeros(pt.num_pages)), cl.ikv[:, 0])
    logical = np.zeros(cl.n_kv, dtype=bool)
    logical[cl.ikv.reshape(-1)] = True
    # every row of the pages -1 and num_pages: inside the buffer, inside its guard page, on no logical element
    end = cl.kbase + pt.num_pages * cl.page_stride
    for bad, (lo, hi) in zip((-1, pt.num_pages), ((cl.kbase - cl.page_stride, cl.kbase), (end, end + cl.page_stride))):      # the two guard pages
        at = cl.rows(np.full(ps, bad), np.arange(ps))
        assert 0 <= lo <= at.min() and at.max() < hi <= cl.n_kv and not logical[at].any()
    # the buffers: nothing but the fill outside the live rows; the views start where the maps say
    live = np.zeros((pt.num_pages, ps), dtype=bool)
    live[0, 0] = live[-1, -1] = live[1, : ps // 2] = True
    g = cl.cache_buffer(0x7E00, live)
    assert g.host.size == cl.n_kv and g.base == cl.kbase and (g.host == 0x7E00).all()
    assert np.array_equal(g.idx, cl.ikv[live].reshape(-1)) and g.outside.sum() == cl.n_kv - live.sum() * kv_width
    assert cl.cache_buffer(0x2BCD).outside.all()


@pytest.mark.parametrize("ps", [16, 128])
@pytest.mark.parametrize("name", list(TABLES))
def test_the_page_table_has_the_properties_its_case_names(name, ps):
    pt, t = build(name, ps)
    absent = {(s, c): w for s, c, w in t.get("absent", ())}
    shared = t.get("shared", 0)
    assert pt.table.shape == (len(pt.lens), t["max_pages"]) and pt.table.dtype == np.int32
    assert pt.need == [-(-L // ps) for L in pt.lens] and pt.num_pages == sum(pt.need) + 3
    in_range = (pt.table >= 0) & (pt.table < pt.num_pages)
    for s, need in enumerate(pt.need):
        beyond = pt.table[s, need:]
        assert not in_range[s, need:].any() and np.array_equal(beyond, np.where(np.arange(beyond.size) % 2 == 0, -1, pt.num_pages)), "beyond ceil(L / P): -1, num_pages, -1 .."
        for c in range(need):
            want = {"lo": -1, "hi": pt.num_pages}.get(absent.get((s, c)))
            assert pt.table[s, c] == want if want is not None else in_range[s, c], "absent ids exactly where the case plants them"
        if need >= 2 and not any((s, c) in absent for c in range(need)) and not (s == 1 and shared):
            assert np.any(np.diff(pt.table[s, :need]) < 0), "a row of two or more pages is not monotone"
    if shared:
        keep = [c for c in range(shared) if (0, c) not in absent and (1, c) not in absent]
        assert keep and np.array_equal(pt.table[1, keep], pt.table[0, keep]), "the prefix pages are shared"
    # apart from the shared prefix no page is named twice, and three pages are named by nobody
    named = pt.table[in_range]
    assert named.size - np.unique(named).size == len([c for c in range(shared) if (0, c) not in absent and (1, c) not in absent])
    unnamed = pt.num_pages - np.unique(named).size
    assert unnamed >= 3 and (unnamed == 3 or absent or shared), "three pages no row refers to"


def test_the_table_buffer_holds_the_table_between_bad_ids():
    pt, _ = build("page-edge", 16)
    cl = CacheLayout(pt.num_pages, 16, 64, pt.seqs, pt.max_pages)
    g = cl.table_buffer(pt.table)
    assert g.host.size == cl.n_table and g.base == cl.tbase and np.unique(cl.it).size == cl.it.size == pt.table.size
    assert np.array_equal(g.host[cl.it].view(np.int32), pt.table) and (g.host[g.outside] == BAD32).all() and g.outside.sum() == cl.n_table - pt.table.size


def test_the_one_draw_from_the_rng_is_a_permutation_of_the_pages():
    """the cases' data were recorded under their seeds: the table takes exactly one permutation(num_pages) from the generator"""
    a, b = np.random.default_rng(7), np.random.default_rng(7)
    pt = PageTable([40, 3], 16, 4, a)
    b.permutation(pt.num_pages)
    assert a.integers(0, 1 << 30) == b.integers(0, 1 << 30)
