"""The paged KV cache of the sm_attn_decode_* and sm_rope_append_* tests, stated once (the library's side: csrc/paged_kv.h).
PageTable: the block table of a case -- permuted and not monotone, bad ids (-1 / num_pages, alternating) in every column beyond a sequence's
live ones, three pages no row refers to, absent ids planted inside the live range, prefix pages shared between sequences 0 and 1.  It draws
from the case's rng exactly once (one permutation of the pages): the cases' data were recorded under these seeds.
CacheLayout: where the cache and the table lie in their guarded buffers -- pitches above their extents, a guard page in front of page 0 and
behind the last page, so that the offset an unclamped kernel forms from id -1 or num_pages lands inside the buffer, where the whole-buffer
comparison sees it, instead of faulting -- and the index maps of the logical elements.  numpy only: the buffers it hands out are
guard_testlib.Guarded, uploaded by their own to_device(); the views take the device tensor."""
import numpy as np

from guard_testlib import Guarded

BAD32 = 0x7FFFFFF0                       # around the table: an id that names nothing near


class PageTable:
    """lens: tokens per sequence (each at most max_pages * page_size); absent: (sequence, column, "lo" | "hi") with a column inside the
    sequence's live ones, id -1 / num_pages; shared: the first `shared` columns of sequence 1 are sequence 0's."""

    def __init__(self, lens, page_size, max_pages, rng, absent=(), shared=0):
        self.lens, self.ps, self.max_pages, self.seqs = list(lens), page_size, max_pages, len(lens)
        assert all(0 <= L <= max_pages * page_size for L in self.lens)
        self.need = need = [-(-L // page_size) for L in self.lens]       # live columns per sequence
        self.num_pages = sum(need) + 3                                   # three pages no table refers to
        perm = rng.permutation(self.num_pages)
        self.table = np.empty((self.seqs, max_pages), dtype=np.int32)
        at = 0
        for s in range(self.seqs):
            row = perm[at:at + need[s]]
            at += need[s]
            if need[s] > 1 and not np.any(np.diff(row) < 0):
                row = row[::-1]
            if s == 1 and shared:
                row = np.concatenate([self.table[0, :shared], row[shared:]])
            bad = np.where(np.arange(max_pages - need[s]) % 2 == 0, -1, self.num_pages)       # never read
            self.table[s] = np.concatenate([row, bad]).astype(np.int32)
            assert need[s] < 2 or np.any(np.diff(row) < 0), "the page table is not monotone"
        for s, col, which in absent:
            assert col < need[s]
            self.table[s, col] = -1 if which == "lo" else self.num_pages


class CacheLayout:
    """kv_width = kv_heads * head_dim.  ikv [num_pages][page_size][kv_width] and it [seqs][max_pages]: buffer indices of the logical elements."""

    def __init__(self, num_pages, page_size, kv_width, seqs, max_pages):
        self.num_pages, self.ps, self.kv_width, self.seqs, self.max_pages = num_pages, page_size, kv_width, seqs, max_pages
        self.ldkv = kv_width + 16
        self.page_stride = page_size * self.ldkv + 8
        self.kbase = 8 + self.page_stride                                      # a guard page in front of page 0 ...
        self.n_kv = self.kbase + (num_pages + 1) * self.page_stride + 16       # ... and one behind the last page
        self.ldbt, self.tbase = max_pages + 3, 5
        self.n_table = self.tbase + seqs * self.ldbt + 7
        ar = np.arange
        self.ikv = self.kbase + ar(num_pages)[:, None, None] * self.page_stride + ar(page_size)[None, :, None] * self.ldkv + ar(kv_width)[None, None, :]
        self.it = self.tbase + ar(seqs)[:, None] * self.ldbt + ar(max_pages)[None, :]

    def rows(self, page, slot):
        """[n][kv_width]: buffer indices of the token rows (page[i], slot[i]); ids -1 and num_pages give what an unclamped kernel would address"""
        page, slot = np.asarray(page, dtype=np.int64), np.asarray(slot, dtype=np.int64)
        return self.kbase + page[:, None] * self.page_stride + slot[:, None] * self.ldkv + np.arange(self.kv_width)[None, :]

    def cache_buffer(self, fill, live=None):
        """a K or V buffer full of `fill`; live [num_pages][page_size] bool: the token rows that are its logical elements (None: none are)"""
        return Guarded(self.n_kv, fill, np.uint16, self.kbase, idx=self.ikv[np.zeros(self.ikv.shape[:2], dtype=bool) if live is None else live].reshape(-1))

    def table_buffer(self, table):
        g = Guarded(self.n_table, BAD32, np.uint32, self.tbase, idx=self.it.reshape(-1))
        g.host[g.idx] = np.ascontiguousarray(table, dtype=np.int32).reshape(-1).view(np.uint32)
        return g

    def cache_view(self, dev, kv_heads, head_dim):
        """the 4-D cache the call is given, on the device tensor of a cache_buffer viewed in the 16-bit type"""
        assert kv_heads * head_dim == self.kv_width
        return dev.as_strided((self.num_pages, self.ps, kv_heads, head_dim), (self.page_stride, self.ldkv, head_dim, 1), self.kbase)

    def table_view(self, dev):
        return dev.as_strided((self.seqs, self.max_pages), (self.ldbt, 1), self.tbase)
