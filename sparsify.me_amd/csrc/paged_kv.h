// paged_kv.h -- the paged KV cache, stated once for every kernel that reads or writes it (attn_decode.hip, rope_append.hip and, on the fp8 cache stated at the end, their _kv8 twins):
// Kc, Vc [num_pages][page_size][kv_heads][head_dim] 16-bit, a token row at pitch ldkv, a page at pitch page_stride; block_table int32
// [seqs][max_pages] at row pitch ldbt.  Token t (below cap = max_pages * page_size) of sequence s lives in page block_table[s][t / page_size]
// at row t % page_size.  A page whose id lies outside [0, num_pages) is ABSENT: nothing of it is read or written, and no address is formed
// from its id -- KV_OFFSET is used only under kv_present.  Host side: the geometry conditions as predicates -- each entry point keeps its own
// documented order of statuses and its own messages (include/sparsifyme.h) and interleaves them with others -- and the one fill.
#pragma once
#include "sm_common.h"

namespace sm {

constexpr size_t KV_I32_MAX = 0x7fffffffull;
inline bool kv_page_size_ok(size_t ps) { return ps >= SM_ATTN_DECODE_MIN_PAGE_SIZE && ps <= SM_ATTN_DECODE_MAX_PAGE_SIZE && (ps & (ps - 1)) == 0; }
// every pitch at least its extent; kv_width = kv_heads * head_dim (saturated)
inline bool kv_pitches_ok(size_t kv_width, size_t page_size, size_t max_pages, size_t ldkv, size_t page_stride, size_t ldbt) {
  return ldkv >= kv_width && page_stride >= mul_sat(page_size, ldkv) && ldbt >= max_pages;
}
// every field at most 2^31 - 1, and the longest context a table row can name
inline bool kv_fields_fit(size_t num_pages, size_t page_size, size_t max_pages, size_t ldkv, size_t page_stride, size_t ldbt) {
  return num_pages <= KV_I32_MAX && page_size <= KV_I32_MAX && max_pages <= KV_I32_MAX && ldkv <= KV_I32_MAX && page_stride <= KV_I32_MAX && ldbt <= KV_I32_MAX;
}
inline bool kv_context_fits(size_t page_size, size_t max_pages) { return mul_sat(max_pages, page_size) <= KV_I32_MAX; }
inline bool kv_rows_aligned16(size_t ldkv, size_t page_stride) { return ldkv % 8 == 0 && page_stride % 8 == 0; }  // (with a 16-byte aligned pointer)

// What a kernel holds of the cache: a new kernel embeds the struct in its arguments.  AdArgs and RaArgs carry the same eight fields under
// the same names where they always were -- everything below takes any holder of these names -- so that their kernarg bytes, with them the
// grouping of the kernarg loads, the SGPR counts and the instruction streams, stay what they were.
struct PagedKv {
  const int* bt;
  size_t ldbt, ldkv, page_stride;
  unsigned num_pages, page_size, page_shift, cap;
};
template <class Holder>  // (after kv_page_size_ok and the predicates held)
inline void paged_kv_fill(Holder& c, const int* block_table, size_t num_pages, size_t page_size, size_t max_pages, size_t ldkv, size_t page_stride, size_t ldbt) {
  c.bt = block_table; c.ldbt = ldbt; c.ldkv = ldkv; c.page_stride = page_stride;
  c.num_pages = (unsigned)num_pages; c.page_size = (unsigned)page_size; c.page_shift = (unsigned)__builtin_ctzll(page_size); c.cap = (unsigned)(max_pages * page_size);
}

#ifdef __HIPCC__
template <class Holder>  // the page id of token t < cap of sequence s, as the table holds it
__device__ __forceinline__ int kv_page_id(const Holder& c, size_t s, unsigned t) { return c.bt[s * c.ldbt + (t >> c.page_shift)]; }
template <class Holder>
__device__ __forceinline__ bool kv_present(const Holder& c, int id) { return id >= 0 && (unsigned)id < c.num_pages; }
#endif
// Element offset of token t's row in the PRESENT page `id`, in 64 bits.  A macro on purpose: behind a function boundary the compiler learns the
// range of t from rope_append's call site (a position that passed `pos >= 0`) and meets the mask as the left operand of the `and`; either
// way it drops the mask's top bit and assembles `page_size - 1` with a 32-bit literal instead of the inline constant -1.
#define KV_OFFSET(c, id, t) ((size_t)(id) * (c).page_stride + (size_t)((t) & ((c).page_size - 1u)) * (c).ldkv)

// ---- the fp8 cache (attn_decode_kv8.hip, rope_append_kv8.hip): Kc8, Vc8 are fp8 bytes (one format, SM_FP8_E4M3 or SM_FP8_E5M2, for both)
// in the layout above -- ldkv and page_stride in elements = bytes, rows 16-byte aligned -- and Ksc, Vsc fp32 [num_pages][kv_heads][page_size]
// at page pitch scale_page_stride: one scale per (token, kv head), element d of the token in (page, slot), head g, is
// fp32(byte) * Ksc[page][g][slot].  Head-major inside a page on purpose: the 16 scales of a 16-token score tile are 64 contiguous bytes, and
// the lane that holds tokens 4 (l >> 4) + r of a tile loads its four with one 16-byte load.  Block table, lengths, page sizes and the ABSENT
// rule are the 16-bit cache's: KV8_SCALE_OFFSET, like KV_OFFSET, is used only under kv_present.
inline bool kv8_rows_aligned16(size_t ldkv, size_t page_stride) { return ldkv % 16 == 0 && page_stride % 16 == 0; }  // (with a 16-byte aligned pointer)
inline bool kv8_scale_pitch_ok(size_t kv_heads, size_t page_size, size_t scale_page_stride) { return scale_page_stride >= mul_sat(kv_heads, page_size); }
inline bool kv8_scale_rows_aligned16(size_t scale_page_stride) { return scale_page_stride % 4 == 0; }  // (with a 16-byte aligned pointer)
// Element offset of the scale of token t, kv head g, in the PRESENT page `id`
#define KV8_SCALE_OFFSET(c, id, g, t) ((size_t)(id) * (c).scale_page_stride + (size_t)(g) * (c).page_size + ((t) & ((c).page_size - 1u)))

}  // namespace sm
