// attn_decode_common.h -- what the decode attention over the 16-bit cache (attn_decode.hip) and over the fp8 cache (attn_decode_kv8.hip)
// share: the chunk, the form and the workspace as functions of the geometry alone, the arguments of the 16-bit call (the combine reads its
// O, lse, workspace and length fields), the length clamp, the exponential and the SPLIT form's combine kernel.  The workspace layout is one:
// acc[seqs][q_heads][chunks][head_dim] fp32, then (m, l)[seqs][q_heads][chunks].
#pragma once
#include <math.h>

#include "mma_tile.h"
#include "paged_kv.h"
#include "quant_fp8.h"

namespace sm {

// tools/attn_decode_table.py builds attn_decode.hip alone at 128, 256 and 512 to time the chunk sizes against each other
#ifndef ATTN_DECODE_CHUNK
#define ATTN_DECODE_CHUNK SM_ATTN_DECODE_CHUNK
#endif
constexpr unsigned AD_CHUNK = ATTN_DECODE_CHUNK;
constexpr unsigned AD_TPW = AD_CHUNK / 4;  // tokens per wave
constexpr unsigned AD_NT = AD_TPW / 16;    // 16-token tiles per wave
constexpr float AD_LOG2E = 1.4426950408889634f;
static_assert(AD_CHUNK % SM_ATTN_DECODE_MAX_PAGE_SIZE == 0 && AD_CHUNK % 64 == 0 && AD_CHUNK <= 512, "the chunk is a multiple of every page size");

inline bool ad_head_dim_ok(size_t d) { return d == SM_ATTN_DECODE_MIN_HEAD_DIM || d == SM_ATTN_DECODE_MAX_HEAD_DIM; }
inline size_t ad_chunks(size_t page_size, size_t max_pages) { return ceil_div(mul_sat(page_size, max_pages), (size_t)AD_CHUNK); }

inline int attn_decode_form(size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t page_size, size_t max_pages) {
  if (!ad_head_dim_ok(head_dim) || !kv_page_size_ok(page_size) || !kv_context_fits(page_size, max_pages)) return SM_ATTN_DECODE_FORM_INVALID;
  if (q_heads > 0 && (kv_heads == 0 || q_heads % kv_heads != 0 || q_heads / kv_heads > SM_ATTN_DECODE_MAX_GROUP)) return SM_ATTN_DECODE_FORM_INVALID;
  if (seqs == 0 || q_heads == 0) return SM_ATTN_DECODE_FORM_EMPTY;
  return page_size * max_pages <= AD_CHUNK ? SM_ATTN_DECODE_FORM_DIRECT : SM_ATTN_DECODE_FORM_SPLIT;
}

// the workspace: acc[seqs][q_heads][chunks][head_dim] fp32, then (m, l)[seqs][q_heads][chunks]; SIZE_MAX: it overflows
inline size_t attn_decode_ws_bytes(size_t seqs, size_t q_heads, size_t head_dim, size_t page_size, size_t max_pages) {
  if (mul_sat(page_size, max_pages) <= AD_CHUNK) return 0;
  return mul_sat(mul_sat(mul_sat(seqs, q_heads), ad_chunks(page_size, max_pages)), mul_sat(head_dim + 2, sizeof(float)));
}

struct AdArgs {
  const uint16_t *Q, *K, *V;
  const int *bt, *sl;
  uint16_t* O;
  float *lse, *ws_acc, *ws_ml;  // lse: or null; ws_*: null in the DIRECT form
  size_t ldq, ldkv, page_stride, ldbt, ldo;
  unsigned q_heads, kv_heads, group, num_pages, page_size, page_shift, cap, nchunks;  // bt .. cap: the PagedKv fields (paged_kv.h)
  float scale;
};

#ifdef __HIPCC__
// L = clamp(seq_lens[s], 0, max_pages * page_size); any holder of sl and cap
template <class Holder>
__device__ __forceinline__ unsigned ad_len(const Holder& p, unsigned s) {
  const int l = p.sl[s];
  return l < 0 ? 0u : ((unsigned)l > p.cap ? p.cap : (unsigned)l);
}
__device__ __forceinline__ float ad_exp(float x) { return __builtin_amdgcn_exp2f(x * AD_LOG2E); }

// SPLIT: the ceil(L / CHUNK) chunks of (sequence, query head) blockIdx.x in ascending order; thread d owns column d
template <bool BF, int HD>
__global__ __launch_bounds__(HD) void attn_combine_kernel(const AdArgs p) {
  const unsigned sh = blockIdx.x, s = sh / p.q_heads, d = threadIdx.x;
  const unsigned L = ad_len(p, s), nch = (L + AD_CHUNK - 1u) / AD_CHUNK;
  const float* ml = p.ws_ml + (size_t)sh * p.nchunks * 2;
  const float* ac = p.ws_acc + (size_t)sh * p.nchunks * HD + d;
  float m = -INFINITY;
  for (unsigned c = 0; c < nch; ++c) m = __builtin_fmaxf(m, ml[2 * c]);
  const bool none = m == -INFINITY;  // L == 0, or every page absent
  float l = 0.0f, a = 0.0f;
  if (!none) {
    for (unsigned c = 0; c < nch; ++c) {
      const float w = ad_exp(ml[2 * c] - m);
      l += w * ml[2 * c + 1];
      a += w * ac[(size_t)c * HD];
    }
  }
  p.O[(size_t)s * p.ldo + (size_t)(sh % p.q_heads) * HD + d] = __builtin_bit_cast(uint16_t, to_elt<BF>(none ? 0.0f : a / l));
  if (d == 0 && p.lse) p.lse[sh] = none ? -INFINITY : m + logf(l);
}
#endif

}  // namespace sm
