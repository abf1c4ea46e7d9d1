// moe_combine.hip -- sm_moe_combine_{f16,bf16} (extension): the un-permute and the weighted sum over top_k that close a mixture-of-experts
// feed-forward block.  Yp holds one row per routed pair in the SORTED order the grouped layers write (row pair_pos[p] is pair p's);
//     out[t][h] = round( R[t][h] + sum_{j ascending} weights[t * top_k + j] * Yp[pair_pos[t * top_k + j]][h] )
// all in fp32: s = R or +0; per kept pair q = w * y (ONE fp32 multiply; q = y without weights), s = s + q (ONE fp32 add) -- never
// contracted into an fma -- then one rounding to nearest even.  A pair with pos < 0 or pos >= rows_p is skipped.  A gather, not a
// scatter: every output element has one thread, the sum has one order, no atomics; the same bits on every run.  R == out is in place
// (the thread reads its piece of R before it writes it).
// Two forms (sm_moe_combine_form): VEC moves 16-byte pieces (eight elements) of Yp, R and out; SCALAR single elements.
#include "mma_tile.h"

namespace sm {

constexpr int MOE_COMBINE_NT = 256;

inline int moe_combine_form(const void* Yp, const void* R, const void* out, size_t hidden, size_t ldp, size_t ldo) {
  if (!Yp || !out || ldp < hidden || ldo < hidden || hidden > 0x7fffffffull || ldp > 0x7fffffffull || ldo > 0x7fffffffull) return SM_MOE_COMBINE_FORM_INVALID;
  if (hidden == 0) return SM_MOE_COMBINE_FORM_EMPTY;
  const bool vec = hidden % 8 == 0 && ldp % 8 == 0 && ldo % 8 == 0 && aligned16(Yp) && aligned16(R) && aligned16(out);
  return vec ? SM_MOE_COMBINE_FORM_VEC : SM_MOE_COMBINE_FORM_SCALAR;
}

struct MoeCombineArgs {
  const half_t* Yp;
  const int* pair_pos;
  const float* weights;  // or null
  const half_t* R;       // or null
  half_t* out;
  size_t ldp, ldo;
  unsigned tokens, top_k, hidden, rows_p;
};

// V elements per thread: 8 (one 16-byte piece) or 1
template <bool BF, int V>
__global__ __launch_bounds__(MOE_COMBINE_NT) void moe_combine_kernel(const MoeCombineArgs a) {
  struct alignas(2 * V) Piece { half_t v[V]; };  // V = 8: one 16-byte access
  const size_t per_row = a.hidden / V, total = (size_t)a.tokens * per_row;
  for (size_t i = (size_t)blockIdx.x * MOE_COMBINE_NT + threadIdx.x; i < total; i += (size_t)gridDim.x * MOE_COMBINE_NT) {
    const size_t t = i / per_row, h = (i - t * per_row) * V;
    float s[V];
#pragma unroll
    for (int q = 0; q < V; ++q) s[q] = 0.f;
    if (a.R) {
      const Piece r = *reinterpret_cast<const Piece*>(a.R + t * a.ldo + h);
#pragma unroll
      for (int q = 0; q < V; ++q) s[q] = to_f32<BF>(r.v[q]);
    }
    for (unsigned j = 0; j < a.top_k; ++j) {
      const size_t p = t * a.top_k + j;
      const int pos = a.pair_pos[p];
      if (pos < 0 || (unsigned)pos >= a.rows_p) continue;
      const Piece y = *reinterpret_cast<const Piece*>(a.Yp + (size_t)pos * a.ldp + h);
      if (a.weights) {
        const float w = a.weights[p];
#pragma unroll
        for (int q = 0; q < V; ++q) {
#pragma clang fp contract(off)
          const float m = w * to_f32<BF>(y.v[q]);
          s[q] = s[q] + m;
        }
      } else {
#pragma unroll
        for (int q = 0; q < V; ++q) s[q] = s[q] + to_f32<BF>(y.v[q]);
      }
    }
    Piece o;
#pragma unroll
    for (int q = 0; q < V; ++q) o.v[q] = to_elt<BF>(s[q]);
    *reinterpret_cast<Piece*>(a.out + t * a.ldo + h) = o;
  }
}

template <bool BF>
static int moe_combine(const void* Yp, const int* pair_pos, const float* weights, const void* R, void* out, size_t tokens, size_t top_k, size_t hidden,
                       size_t rows_p, size_t ldp, size_t ldo, sm_stream_t stream) {
  static const char* const who = "sm_moe_combine_{f16,bf16}";
  if (!Yp || !pair_pos || !out || ldp < hidden || ldo < hidden) {
    set_error("%s: invalid argument (null Yp, pair_pos or out, ldp < hidden or ldo < hidden)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  const size_t lim = 0x7fffffffull;
  if (tokens > lim || top_k > lim || hidden > lim || rows_p > lim || ldp > lim || ldo > lim || (top_k != 0 && tokens > lim / top_k)) {
    set_error("%s: tokens * top_k or a dimension exceeds 2^31-1", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (tokens == 0 || top_k == 0 || hidden == 0) return SM_STATUS_SUCCESS;
  const MoeCombineArgs a = {(const half_t*)Yp, pair_pos, weights, (const half_t*)R, (half_t*)out, ldp, ldo, (unsigned)tokens, (unsigned)top_k, (unsigned)hidden,
                            (unsigned)rows_p};
  hipStream_t st = (hipStream_t)stream;
  if (moe_combine_form(Yp, R, out, hidden, ldp, ldo) == SM_MOE_COMBINE_FORM_VEC) {
    moe_combine_kernel<BF, 8><<<dim3(stream_grid(tokens * (hidden / 8), MOE_COMBINE_NT, true)), dim3(MOE_COMBINE_NT), 0, st>>>(a);
  } else {
    moe_combine_kernel<BF, 1><<<dim3(stream_grid(tokens * hidden, MOE_COMBINE_NT, true)), dim3(MOE_COMBINE_NT), 0, st>>>(a);
  }
  return check_launch("moe_combine_kernel");
}

}  // namespace sm

using namespace sm;

extern "C" int sm_moe_combine_form(const void* Yp, const void* R, const void* out, size_t hidden, size_t ldp, size_t ldo, int* form) {
  if (!form) {
    set_error("sm_moe_combine_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = moe_combine_form(Yp, R, out, hidden, ldp, ldo);
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_moe_combine_f16(const void* Yp, const int* pair_pos, const float* weights, const void* R, void* out, size_t tokens, size_t top_k,
                                  size_t hidden, size_t rows_p, size_t ldp, size_t ldo, sm_stream_t stream) {
  return moe_combine<false>(Yp, pair_pos, weights, R, out, tokens, top_k, hidden, rows_p, ldp, ldo, stream);
}
extern "C" int sm_moe_combine_bf16(const void* Yp, const int* pair_pos, const float* weights, const void* R, void* out, size_t tokens, size_t top_k,
                                   size_t hidden, size_t rows_p, size_t ldp, size_t ldo, sm_stream_t stream) {
  return moe_combine<true>(Yp, pair_pos, weights, R, out, tokens, top_k, hidden, rows_p, ldp, ldo, stream);
}
