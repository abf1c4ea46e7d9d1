// moe_gate.hip -- sm_moe_gate_{f16,bf16,f32} (extension): the router's logits[tokens][experts] to what sm_moe_route (topk_ids) and
// sm_moe_combine_* (topk_weights) read, in one launch.  The definition (include/sparsifyme.h) fixes every id; the weights are fp32
// arithmetic in a stated order.
//
// One wave per token, MOE_GATE_NW waves per workgroup, no LDS, no barrier (a wave past the last token leaves at once).
//   load    lane l holds experts l, l + 64, ...: KPL = ceil(experts / 64) keys per lane, rounded up to an instantiation (1, 2, 4, 8,
//           16); every load instruction reads 64 consecutive elements of the row.
//   pack    key -> (order-preserving u32 of the fp32 key) << 32 | ~e.  -0 is packed as +0 (they are EQUAL keys), a NaN as -inf.  A plain
//           unsigned maximum is then "largest key, lowest expert".  An expert past `experts` and a retired entry are 0, below every
//           real entry (a real entry's low word is ~e != 0), and top_k <= experts: every round finds a real, not yet taken expert --
//           distinct ids in [0, experts) whatever the logits hold.
//   select  top_k rounds: the lane's maximum over its registers, the wave's by six __shfl_xor steps (the 64-bit value as two 32-bit
//           shuffles: ds_bpermute, no LDS memory touched), the owner (the entry equal to the winner: e is part of it) retires it;
//           lane j keeps round j's expert.
//   weigh   lane j reads x of its expert again (one gathered load per wave from the row the wave has just read); m and the sums as
//           the header states them: the sum over j by a wave-uniform loop of v_readlane in ascending j, the sum over all experts
//           (SOFTMAX without renormalize only) per lane and then across the wave.  expf is the library's (never the fast intrinsic),
//           the division the correctly rounded one.
//   store   lanes 0 .. top_k - 1 write ids and weights: one coalesced store each.
#include "sm_common.h"

namespace sm {

constexpr int MOE_GATE_NW = 4, MOE_GATE_NT = 64 * MOE_GATE_NW;
static_assert(SM_MOE_GATE_MAX_TOP_K <= 64, "lane j keeps result j");
static_assert(SM_LINEAR24_MAX_GROUPS <= 64 * 16, "the largest instantiation holds 16 keys per lane");

inline int moe_gate_form(size_t tokens, size_t experts, size_t top_k) {
  const size_t lim = 0x7fffffffull;
  if (top_k > experts || tokens > lim || experts > SM_LINEAR24_MAX_GROUPS || top_k > SM_MOE_GATE_MAX_TOP_K) return SM_MOE_GATE_FORM_INVALID;
  if (top_k != 0 && tokens > lim / top_k) return SM_MOE_GATE_FORM_INVALID;
  if (tokens == 0 || top_k == 0) return SM_MOE_GATE_FORM_EMPTY;
  const size_t kpl = ceil_div(experts, 64);
  return kpl <= 1 ? SM_MOE_GATE_FORM_LANE1 : kpl <= 2 ? SM_MOE_GATE_FORM_LANE2 : kpl <= 4 ? SM_MOE_GATE_FORM_LANE4 : kpl <= 8 ? SM_MOE_GATE_FORM_LANE8
                                                                                                                                : SM_MOE_GATE_FORM_LANE16;
}

struct MoeGateArgs {
  const void* logits;
  const float* bias;  // or null
  int* ids;
  float* weights;
  size_t ld;
  unsigned tokens, experts, top_k;
  int scoring, renorm;
  float scale;
};

// T: 0 fp16, 1 bf16, 2 fp32.  The conversion to fp32 is exact.
template <int T>
__device__ __forceinline__ float gate_load(const void* base, size_t i) {
  if constexpr (T == 2) return reinterpret_cast<const float*>(base)[i];
  else if constexpr (T == 1) return __builtin_bit_cast(float, (unsigned)reinterpret_cast<const unsigned short*>(base)[i] << 16);
  else return (float)reinterpret_cast<const half_t*>(base)[i];
}

__device__ __forceinline__ float gate_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ unsigned long long gate_pack(float key, unsigned e) {
  unsigned b = __builtin_bit_cast(unsigned, key);
  if (key != key) b = 0xff800000u;   // NaN counts as -inf
  if ((b << 1) == 0u) b = 0u;        // -0 == +0
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((unsigned long long)b << 32) | (unsigned)~e;
}

__device__ __forceinline__ unsigned long long gate_wave_max(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned hi = (unsigned)__shfl_xor((int)(v >> 32), d), lo = (unsigned)__shfl_xor((int)v, d);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

template <class F>
__device__ __forceinline__ float gate_wave_reduce(float v, F f) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = f(v, __shfl_xor(v, d));
  return v;
}

// sum over lanes 0 .. n - 1 in ascending lane order (n wave-uniform, <= 64): v_readlane and a scalar-issued chain of fp32 adds
__device__ __forceinline__ float gate_ordered_sum(float v, unsigned n) {
  float s = 0.0f;  // (+0 + v_0 == v_0 for every v_0 but -0, which no exponential and no sigmoid gives)
  for (unsigned j = 0; j < n; ++j) s = s + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), (int)j));
  return s;
}

template <int T, int KPL>
__global__ __launch_bounds__(MOE_GATE_NT) void moe_gate_kernel(const MoeGateArgs a) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned t = blockIdx.x * MOE_GATE_NW + (threadIdx.x >> 6);
  if (t >= a.tokens) return;  // (wave-uniform; no barrier in this kernel)
  const size_t row = (size_t)t * a.ld;
  const bool softmax_all = a.scoring == SM_MOE_SCORE_SOFTMAX && !a.renorm;

  float x[KPL];
  unsigned long long pk[KPL];
#pragma unroll
  for (int r = 0; r < KPL; ++r) {
    const unsigned e = lane + 64u * r;
    pk[r] = 0ull;
    x[r] = -INFINITY;
    if (e < a.experts) {
      x[r] = gate_load<T>(a.logits, row + e);
      float key = x[r];
      if (a.bias) key = gate_sigmoid(key) + a.bias[e];
      pk[r] = gate_pack(key, e);
    }
  }

  // SOFTMAX without renormalize: m and S over all the experts
  float m_all = 0.0f, S_all = 0.0f;
  if (softmax_all) {
    float m = x[0];
#pragma unroll
    for (int r = 1; r < KPL; ++r) m = fmaxf(m, x[r]);
    m_all = gate_wave_reduce(m, [](float p, float q) { return fmaxf(p, q); });
    float s = 0.0f;
#pragma unroll
    for (int r = 0; r < KPL; ++r)
      if (lane + 64u * r < a.experts) s += expf(x[r] - m_all);
    S_all = gate_wave_reduce(s, [](float p, float q) { return p + q; });
  }

  unsigned my_id = 0;  // (lanes top_k .. 63 keep 0: an address inside the row for their load below)
  for (unsigned j = 0; j < a.top_k; ++j) {
    unsigned long long best = pk[0];
#pragma unroll
    for (int r = 1; r < KPL; ++r) best = pk[r] > best ? pk[r] : best;
    best = gate_wave_max(best);
#pragma unroll
    for (int r = 0; r < KPL; ++r)
      if (pk[r] == best) pk[r] = 0ull;
    if (lane == j) my_id = ~(unsigned)best;
  }

  const float xj = gate_load<T>(a.logits, row + my_id);
  float w;
  if (a.scoring == SM_MOE_SCORE_SOFTMAX) {
    const float m = softmax_all ? m_all : __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, xj)));
    const float ej = expf(xj - m);
    const float S = softmax_all ? S_all : gate_ordered_sum(ej, a.top_k);
    w = (ej / S) * a.scale;
  } else {
    const float q = gate_sigmoid(xj);
    w = a.renorm ? (q / gate_ordered_sum(q, a.top_k)) * a.scale : q * a.scale;
  }
  if (lane < a.top_k) {
    const size_t p = (size_t)t * a.top_k + lane;
    a.ids[p] = (int)my_id;
    a.weights[p] = w;
  }
}

template <int T>
static int moe_gate(const void* logits, const float* select_bias, int* topk_ids, float* topk_weights, size_t tokens, size_t experts, size_t top_k, size_t ld,
                    int scoring, int renormalize, float scale, sm_stream_t stream) {
  static const char* const who = "sm_moe_gate_{f16,bf16,f32}";
  if (!logits || !topk_ids || !topk_weights || ld < experts || top_k > experts || (scoring != SM_MOE_SCORE_SOFTMAX && scoring != SM_MOE_SCORE_SIGMOID) ||
      (select_bias && scoring == SM_MOE_SCORE_SOFTMAX)) {
    set_error("%s: invalid argument (null logits, topk_ids or topk_weights, ld < experts, top_k > experts, scoring not SM_MOE_SCORE_*, or a select_bias "
              "with SM_MOE_SCORE_SOFTMAX)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  const size_t lim = 0x7fffffffull;
  if (tokens > lim || experts > lim || top_k > lim || ld > lim || (top_k != 0 && tokens > lim / top_k) || (ld != 0 && tokens > lim / ld)) {
    set_error("%s: tokens * top_k, tokens * ld or a dimension exceeds 2^31-1", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (experts > SM_LINEAR24_MAX_GROUPS) {
    set_error("%s: experts exceeds SM_LINEAR24_MAX_GROUPS", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (top_k > SM_MOE_GATE_MAX_TOP_K) {
    set_error("%s: top_k exceeds SM_MOE_GATE_MAX_TOP_K", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (tokens == 0 || top_k == 0) return SM_STATUS_SUCCESS;
  const MoeGateArgs a = {logits, select_bias, topk_ids, topk_weights, ld, (unsigned)tokens, (unsigned)experts, (unsigned)top_k, scoring, renormalize != 0, scale};
  const dim3 grid((unsigned)ceil_div(tokens, MOE_GATE_NW)), block(MOE_GATE_NT);
  hipStream_t st = (hipStream_t)stream;
  switch (moe_gate_form(tokens, experts, top_k)) {
    case SM_MOE_GATE_FORM_LANE1: moe_gate_kernel<T, 1><<<grid, block, 0, st>>>(a); break;
    case SM_MOE_GATE_FORM_LANE2: moe_gate_kernel<T, 2><<<grid, block, 0, st>>>(a); break;
    case SM_MOE_GATE_FORM_LANE4: moe_gate_kernel<T, 4><<<grid, block, 0, st>>>(a); break;
    case SM_MOE_GATE_FORM_LANE8: moe_gate_kernel<T, 8><<<grid, block, 0, st>>>(a); break;
    default: moe_gate_kernel<T, 16><<<grid, block, 0, st>>>(a); break;
  }
  return check_launch("moe_gate_kernel");
}

}  // namespace sm

using namespace sm;

extern "C" int sm_moe_gate_form(size_t tokens, size_t experts, size_t top_k, int* form) {
  if (!form) {
    set_error("sm_moe_gate_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = moe_gate_form(tokens, experts, top_k);
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_moe_gate_f16(const void* logits, const float* select_bias, int* topk_ids, float* topk_weights, size_t tokens, size_t experts, size_t top_k,
                               size_t ld, int scoring, int renormalize, float scale, sm_stream_t stream) {
  return moe_gate<0>(logits, select_bias, topk_ids, topk_weights, tokens, experts, top_k, ld, scoring, renormalize, scale, stream);
}
extern "C" int sm_moe_gate_bf16(const void* logits, const float* select_bias, int* topk_ids, float* topk_weights, size_t tokens, size_t experts, size_t top_k,
                                size_t ld, int scoring, int renormalize, float scale, sm_stream_t stream) {
  return moe_gate<1>(logits, select_bias, topk_ids, topk_weights, tokens, experts, top_k, ld, scoring, renormalize, scale, stream);
}
extern "C" int sm_moe_gate_f32(const void* logits, const float* select_bias, int* topk_ids, float* topk_weights, size_t tokens, size_t experts, size_t top_k,
                               size_t ld, int scoring, int renormalize, float scale, sm_stream_t stream) {
  return moe_gate<2>(logits, select_bias, topk_ids, topk_weights, tokens, experts, top_k, ld, scoring, renormalize, scale, stream);
}
