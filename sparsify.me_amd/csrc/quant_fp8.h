// quant_fp8.h -- the per-row fp8 rule of include/sparsifyme.h on 16-bit source bits, shared by quant_fp8.hip (the quantisers) and
// rmsnorm.hip (the norm with an fp8 output): the two 16-bit source kinds, the conversion of four elements with the non-finite
// byte rule, the packed maximum over magnitude bits and its reduction over the 2^L lanes of a row.
#pragma once
#include "sm_common.h"

namespace sm {

inline bool fmt_ok(int f) { return f == SM_FP8_E4M3 || f == SM_FP8_E5M2; }

template <int FMT>
struct F8Lim {
  static constexpr float fmax = FMT == SM_FP8_E4M3 ? 448.0f : 57344.0f;
};

// 16-bit source kinds: magnitude bits of the infinity, fp32 value of the bits, the bits of an fp32 value
template <bool BF>
struct Src16 {
  static constexpr uint32_t inf = BF ? 0x7f80u : 0x7c00u;
  static __device__ __forceinline__ float f32(uint32_t h) {
    if constexpr (BF) return __builtin_bit_cast(float, h << 16);
    else return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
  }
  static __device__ __forceinline__ uint32_t bits(float x) {  // rounded to nearest even, once
    if constexpr (BF) return __builtin_bit_cast(uint16_t, (__bf16)x);
    else return __builtin_bit_cast(uint16_t, (_Float16)x);
  }
};
// four dwords of eight 16-bit elements <-> eight fp32 (rope_append.hip; attn_decode.hip writes the first out, see there)
template <bool BF>
__device__ __forceinline__ void unpack8(const u4 v, float (&x)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    x[2 * e] = Src16<BF>::f32(v[e] & 0xffffu);
    x[2 * e + 1] = Src16<BF>::f32(v[e] >> 16);
  }
}
template <bool BF>
__device__ __forceinline__ u4 pack8(const float (&y)[8]) {
  u4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = Src16<BF>::bits(y[2 * e]) | (Src16<BF>::bits(y[2 * e + 1]) << 16);
  return v;
}

// two fp32 -> two fp8 bytes in the low / high half of `old` (v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32: OCP encodings on
// gfx950, round to nearest even, subnormals of the format included)
template <int FMT, bool HI>
__device__ __forceinline__ uint32_t cvt2(float a, float b, uint32_t old) {
  if constexpr (FMT == SM_FP8_E4M3) return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, (int)old, HI);
  else return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, (int)old, HI);
}

// the byte a non-finite source element becomes (h: its 16 bits)
template <bool BF, int FMT>
__device__ __forceinline__ uint32_t nonfinite_byte(uint32_t h) {
  if constexpr (FMT == SM_FP8_E5M2) {
    if ((h & 0x7fffu) == Src16<BF>::inf) return 0x7cu | ((h >> 8) & 0x80u);
  }
  return 0x7fu;
}

// {x1:x0}, {x3:x2} (16-bit source elements) -> four fp8 bytes of y = fp32(x) * inv; SAT: y clamped to +-FMAX first.
// `fix`: the dwords may hold non-finite elements, patch their bytes.
template <bool BF, int FMT, bool SAT>
__device__ __forceinline__ uint32_t quant4(uint32_t d0, uint32_t d1, float inv, bool fix) {
  float y[4] = {Src16<BF>::f32(d0 & 0xffffu) * inv, Src16<BF>::f32(d0 >> 16) * inv, Src16<BF>::f32(d1 & 0xffffu) * inv,
                Src16<BF>::f32(d1 >> 16) * inv};
  if constexpr (SAT) {
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = __builtin_fminf(__builtin_fmaxf(y[e], -F8Lim<FMT>::fmax), F8Lim<FMT>::fmax);
  }
  uint32_t q = cvt2<FMT, false>(y[0], y[1], 0u);
  q = cvt2<FMT, true>(y[2], y[3], q);
  if (fix) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t h = ((e < 2 ? d0 : d1) >> (16 * (e & 1))) & 0xffffu;
      if ((h & 0x7fffu) >= Src16<BF>::inf) q = (q & ~(0xffu << (8 * e))) | (nonfinite_byte<BF, FMT>(h) << (8 * e));
    }
  }
  return q;
}

// packed 16-bit maximum of the magnitude bits; FINITE: non-finite elements count as 0
template <bool BF, bool FINITE>
__device__ __forceinline__ uint32_t mag_max8(uint32_t acc, const u4& d) {
  typedef unsigned short us2 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t a = d[i] & 0x7fff7fffu;
    if constexpr (FINITE) {
      if ((a & 0xffffu) >= Src16<BF>::inf) a &= 0xffff0000u;
      if ((a >> 16) >= Src16<BF>::inf) a &= 0x0000ffffu;
    }
    acc = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, acc), __builtin_bit_cast(us2, a)));
  }
  return acc;
}

// maximum of both halves over the 2^lpr_log2 lanes of a row, for NB rows at once so that their exchanges overlap (all 64
// lanes call this)
template <int NB>
__device__ __forceinline__ void row_reduce(uint32_t (&m)[NB], unsigned lpr) {
#pragma unroll
  for (int b = 0; b < NB; ++b) m[b] = (m[b] & 0xffffu) > (m[b] >> 16) ? (m[b] & 0xffffu) : (m[b] >> 16);
  for (unsigned off = 1; off < lpr; off <<= 1) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const uint32_t o = (uint32_t)__shfl_xor((int)m[b], (int)off);
      m[b] = o > m[b] ? o : m[b];
    }
  }
}

}  // namespace sm
