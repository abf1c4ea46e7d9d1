// rope_common.h -- what the RoPE + append over the 16-bit cache (rope_append.hip) and over the fp8 cache (rope_append_kv8.hip) share: the
// style predicate and the rotation of one pair, stated once so that both write the same Qo and Ko bits.
#pragma once
#include "sm_common.h"

namespace sm {

inline bool ra_style_ok(int s) { return s == SM_ROPE_NEOX || s == SM_ROPE_INTERLEAVED; }

#ifdef __HIPCC__
// (y_a, y_b) of the definition in fp32: two products, each rounded, then the subtraction / the addition -- never an fma
__device__ __forceinline__ void ra_rot(float xa, float xb, float c, float s, float& ya, float& yb) {
#pragma clang fp contract(off)
  const float ac = xa * c, bs = xb * s, bc = xb * c, as = xa * s;
  ya = ac - bs;
  yb = bc + as;
}
#endif

}  // namespace sm
