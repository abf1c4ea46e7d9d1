// rmsnorm.hip -- sm_rmsnorm_{f16,bf16} (extension): the pre-norm of a decoder layer in one launch, h = H + D, n = rmsnorm(h) * gamma,
// with the updated residual stream, the 16-bit normalised row and / or its per-row fp8 quantisation (the rule of quant_fp8.hip, from
// quant_fp8.h) as outputs.  The definition (include/sparsifyme.h) is fp32 to the operation; only the order of the sum of squares is the
// kernel's, fixed per `hidden`.
//
// A row is read once and held in registers as its ROUNDED 16-bit h, 8 elements (one 16-byte access) per lane and chunk, and every
// stage works on those registers in place:
//   add     h = rne16(fp32(H) + fp32(D)) per element; stored to res_out from the registers.  Every load of H and D is issued before
//           the first store (the allowed aliasings N == D, N == H rest on it).
//   sum     two fma chains per lane (even / odd element of a dword) in ascending chunk order, added; then over the row's lanes by
//           xor-butterfly steps (every lane ends with the same bits: a + b == b + a), and in the BLOCK form over the four waves
//           through LDS, (w0 + w1) + (w2 + w3).
//   scale   r = 1 / sqrtf(S / hidden + eps): the division, the add, sqrtf and the division are separate, correctly rounded operations
//           (hipcc's default for `/` and sqrtf; __fsqrt_rn is NOT used: without OCML_BASIC_ROUNDED_OPERATIONS the toolchain's header
//           maps it to the native approximation).
//   norm    n = rne16((fp32(h) * r) * fp32(gamma)) overwrites h in the registers; stored to N.
//   quant   amax over the magnitude bits of n (integer maximum, exact), the two divisions, q = rne_fmt(fp32(n) * inv) with the
//           non-finite bytes patched: quant_rows_kernel's steps on the same register layout, so Q / row_scale are what
//           sm_quantize_rows_fp8_* gives on N byte for byte.
// Two geometries share that body (rms_rows):
//   LANES   2^L lanes (8 .. 64) of one wave own a row, the least power of two that covers it with one chunk; a wave works on
//           PB = 4 / 2 / 1 groups of 64 / 2^L rows at once (NCHMAX = 2 / 4 / 9 chunks per lane) so that short rows keep 4 KiB of loads
//           in flight per wave, as quant_rows_kernel does -- or on one group when the call has few rows.  No LDS, no barrier: a wave
//           past the last row leaves at once.  The library's threshold keeps LANES to rows of at most two chunks; the larger
//           instantiations exist for the build that times both forms (tools/probes/rmsnorm_forced.hip).
//   BLOCK   the 256 threads of a workgroup own a row: up to 8 chunks of 2048 elements; three LDS exchanges of four words (sum, amax bits,
//           finite amax bits: a slot each, so one barrier per exchange).
// The form is a function of `hidden` alone and so is the lane that owns an element: a row's bits do not depend on its neighbours.
#include "quant_fp8.h"

namespace sm {

// tools/rmsnorm_table.py builds this file alone with both extremes to time LANES against BLOCK on the same shapes
#ifndef RMSNORM_LANES_MAX
#define RMSNORM_LANES_MAX SM_RMSNORM_LANES_MAX_HIDDEN
#endif
constexpr int RMS_LANES_NCH = 9;  // chunks a lane may hold in the LANES form: 9 x 512 = 4608 elements (36 VGPRs), the quantiser's budget
constexpr unsigned RMS_FEW_WAVES = 2048;  // LANES: up to this many waves (8 per CU of 256) a wave takes one group of rows, not PB
constexpr int RMS_BLOCK_NCH = 8;  // chunks a thread may hold in the BLOCK form: 8 x 2048 = SM_RMSNORM_MAX_HIDDEN
static_assert(RMSNORM_LANES_MAX <= 512 * RMS_LANES_NCH && RMSNORM_LANES_MAX % 8 == 0, "the LANES form holds at most 9 chunks of 512");
static_assert(SM_RMSNORM_MAX_HIDDEN == 2048 * RMS_BLOCK_NCH, "the BLOCK form holds 8 chunks of 2048");

inline int rmsnorm_form(size_t hidden) {
  if (hidden > SM_RMSNORM_MAX_HIDDEN || hidden % 8 != 0) return SM_RMSNORM_FORM_INVALID;
  if (hidden == 0) return SM_RMSNORM_FORM_EMPTY;
  return hidden <= RMSNORM_LANES_MAX ? SM_RMSNORM_FORM_LANES : SM_RMSNORM_FORM_BLOCK;
}

struct RmsArgs {
  const uint16_t *H, *D, *gamma;  // D, gamma: or null
  uint16_t *res, *N;              // or null
  uint8_t* Q;                     // with row_scale, or both null
  float* row_scale;
  size_t ldh, ldd, ldn, ldq;
  unsigned tokens, hidden, lpr_log2, nch;
  float eps;
  int fmt;
  bool qvec;  // 8-byte stores into Q are aligned
};

// fp32 -> the bits of the 16-bit type, round to nearest even
template <bool BF>
__device__ __forceinline__ uint32_t rms_round(float x) {
  if constexpr (BF) return (uint32_t)__builtin_bit_cast(unsigned short, (__bf16)x);  // v_cvt_pk_bf16_f32
  else return (uint32_t)__builtin_bit_cast(unsigned short, (_Float16)x);
}
// rne16(fp32(a) + fp32(b)) on both halves of a dword
template <bool BF>
__device__ __forceinline__ uint32_t rms_add2(uint32_t a, uint32_t b) {
  const float lo = Src16<BF>::f32(a & 0xffffu) + Src16<BF>::f32(b & 0xffffu), hi = Src16<BF>::f32(a >> 16) + Src16<BF>::f32(b >> 16);
  return rms_round<BF>(lo) | (rms_round<BF>(hi) << 16);
}
// rne16((fp32(h) * r) * fp32(g)) on both halves of a dword; GAMMA false: one multiply
template <bool BF, bool GAMMA>
__device__ __forceinline__ uint32_t rms_norm2(uint32_t h, float r, uint32_t g) {
  float lo = Src16<BF>::f32(h & 0xffffu) * r, hi = Src16<BF>::f32(h >> 16) * r;
  if constexpr (GAMMA) {
    lo = lo * Src16<BF>::f32(g & 0xffffu);
    hi = hi * Src16<BF>::f32(g >> 16);
  }
  // fp16: the product is made opaque before it is rounded.  Left alone, the multiply and the conversion are selected as one
  // v_fma_mixlo_f16 with a +0 addend, and (-0) + (+0) = +0: a zero product lost its sign (h = 0 under a negative gamma, r = 0 under a
  // negative h), where the definition's two IEEE multiplies keep it.
  if constexpr (!BF) asm volatile("" : "+v"(lo), "+v"(hi));
  return rms_round<BF>(lo) | (rms_round<BF>(hi) << 16);
}

// The LANES geometry: lane l of the 2^L lanes of a row holds elements (c 2^L + l) 8 .. + 7 of chunk c.
struct RmsLanes {
  unsigned lpr, l;
  __device__ __forceinline__ unsigned col(unsigned c) const { return (c * lpr + l) * 8u; }
  template <int PB>
  __device__ __forceinline__ void sum(float (&s)[PB]) const {
    for (unsigned off = 1; off < lpr; off <<= 1) {
#pragma unroll
      for (int b = 0; b < PB; ++b) s[b] = s[b] + __shfl_xor(s[b], (int)off);
    }
  }
  template <int PB>
  __device__ __forceinline__ void max_bits(uint32_t (&m)[PB], int) const { row_reduce<PB>(m, lpr); }
  __device__ __forceinline__ bool leader() const { return l == 0; }
};

// The BLOCK geometry: thread t of the 256 holds elements (c 256 + t) 8 .. + 7 of chunk c; lds: 12 words.
struct RmsBlock {
  unsigned tid;
  uint32_t* lds;
  __device__ __forceinline__ unsigned col(unsigned c) const { return (c * 256u + tid) * 8u; }
  __device__ __forceinline__ void sum(float (&s)[1]) const {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) s[0] = s[0] + __shfl_xor(s[0], off);
    if ((tid & 63u) == 0) lds[tid >> 6] = __builtin_bit_cast(uint32_t, s[0]);
    __syncthreads();
    s[0] = (__builtin_bit_cast(float, lds[0]) + __builtin_bit_cast(float, lds[1])) + (__builtin_bit_cast(float, lds[2]) + __builtin_bit_cast(float, lds[3]));
  }
  // slot 1: the maximum over all elements, slot 2: over the finite ones (block-uniform call sites)
  __device__ __forceinline__ void max_bits(uint32_t (&m)[1], int slot) const {
    row_reduce<1>(m, 64u);
    uint32_t* w = lds + 4 * slot;
    if ((tid & 63u) == 0) w[tid >> 6] = m[0];
    __syncthreads();
    const uint32_t a = w[0] > w[1] ? w[0] : w[1], b = w[2] > w[3] ? w[2] : w[3];
    m[0] = a > b ? a : b;
  }
  __device__ __forceinline__ bool leader() const { return tid == 0; }
};

// 8 elements of a row at column col: one 16-byte load, zeros beyond the row or for a row that does not exist (hidden % 8 == 0: a
// chunk piece is inside or outside as a whole)
__device__ __forceinline__ u4 rms_load8(const uint16_t* row, unsigned col, unsigned hidden, bool valid) {
  if (!valid || col >= hidden) return u4{0u, 0u, 0u, 0u};
  return *reinterpret_cast<const u4*>(row + col);
}

// the fp8 output of PB rows held as n in v: quant_rows_kernel's steps
template <bool BF, int FMT, int NV, int PB, class G>
__device__ __forceinline__ void rms_quant(const RmsArgs& p, const G& g, const size_t (&R)[PB], const bool (&valid)[PB], const u4 (&v)[PB][NV]) {
  uint32_t mx[PB];
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    mx[b] = 0;
#pragma unroll
    for (unsigned c = 0; c < (unsigned)NV; ++c)
      if (c < p.nch) mx[b] = mag_max8<BF, false>(mx[b], v[b][c]);
  }
  g.max_bits(mx, 1);
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    const bool fix = mx[b] >= Src16<BF>::inf;  // the row holds a NaN or an infinity: they do not enter amax (uniform over the row's lanes)
    if (fix) {
      uint32_t fin[1] = {0};
#pragma unroll
      for (unsigned c = 0; c < (unsigned)NV; ++c)
        if (c < p.nch) fin[0] = mag_max8<BF, true>(fin[0], v[b][c]);
      if constexpr (PB == 1) g.max_bits(fin, 2);
      else row_reduce<1>(fin, g.lpr);
      mx[b] = fin[0];
    }
    const float amax = __builtin_fmaxf(Src16<BF>::f32(mx[b]), 0x1p-100f);
    const float scale = amax / F8Lim<FMT>::fmax, inv = F8Lim<FMT>::fmax / amax;
    if (valid[b] && g.leader()) p.row_scale[R[b]] = scale;
#pragma unroll
    for (unsigned c = 0; c < (unsigned)NV; ++c) {
      const unsigned col = g.col(c);
      if (c >= p.nch || !valid[b] || col >= p.hidden) continue;
      const uint32_t q0 = quant4<BF, FMT, false>(v[b][c][0], v[b][c][1], inv, fix), q1 = quant4<BF, FMT, false>(v[b][c][2], v[b][c][3], inv, fix);
      uint8_t* dst = p.Q + R[b] * p.ldq + col;
      if (p.qvec) {
        *reinterpret_cast<u2*>(dst) = u2{q0, q1};
      } else {
#pragma unroll
        for (unsigned t = 0; t < 8; ++t) dst[t] = (uint8_t)((t < 4 ? q0 : q1) >> (8u * (t & 3u)));
      }
    }
  }
}

// PB rows R[b] (valid[b]: the row exists) through the whole definition; NV: the chunks a lane may hold (p.nch <= NV of them are used)
template <bool BF, int NV, int PB, class G>
__device__ __forceinline__ void rms_rows(const RmsArgs& p, const G& g, const size_t (&R)[PB], const bool (&valid)[PB]) {
  u4 v[PB][NV];
#pragma unroll
  for (int b = 0; b < PB; ++b)
#pragma unroll
    for (unsigned c = 0; c < (unsigned)NV; ++c)
      v[b][c] = rms_load8(p.H + R[b] * p.ldh, g.col(c), p.hidden, valid[b] && c < p.nch);
  if (p.D) {
    u4 d[PB][NV];
#pragma unroll
    for (int b = 0; b < PB; ++b)
#pragma unroll
      for (unsigned c = 0; c < (unsigned)NV; ++c)
        d[b][c] = rms_load8(p.D + R[b] * p.ldd, g.col(c), p.hidden, valid[b] && c < p.nch);
    // (no `c < p.nch` around the adds: an absent chunk is 0 + 0, and one straight block lets the scheduler keep the row packed -- with a
    // branch per chunk the fp32 images of H and D were made where they were loaded, and the 8-chunk BLOCK form went past 256 VGPRs)
#pragma unroll
    for (int b = 0; b < PB; ++b)
#pragma unroll
      for (unsigned c = 0; c < (unsigned)NV; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[b][c][i] = rms_add2<BF>(v[b][c][i], d[b][c][i]);
  }
  if (p.res) {
#pragma unroll
    for (int b = 0; b < PB; ++b)
#pragma unroll
      for (unsigned c = 0; c < (unsigned)NV; ++c)
        if (c < p.nch && valid[b] && g.col(c) < p.hidden) *reinterpret_cast<u4*>(p.res + R[b] * p.ldh + g.col(c)) = v[b][c];
  }

  float s[PB];
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
    for (unsigned c = 0; c < (unsigned)NV; ++c)
      if (c < p.nch) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float x = Src16<BF>::f32(v[b][c][i] & 0xffffu), y = Src16<BF>::f32(v[b][c][i] >> 16);
          s0 = __builtin_fmaf(x, x, s0);
          s1 = __builtin_fmaf(y, y, s1);
        }
      }
    s[b] = s0 + s1;
  }
  g.sum(s);
  // the row stays PACKED across the reduction: without this the fp32 images of h made for the sum are kept for the multiplies below
  // (twice the registers for a conversion that costs one instruction; the 8-chunk BLOCK form went past 256 VGPRs)
#pragma unroll
  for (int b = 0; b < PB; ++b)
#pragma unroll
    for (unsigned c = 0; c < (unsigned)NV; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(v[b][c][i]));

  u4 gm[NV];
  if (p.gamma) {
#pragma unroll
    for (unsigned c = 0; c < (unsigned)NV; ++c)
      if (c < p.nch) gm[c] = rms_load8(p.gamma, g.col(c), p.hidden, true);
  }
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    const float ms = s[b] / (float)p.hidden;
    const float r = 1.0f / __builtin_sqrtf(ms + p.eps);
#pragma unroll
    for (unsigned c = 0; c < (unsigned)NV; ++c)
      if (c < p.nch) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[b][c][i] = p.gamma ? rms_norm2<BF, true>(v[b][c][i], r, gm[c][i]) : rms_norm2<BF, false>(v[b][c][i], r, 0u);
      }
  }
  if (p.N) {
#pragma unroll
    for (int b = 0; b < PB; ++b)
#pragma unroll
      for (unsigned c = 0; c < (unsigned)NV; ++c)
        if (c < p.nch && valid[b] && g.col(c) < p.hidden) *reinterpret_cast<u4*>(p.N + R[b] * p.ldn + g.col(c)) = v[b][c];
  }
  if (!p.Q) return;
  if (p.fmt == SM_FP8_E4M3) rms_quant<BF, SM_FP8_E4M3, NV, PB>(p, g, R, valid, v);
  else rms_quant<BF, SM_FP8_E5M2, NV, PB>(p, g, R, valid, v);
}

// NCHMAX = 2, 4, RMS_LANES_NCH: the chunks a lane may hold; a wave holds PB groups of 64 / 2^L rows at once: 4, 2, 1 when there are rows
// enough to fill the device (short rows keep 4 KiB of loads in flight per wave), 1 when there are few (see RMS_FEW_WAVES)
template <bool BF, int NCHMAX, int PB>
__global__ __launch_bounds__(256) void rmsnorm_lanes_kernel(const RmsArgs p) {
  const unsigned lane = threadIdx.x & 63u, gw = blockIdx.x * 4u + (threadIdx.x >> 6);  // (gw * PB * rpp < tokens + 4 PB rpp: no overflow)
  const unsigned rpp = 64u >> p.lpr_log2;
  const RmsLanes g = {1u << p.lpr_log2, lane & ((1u << p.lpr_log2) - 1u)};
  size_t R[PB];
  bool valid[PB];
#pragma unroll
  for (int b = 0; b < PB; ++b) {
    R[b] = ((size_t)gw * PB + b) * rpp + (lane >> p.lpr_log2);
    valid[b] = R[b] < p.tokens;
  }
  if ((size_t)gw * PB * rpp >= p.tokens) return;  // (wave-uniform; no barrier in this kernel)
  rms_rows<BF, NCHMAX, PB>(p, g, R, valid);
}

// NCHMAX = 2, 4, RMS_BLOCK_NCH: the chunks a thread may hold; blockIdx.x is the row
template <bool BF, int NCHMAX>
__global__ __launch_bounds__(256) void rmsnorm_block_kernel(const RmsArgs p) {
  __shared__ uint32_t lds[12];
  const RmsBlock g = {threadIdx.x, lds};
  const size_t R[1] = {blockIdx.x};
  const bool valid[1] = {true};
  rms_rows<BF, NCHMAX, 1>(p, g, R, valid);
}

template <bool BF>
static int rmsnorm_launch(RmsArgs a, hipStream_t st) {
  if (rmsnorm_form(a.hidden) == SM_RMSNORM_FORM_LANES) {
    unsigned L = 3;  // lanes per row: the smallest power of two in 8 .. 64 that covers the row with one chunk, 64 beyond 512 elements
    while (L < 6 && (8u << L) < a.hidden) ++L;
    a.lpr_log2 = L;
    a.nch = (unsigned)ceil_div(a.hidden, (size_t)(8u << L));
    // Few rows: one group per wave.  With PB groups a wave issues PB times the instructions, and below a device's worth of waves that
    // stream, not bytes, is the call's time (16 rows of 256: 4.7 us at PB = 4 against 2.7 us for the same row in a workgroup of its
    // own).  Which lane owns an element does not depend on PB: the same bits either way.
    const unsigned rpp = 64u >> L;
    const bool few = ceil_div((size_t)a.tokens, (size_t)rpp) <= RMS_FEW_WAVES;
    const unsigned pb = few ? 1 : (a.nch <= 2 ? 4 : (a.nch <= 4 ? 2 : 1));
    const dim3 grid((unsigned)ceil_div((size_t)a.tokens, (size_t)4 * pb * rpp));
    if (a.nch <= 2) {
      if (few) rmsnorm_lanes_kernel<BF, 2, 1><<<grid, 256, 0, st>>>(a);
      else rmsnorm_lanes_kernel<BF, 2, 4><<<grid, 256, 0, st>>>(a);
    }
    if constexpr (RMSNORM_LANES_MAX > 1024) {  // (rows past two chunks: only in a build with the threshold moved up)
      if (a.nch > 2 && a.nch <= 4) {
        if (few) rmsnorm_lanes_kernel<BF, 4, 1><<<grid, 256, 0, st>>>(a);
        else rmsnorm_lanes_kernel<BF, 4, 2><<<grid, 256, 0, st>>>(a);
      } else if (a.nch > 4) {
        rmsnorm_lanes_kernel<BF, RMS_LANES_NCH, 1><<<grid, 256, 0, st>>>(a);
      }
    }
    return check_launch("rmsnorm_lanes_kernel");
  }
  a.nch = (unsigned)ceil_div(a.hidden, (size_t)2048);
  const dim3 grid(a.tokens);
  if (a.nch <= 2) rmsnorm_block_kernel<BF, 2><<<grid, 256, 0, st>>>(a);
  else if (a.nch <= 4) rmsnorm_block_kernel<BF, 4><<<grid, 256, 0, st>>>(a);
  else rmsnorm_block_kernel<BF, RMS_BLOCK_NCH><<<grid, 256, 0, st>>>(a);
  return check_launch("rmsnorm_block_kernel");
}

template <bool BF>
static int rmsnorm(const void* H, const void* D, const void* gamma, void* res_out, void* N, void* Q, float* row_scale, size_t tokens, size_t hidden,
                   size_t ldh, size_t ldd, size_t ldn, size_t ldq, float eps, int fmt, sm_stream_t stream) {
  static const char* const who = "sm_rmsnorm_{f16,bf16}";
  if (!H || (!N && !Q) || (Q == nullptr) != (row_scale == nullptr) || (Q && !fmt_ok(fmt)) || ldh < hidden || (D && ldd < hidden) || (N && ldn < hidden) ||
      (Q && ldq < hidden) || !(eps >= 0.0f)) {
    set_error("%s: invalid argument (null H, N and Q both null, one of Q / row_scale null, fmt not SM_FP8_*, a pitch below hidden, or eps negative or NaN)",
              who);
    return SM_STATUS_INVALID_VALUE;
  }
  if ((N && N == H && ((res_out && res_out != H) || ldn != ldh)) || (N && N == D && ldn != ldd) || (res_out && res_out == D) ||
      (res_out && res_out == N && N != H)) {
    set_error("%s: invalid argument (aliasing: only res_out == H, N == D and N == H with res_out null or == H are allowed, at equal pitches)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  const size_t lim = 0x7fffffffull;
  if (tokens > lim || hidden > lim || ldh > lim || (D && ldd > lim) || (N && ldn > lim) || (Q && ldq > lim)) {
    set_error("%s: tokens, hidden or a pitch exceeds 2^31-1", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (hidden > SM_RMSNORM_MAX_HIDDEN) {
    set_error("%s: hidden exceeds SM_RMSNORM_MAX_HIDDEN (%d)", who, SM_RMSNORM_MAX_HIDDEN);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (hidden % 8 != 0) {
    set_error("%s: needs hidden %% 8 == 0", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!aligned16(H) || ldh % 8 != 0 || (D && (!aligned16(D) || ldd % 8 != 0)) || !aligned16(gamma) || !aligned16(res_out) ||
      (N && (!aligned16(N) || ldn % 8 != 0))) {
    set_error("%s: needs 16-byte aligned rows of H, D, gamma, res_out and N (pointer, pitch %% 8 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (tokens == 0 || hidden == 0) return SM_STATUS_SUCCESS;
  RmsArgs a = {};
  a.H = (const uint16_t*)H; a.D = (const uint16_t*)D; a.gamma = (const uint16_t*)gamma; a.N = (uint16_t*)N; a.Q = (uint8_t*)Q; a.row_scale = row_scale;
  // without D the stream is unchanged: res_out == H needs no store
  a.res = (D || res_out != H) ? (uint16_t*)res_out : nullptr;
  a.ldh = ldh; a.ldd = ldd; a.ldn = ldn; a.ldq = ldq;
  a.tokens = (unsigned)tokens; a.hidden = (unsigned)hidden; a.eps = eps; a.fmt = fmt;
  a.qvec = (reinterpret_cast<uintptr_t>(Q) & 7u) == 0 && ldq % 8 == 0;
  return rmsnorm_launch<BF>(a, (hipStream_t)stream);
}

}  // namespace sm

using namespace sm;

extern "C" int sm_rmsnorm_form(size_t hidden, int* form) {
  if (!form) {
    set_error("sm_rmsnorm_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = rmsnorm_form(hidden);
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_rmsnorm_f16(const void* H, const void* D, const void* gamma, void* res_out, void* N, void* Q, float* row_scale, size_t tokens, size_t hidden,
                              size_t ldh, size_t ldd, size_t ldn, size_t ldq, float eps, int fmt, sm_stream_t stream) {
  return rmsnorm<false>(H, D, gamma, res_out, N, Q, row_scale, tokens, hidden, ldh, ldd, ldn, ldq, eps, fmt, stream);
}
extern "C" int sm_rmsnorm_bf16(const void* H, const void* D, const void* gamma, void* res_out, void* N, void* Q, float* row_scale, size_t tokens, size_t hidden,
                               size_t ldh, size_t ldd, size_t ldn, size_t ldq, float eps, int fmt, sm_stream_t stream) {
  return rmsnorm<true>(H, D, gamma, res_out, N, Q, row_scale, tokens, hidden, ldh, ldd, ldn, ldq, eps, fmt, stream);
}
