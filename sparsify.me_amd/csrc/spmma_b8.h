// spmma_b8.h -- the 1-byte 2:4 path, shared by the int8 (spmma_i8.hip) and OCP fp8 (spmma_fp8.hip) entry points:
// prune STRIP / TILE, check, compress, decompress and the pipelined matmul, each written once over a small element
// kind (how a byte orders, what counts as zero, its TILE magnitude) and, for the matmul, the matrix instruction with
// its accumulator and epilogue.  Blob geometry (include/sparsifyme.h) with 1-byte elements: values [kc/64][M][32 B],
// metadata [kc/64][M][8 B].
// Operand maps of the 1-byte sparse instructions, determined on hardware for v_smfmac_i32_16x16x128_i8
// (tools/archive/probe_i8.hip -> profiles/probe_i8_r01.txt); v_smfmac_f32_16x16x128_{fp8,bf8}_{fp8,bf8} take the same
// operand registers and share them (tests/test_gpu_fp8.py: exact products over every format pair):
//   A lane l: row l & 15, g = l >> 4: 16 kept bytes = strips 8 g .. 8 g + 7 of the 128-k stage (dense k 32 g .. + 31),
//     2-bit position code of kept byte e in bits [2 e, 2 e + 1] of the index operand -- i.e. the blob's nibbles of
//     those 8 strips, 4 consecutive metadata bytes, as they are;
//   B lane l: column l & 15, G = l >> 4: bytes 0-15 = dense k 16 G .. 16 G + 15, bytes 16-31 = dense k 64 + 16 G .. + 15;
//   D lane l, register q: row 4 (l >> 4) + q, column l & 15 (the fp16 SMFMAC's map).
// Stage = 128 k = two 64-k planes of the blob: A values image [BM][64 B] (plane 0 | plane 1 per row: lane g's chunk is
// chunk g), metadata [2][BM][8 B], B image [BN][128 B]; all by global_load_lds, ring of 2, one barrier per stage.
// Three A modes: STAGED (the blob's values and metadata), FUSED (the dense tile [BM][128 B], selected in registers) and
// DENSE (the same dense tile fed whole to the dense instruction, MmaI8Dense / MmaF8Dense: the dense GEMM).
#pragma once
#include "select24.h"
#include "mma_tile.h"

namespace sm {

static __device__ __attribute__((aligned(256))) const unsigned char sm_zero_page_b8[256] = {0};

// ---------------------------------------------------------------------------------------------
// element kinds: key4 = the per-byte selection key of four bytes at once (no carry ever leaves a byte), key / mag /
// nz of one byte
// ---------------------------------------------------------------------------------------------
// int8: |x| of a signed byte (|-128| = 128 > 127)
struct ElemI8 {
  static __device__ __forceinline__ uint32_t key4(uint32_t d) {
    // flip the negative bytes and add their sign bit (0x80 -> 0x7f + 1 = 0x80)
    const uint32_t sgn = (d >> 7) & 0x01010101u;
    return (d ^ (sgn * 0xffu)) + sgn;
  }
  static __device__ __forceinline__ uint32_t key(uint8_t v) {
    const int x = (int)(int8_t)v;
    return (uint32_t)(x < 0 ? -x : x);  // 0 .. 128
  }
  static __device__ __forceinline__ float mag(uint8_t v) { return (float)key(v); }
  static __device__ __forceinline__ bool nz(uint8_t v) { return v != 0; }
};

// OCP fp8 (SM_FP8_E4M3 / SM_FP8_E5M2): the fp16 rules on the exact fp16 image.  Sign-magnitude, monotone encodings: the
// key is bits & 0x7f, i.e. the high byte of the image's bits & 0x7fff, with the one difference the conversion makes --
// an e5m2 NaN is quieted (0x7d -> 0x7f00, 0x7e -> 0x7e00, 0x7f -> 0x7f00), so its key gets the quiet bit too.  e4m3 has
// one NaN (0x7f, above every finite 0x00 .. 0x7e).  Zero is (v & 0x7f) == 0, so -0 (0x80) is zero and NaN is not.
template <int FMT>
struct ElemF8 {
  static __device__ __forceinline__ uint32_t key4(uint32_t d) {
    uint32_t a = d & 0x7f7f7f7fu;
    if constexpr (FMT == SM_FP8_E5M2) a |= ((a + 0x03030303u) >> 6) & 0x02020202u;  // bytes 0x7d .. 0x7f: set 0x02
    return a;
  }
  static __device__ __forceinline__ uint32_t key(uint8_t v) { return key4(v) & 0xffu; }
  // TILE magnitude: |x| as fp32, exact; NaN (and e5m2 inf) -> inf, as the fp16 rule's mag_of does
  static __device__ __forceinline__ float mag(uint8_t v) {
    const uint32_t a = v & 0x7fu;
    if constexpr (FMT == SM_FP8_E5M2) {
      if (a >= 0x7cu) return __builtin_inff();
      return (float)__builtin_bit_cast(_Float16, (uint16_t)(a << 8));
    } else {
      if (a == 0x7fu) return __builtin_inff();
      const uint32_t e = a >> 3, mt = a & 7u;
      // subnormal m * 2^-9, normal (8 + m) * 2^(e - 10): one exponent shift of an exact small integer
      return e == 0 ? (float)mt * 0x1p-9f : __builtin_ldexpf((float)(8u + mt), (int)e - 10);
    }
  }
  static __device__ __forceinline__ bool nz(uint8_t v) { return (v & 0x7fu) != 0; }
};

// One strip (four bytes in a dword) in the composite-key form of select24.h: key_i = key(x_i) << 2 | (3 - i) --
// distinct, larger = kept earlier, equal keys ordered by the lower index -- the two largest by a max / min / med
// chain, their low two bits name the kept positions, one v_perm_b32 pulls the two kept bytes out in position order.
//   d = {x3:x2:x1:x0}  ->  kept = {x[p1]:x[p0]} in the low 16 bits,  nib = p0 | p1 << 2  (p0 < p1)
template <class E>
__device__ __forceinline__ void strip_select_b8(uint32_t d, uint32_t& kept, uint32_t& nib) {
  const uint32_t ab = E::key4(d);
  uint32_t K[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) K[i] = (((ab >> (8 * i)) & 0xffu) << 2) | (uint32_t)(3 - i);
  const uint32_t m01 = K[0] > K[1] ? K[0] : K[1], n01 = K[0] > K[1] ? K[1] : K[0];
  const uint32_t m = m01 > K[2] ? m01 : K[2];
  const uint32_t c01 = m01 < K[2] ? m01 : K[2];
  const uint32_t med = n01 > c01 ? n01 : c01;
  const uint32_t first = m > K[3] ? m : K[3], lo = m > K[3] ? K[3] : m;
  const uint32_t second = lo > med ? lo : med;
  const uint32_t a = first & 3u, b = second & 3u;
  const uint32_t A = a > b ? a : b, B = a > b ? b : a;  // p0 = 3 - A < p1 = 3 - B
  const uint32_t sel = 0x0c0c0000u | ((3u - B) << 8) | (3u - A);
  kept = __builtin_amdgcn_perm(0u, d, sel);
  nib = 15u - (A | (B << 2));
}

// item = 16 dense k of one row (4 strips): one 16-byte load (when aligned) -> 8 kept bytes + 2 metadata bytes
struct B8Item {
  uint8_t e[16];
};
__device__ __forceinline__ void load_item_b8(B8Item& v, const uint8_t* p, size_t nvalid, bool vec) {
  if (vec && nvalid >= 16) {
    *reinterpret_cast<u4*>(v.e) = *reinterpret_cast<const u4*>(p);
  } else {
#pragma unroll
    for (unsigned t = 0; t < 16; ++t) v.e[t] = t < nvalid ? p[t] : (uint8_t)0;
  }
}

template <class E>
__global__ __launch_bounds__(256) void prune_strip_b8_kernel(const uint8_t* A_in, uint8_t* A_out, size_t m, size_t k, size_t ld, bool vec) {
  const size_t ipr = (k + 15) / 16, total = m * ipr;
  for (size_t it = blockIdx.x * (size_t)256 + threadIdx.x; it < total; it += (size_t)gridDim.x * 256) {
    const size_t row = it / ipr, c = (it - row * ipr) * 16;
    const size_t nvalid = k - c < 16 ? k - c : 16;
    __attribute__((aligned(16))) B8Item v;
    load_item_b8(v, A_in + row * ld + c, nvalid, vec);
#pragma unroll
    for (unsigned s = 0; s < 4; ++s) {
      const unsigned keep = strip_keepmask(E::key(v.e[4 * s]), E::key(v.e[4 * s + 1]), E::key(v.e[4 * s + 2]), E::key(v.e[4 * s + 3]));
#pragma unroll
      for (unsigned t = 0; t < 4; ++t)
        if (!((keep >> t) & 1u)) v.e[4 * s + t] = 0;
    }
    uint8_t* dst = A_out + row * ld + c;
    if (vec && nvalid >= 16) {
      *reinterpret_cast<u4*>(dst) = *reinterpret_cast<const u4*>(v.e);
    } else {
#pragma unroll
      for (unsigned t = 0; t < 16; ++t)
        if (t < nvalid) dst[t] = v.e[t];
    }
  }
}

// TILE rule (the variant the reference's spmma asks for, spmma.hxx:86): one 4 x 4 tile per thread, magnitudes as fp32
// (exact), the frozen candidate order of select24.h: tile_keepmask.
template <class E>
__global__ __launch_bounds__(256) void prune_tile_b8_kernel(const uint8_t* A_in, uint8_t* A_out, size_t m, size_t k, size_t ld, bool vec) {
  const size_t tpr = (k + 3) / 4, trows = (m + 3) / 4, total = tpr * trows;
  for (size_t it = blockIdx.x * (size_t)256 + threadIdx.x; it < total; it += (size_t)gridDim.x * 256) {
    const size_t tr = it / tpr, tc = it - tr * tpr, r0 = tr * 4, c0 = tc * 4;
    const unsigned ncol = k - c0 < 4 ? (unsigned)(k - c0) : 4u;
    uint8_t v[4][4];
    float mag[4][4];
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      const bool rv = r0 + r < m;
      const uint8_t* p = A_in + (r0 + r) * ld + c0;
      if (rv && vec && ncol == 4) {
        const uint32_t d = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (unsigned t = 0; t < 4; ++t) v[r][t] = (uint8_t)(d >> (8 * t));
      } else {
#pragma unroll
        for (unsigned t = 0; t < 4; ++t) v[r][t] = (rv && t < ncol) ? p[t] : (uint8_t)0;
      }
#pragma unroll
      for (unsigned t = 0; t < 4; ++t) mag[r][t] = E::mag(v[r][t]);
    }
    const unsigned keep = tile_keepmask(mag);
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      if (r0 + r >= m) continue;
      uint8_t* p = A_out + (r0 + r) * ld + c0;
#pragma unroll
      for (unsigned t = 0; t < 4; ++t)
        if (t < ncol) p[t] = ((keep >> (4 * r + t)) & 1u) ? v[r][t] : (uint8_t)0;
    }
  }
}

template <class E>
__global__ __launch_bounds__(256) void prune_check_b8_kernel(const uint8_t* A, size_t m, size_t k, size_t ld, bool vec, int* d_valid) {
  const size_t ipr = (k + 15) / 16, total = m * ipr;
  bool bad = false;
  for (size_t it = blockIdx.x * (size_t)256 + threadIdx.x; it < total; it += (size_t)gridDim.x * 256) {
    const size_t row = it / ipr, c = (it - row * ipr) * 16;
    __attribute__((aligned(16))) B8Item v;
    load_item_b8(v, A + row * ld + c, k - c < 16 ? k - c : 16, vec);
#pragma unroll
    for (unsigned s = 0; s < 4; ++s) {
      unsigned nnz = 0;
#pragma unroll
      for (unsigned t = 0; t < 4; ++t) nnz += E::nz(v.e[4 * s + t]) ? 1u : 0u;
      bad |= nnz > 2;
    }
  }
  if (__any(bad)) {
    if ((threadIdx.x & 63) == 0) raise_flag(d_valid);
  }
}

// Items (16 dense k of one row -> 8 kept bytes + 2 metadata bytes) are walked so that a row's 128 input bytes of a PAIR
// of planes are read by 8 consecutive lanes (whole cache lines; walking plane by plane reads every line twice, half
// each time: 2.3-2.9 TB/s) -- item it = ((pair * M + R) * 8 + j8): plane 2 pair + j8 / 4, quarter j8 % 4.  The writes
// are then runs of 32 B of values and 8 B of metadata per row and plane, consecutive rows adjacent.
template <class E>
__global__ __launch_bounds__(256) void compress_b8_kernel(const uint8_t* A, size_t m, size_t k, size_t ld, size_t strideA, size_t kc,
                                                         size_t M, uint8_t* vals, unsigned char* meta, bool vec) {
  // blockIdx.y = plane pair, so that no item needs a 64-bit division; contiguous batches (strideA == m * ld) are one
  // tall matrix and need none for the row either
  const size_t nplanes = kc / 64, total = M * 8, sp = blockIdx.y;
  const bool tall = strideA == m * ld;
  for (size_t it = blockIdx.x * (size_t)256 + threadIdx.x; it < total; it += (size_t)gridDim.x * 256) {
    const size_t R = it >> 3, j8 = it & 7, s = 2 * sp + (j8 >> 2), c = s * 64 + (j8 & 3) * 16;
    if (s >= nplanes) continue;  // odd plane count: the last pair has one plane
    const size_t o = (s * M + R) * 4 + (j8 & 3);  // output item: 8 value bytes at 8 o, 2 metadata bytes at 2 o
    __attribute__((aligned(8))) uint8_t out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned mb = 0x4444u;  // padding strips: positions (0, 1)
    if (c < k) {
      const uint8_t* src = A + R * ld + c;
      if (!tall) {
        const size_t b = R / m, i = R - b * m;
        src = A + b * strideA + i * ld + c;
      }
      __attribute__((aligned(16))) B8Item v;
      load_item_b8(v, src, k - c < 16 ? k - c : 16, vec);
      mb = 0;
      const u4 d4 = *reinterpret_cast<const u4*>(v.e);
      uint32_t kp[4];
#pragma unroll
      for (unsigned st = 0; st < 4; ++st) {
        uint32_t nib;
        strip_select_b8<E>(d4[st], kp[st], nib);  // a strip at or beyond k is all zeros here: keeps (0, 1), nibble 0x4
        mb |= nib << (4 * st);
      }
      *reinterpret_cast<u2*>(out) = u2{kp[0] | (kp[1] << 16), kp[2] | (kp[3] << 16)};
    }
    *reinterpret_cast<u2*>(vals + o * 8) = *reinterpret_cast<const u2*>(out);
    *reinterpret_cast<unsigned short*>(meta + o * 2) = (unsigned short)mb;
  }
}

// the inverse moves bytes only: one kernel for every element kind
static __global__ __launch_bounds__(256) void decompress_b8_kernel(const uint8_t* vals, const unsigned char* meta, size_t m, size_t k, size_t ld,
                                                           size_t strideA, size_t kc, size_t M, uint8_t* A) {
  const size_t total = M * (kc / 16);
  for (size_t it = blockIdx.x * (size_t)256 + threadIdx.x; it < total; it += (size_t)gridDim.x * 256) {
    const size_t t4 = it >> 2, s = t4 / M, R = t4 - s * M, c = s * 64 + (it & 3) * 16;
    if (c >= k) continue;
    const size_t b = R / m, i = R - b * m;
    const unsigned mb = *reinterpret_cast<const unsigned short*>(meta + it * 2);
    uint8_t* dst = A + b * strideA + i * ld + c;
#pragma unroll
    for (unsigned st = 0; st < 4; ++st) {
      const unsigned nib = (mb >> (4 * st)) & 0xfu, p0 = nib & 3u, p1 = nib >> 2;
#pragma unroll
      for (unsigned t = 0; t < 4; ++t)
        if (c + 4 * st + t < k) dst[4 * st + t] = t == p0 ? vals[it * 8 + 2 * st] : (t == p1 ? vals[it * 8 + 2 * st + 1] : (uint8_t)0);
    }
  }
}

// host side of the streaming kernels: the launches every 1-byte entry point shares (arguments already validated)
template <class E>
inline int launch_prune24_b8(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, int alg, hipStream_t st) {
  if (alg == SM_PRUNE_TILE) {
    const bool vec4 = (reinterpret_cast<uintptr_t>(A_in) & 3u) == 0 && (reinterpret_cast<uintptr_t>(A_out) & 3u) == 0 && ld % 4 == 0;
    prune_tile_b8_kernel<E><<<stream_grid(ceil_div(m, (size_t)4) * ceil_div(k, (size_t)4), 256), 256, 0, st>>>(
        (const uint8_t*)A_in, (uint8_t*)A_out, m, k, ld, vec4);
    return check_launch("prune_tile_b8_kernel");
  }
  const bool vec = aligned16(A_in) && aligned16(A_out) && ld % 16 == 0;
  prune_strip_b8_kernel<E><<<stream_grid(m * ceil_div(k, (size_t)16), 256), 256, 0, st>>>((const uint8_t*)A_in, (uint8_t*)A_out, m, k, ld, vec);
  return check_launch("prune_strip_b8_kernel");
}

template <class E>
inline int launch_prune24_check_b8(const void* A, size_t m, size_t k, size_t ld, int* d_valid, hipStream_t st) {
  if (hipMemsetAsync(d_valid, 0, sizeof(int), st) != hipSuccess) return check_launch("hipMemsetAsync");
  if (m == 0 || k == 0) return SM_STATUS_SUCCESS;
  prune_check_b8_kernel<E><<<stream_grid(m * ceil_div(k, (size_t)16), 256), 256, 0, st>>>((const uint8_t*)A, m, k, ld,
                                                                                       aligned16(A) && ld % 16 == 0, d_valid);
  return check_launch("prune_check_b8_kernel");
}

// compress after validation (A, blob non-null, ld >= k, blob 16-byte aligned); `what` names the entry point in errors
template <class E>
inline int launch_compress24_b8(const void* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* blob, hipStream_t st,
                                const char* what) {
  const BlobLayout L = blob_layout(m, k, 1, batch);
  if (L.M == 0 || k == 0) return SM_STATUS_SUCCESS;
  if ((L.kc / 64 + 1) / 2 > 65535) {
    set_error("%s: k too large", what);
    return SM_STATUS_NOT_SUPPORTED;
  }
  const size_t vbytes = L.M * (L.kc / 2), mbytes = L.M * (L.kc / 8);
  if (L.meta_off > vbytes && hipMemsetAsync((char*)blob + vbytes, 0, L.meta_off - vbytes, st) != hipSuccess) return check_launch("hipMemsetAsync");
  if (L.total > L.meta_off + mbytes && hipMemsetAsync((char*)blob + L.meta_off + mbytes, 0, L.total - L.meta_off - mbytes, st) != hipSuccess)
    return check_launch("hipMemsetAsync");
  const bool vec = aligned16(A) && ld % 16 == 0 && strideA % 16 == 0;
  compress_b8_kernel<E><<<dim3(stream_grid(L.M * 8, 256), (unsigned)((L.kc / 64 + 1) / 2)), 256, 0, st>>>(
      (const uint8_t*)A, m, k, ld, strideA, L.kc, L.M, (uint8_t*)blob, (unsigned char*)blob + L.meta_off, vec);
  return check_launch("compress_b8_kernel");
}

static inline int launch_decompress24_b8(const void* blob, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* A, hipStream_t st) {
  const BlobLayout L = blob_layout(m, k, 1, batch);
  if (L.M == 0 || k == 0) return SM_STATUS_SUCCESS;
  decompress_b8_kernel<<<stream_grid(L.M * (L.kc / 16), 256), 256, 0, st>>>((const uint8_t*)blob, (const unsigned char*)blob + L.meta_off, m, k, ld,
                                                                            strideA, L.kc, L.M, (uint8_t*)A);
  return check_launch("decompress_b8_kernel");
}

// ---------------------------------------------------------------------------------------------
// matmul
// ---------------------------------------------------------------------------------------------
struct Spmma8Args {
  const char* vals;
  const char* meta;
  size_t Mtot;
  const uint8_t* Ad;  // fused form: the DENSE A (row-major, lda), selected in the consumer's registers
  size_t sA;          //   its batch stride (elements)
  int lda;
  const uint8_t* B;  // [n][k] per batch, ldb = k
  // int8: int32 output C, or the requantised output C8 = sat_int8(rne(scale * acc)); accumulate: C += acc
  int* C;
  int8_t* C8;
  float scale;
  int accumulate;
  // fp8: Cf (out_type SM_OUT_F32 / F16 / BF16) = alpha * row_scale[i] * acc + beta * Cf; row_scale NULL: 1
  void* Cf;
  const float* row_scale;
  float alpha, beta;
  int out_type;
  size_t sB, sC;  // batch strides (elements)
  int m, Mrows, N, K, batch, tiles_m, tiles_n, nplanes;
};

typedef int i4v __attribute__((ext_vector_type(4)));
typedef int i8v __attribute__((ext_vector_type(8)));

// the matrix instruction of an element kind: Elem = A's kind (the fused form's selection), acc_t, mma; kDense: the
// dense instruction of the same kind (A's fragment is 32 dense bytes, no index operand)
struct MmaI8 {
  using Elem = ElemI8;
  using acc_t = i4v;
  static constexpr bool kFloat = false, kDense = false;
  static __device__ __forceinline__ i4v mma(i4v a, i8v b, i4v c, int idx) { return __builtin_amdgcn_smfmac_i32_16x16x128_i8(a, b, c, idx, 0, 0); }
};
template <int FA, int FB>
struct MmaF8 {
  using Elem = ElemF8<FA>;
  using acc_t = f4;
  static constexpr bool kFloat = true, kDense = false;
  static __device__ __forceinline__ f4 mma(i4v a, i8v b, f4 c, int idx) {
    if constexpr (FA == SM_FP8_E4M3 && FB == SM_FP8_E4M3) return __builtin_amdgcn_smfmac_f32_16x16x128_fp8_fp8(a, b, c, idx, 0, 0);
    else if constexpr (FA == SM_FP8_E4M3) return __builtin_amdgcn_smfmac_f32_16x16x128_fp8_bf8(a, b, c, idx, 0, 0);
    else if constexpr (FB == SM_FP8_E4M3) return __builtin_amdgcn_smfmac_f32_16x16x128_bf8_fp8(a, b, c, idx, 0, 0);
    else return __builtin_amdgcn_smfmac_f32_16x16x128_bf8_bf8(a, b, c, idx, 0, 0);
  }
};

// Dense forms.  A's fragment is read from a dense [rows][128 B] image exactly as B's is (frag_b8: chunks g and 4 + g), so A
// and B share one k-to-lane map and every product pairs the right k whatever order the instruction sums in.
//   int8: two v_mfma_i32_16x16x64_i8, one per 64-k half of the stage (bytes 0-15: k 16 g .., bytes 16-31: k 64 + 16 g ..).
//   fp8: v_mfma_f32_16x16x128_f8f6f4 with cbsz / blgp = A's / B's format (0 = e4m3, 1 = e5m2, as SM_FP8_*) -- the
//   full-rate dense fp8 instruction; literal-0 scale operands select its unscaled encoding (scale 1: exact products
//   in tests/test_gpu_dense8.py).
struct MmaI8Dense {
  using Elem = ElemI8;
  using acc_t = i4v;
  static constexpr bool kFloat = false, kDense = true;
  static __device__ __forceinline__ i4v mma(i8v a, i8v b, i4v c) {
    c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a.lo, b.lo, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a.hi, b.hi, c, 0, 0, 0);
  }
};
template <int FA, int FB>
struct MmaF8Dense {
  static_assert(SM_FP8_E4M3 == 0 && SM_FP8_E5M2 == 1, "SM_FP8_* are the f8f6f4 format codes");
  using Elem = ElemF8<FA>;
  using acc_t = f4;
  static constexpr bool kFloat = true, kDense = true;
  static __device__ __forceinline__ f4 mma(i8v a, i8v b, f4 c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, 0, 0, 0, 0);
  }
};

// one lane's 32 operand bytes of row `row` of a [rows][128 B] stage image (a_off swizzle): chunks g and 4 + g
__device__ __forceinline__ i8v frag_b8(const char* img, unsigned row, unsigned g) {
  const u4 lo = *reinterpret_cast<const u4*>(img + a_off(row, g));
  const u4 hi = *reinterpret_cast<const u4*>(img + a_off(row, 4u + g));
  return i8v{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// fp8 epilogue of one output type: v = (alpha * row_scale[i]) * acc (+ beta * C), one rounding to the output type.
// The accumulators were staged in the LDS image (4-byte words, CP bytes per row) when vec; otherwise they come from acc.
template <int OT>
struct OutElt;
template <>
struct OutElt<SM_OUT_F32> {
  typedef float T;
  static __device__ __forceinline__ float load(const float* p) { return *p; }
  static __device__ __forceinline__ float conv(float v) { return v; }
};
template <>
struct OutElt<SM_OUT_F16> {
  typedef _Float16 T;
  static __device__ __forceinline__ float load(const _Float16* p) { return (float)*p; }
  static __device__ __forceinline__ _Float16 conv(float v) { return (_Float16)v; }
};
template <>
struct OutElt<SM_OUT_BF16> {
  typedef __bf16 T;
  static __device__ __forceinline__ float load(const __bf16* p) { return (float)*p; }
  static __device__ __forceinline__ __bf16 conv(float v) { return (__bf16)v; }
};

template <int OT, int BM, int BN, int TM, int TN, int FM, int FN, int NT>
__device__ __forceinline__ void store_c_f8(const Spmma8Args& p, char* smem, const f4 (&acc)[FM][FN], unsigned b, unsigned wm, unsigned wn, int m0,
                                           int n0, unsigned tid) {
  typedef typename OutElt<OT>::T T;
  constexpr int CP = BN * 4 + 16;
  const unsigned lane = tid & 63u, g = lane >> 4, r = lane & 15u;
  T* C = reinterpret_cast<T*>(p.Cf) + (size_t)b * p.sC;
  const bool tall = p.Mrows > p.m;
  auto rscale = [&](int gr) -> float {  // alpha * row_scale of global row gr
    if (!p.row_scale) return p.alpha;
    return p.alpha * p.row_scale[tall ? gr % p.m : gr];
  };
  const bool c_vec = (p.N % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & (4 * sizeof(T) - 1)) == 0);
  if (c_vec) {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const unsigned row = wm * TM + i * 16 + 4u * g, col = wn * TN + j * 16 + r;
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<float*>(smem + (row + q) * CP + col * 4) = acc[i][j][q];
      }
    __syncthreads();
    constexpr int NCH = BM * (BN / 4);
    for (unsigned q = tid; q < (unsigned)NCH; q += (unsigned)NT) {
      const unsigned row = q / (BN / 4), cn = q % (BN / 4);
      const int gr = m0 + (int)row, gc = n0 + 4 * (int)cn;
      if (gr >= p.Mrows || gc >= p.N) continue;  // N % 4 == 0: a chunk is all in or all out
      const f4 a = *reinterpret_cast<const f4*>(smem + row * CP + cn * 16);
      const float s = rscale(gr);
      T* dst = C + (size_t)gr * p.N + gc;
      T o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = s * a[e];
        if (p.beta != 0.0f) v += p.beta * OutElt<OT>::load(dst + e);
        o[e] = OutElt<OT>::conv(v);
      }
      if constexpr (sizeof(T) == 4) __builtin_nontemporal_store(*reinterpret_cast<const u4*>(o), reinterpret_cast<u4*>(dst));
      else __builtin_nontemporal_store(*reinterpret_cast<const u2*>(o), reinterpret_cast<u2*>(dst));
    }
  } else {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int gc = n0 + (int)(wn * TN + j * 16 + r);
        if (gc >= p.N) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int gr = m0 + (int)(wm * TM + i * 16 + 4u * g) + q;
          if (gr >= p.Mrows) continue;
          T* dst = C + (size_t)gr * p.N + gc;
          float v = rscale(gr) * acc[i][j][q];
          if (p.beta != 0.0f) v += p.beta * OutElt<OT>::load(dst);
          *dst = OutElt<OT>::conv(v);
        }
      }
  }
}

// FUSED: prune + compress + matmul in one kernel, the 1-byte counterpart of spmma_f16_fused_direct_kernel: the stage's A
// image is the DENSE tile [BM][128 B] (128 k), no metadata, and the lane that feeds the matrix instruction selects its
// 8 strips (dense k 32 g .. 32 g + 31 = chunks 2 g, 2 g + 1 of its row) in registers: the same kept bytes and codes as
// the compress kernel would have stored, so the result is bit-identical to compress + spmma; no blob exists.
// DENSE (MM::kDense, FUSED false): the same dense tile, fed whole (frag_b8) to the dense instruction: C = A . B.
template <class MM, int BN, int WM, int WN, bool FUSED = false>
__global__ __launch_bounds__(64 * WM * WN) void spmma_b8_kernel(const Spmma8Args p) {
  using E = typename MM::Elem;
  using acc_t = typename MM::acc_t;
  constexpr bool DENSE = MM::kDense, DA = FUSED || DENSE;  // DA: the stage holds the dense A tile
  static_assert(!(FUSED && DENSE), "the dense instruction takes the dense tile as it is");
  constexpr int BM = 128, NW = WM * WN, TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  constexpr int SA = DA ? BM * 128 : BM * 64, SM_ = DA ? 0 : 2 * BM * 8, SB = BN * 128, STAGE = SA + SM_ + SB;
  constexpr int A_N = DA ? BM / 8 : BM / 16, M_N = DA ? 0 : 2, B_N = BN / 8, W = A_N + M_N + B_N;  // 1 KiB DMA wave-instructions per stage
  constexpr int SL = (W + NW - 1) / NW;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const unsigned tid = threadIdx.x, lane = tid & 63u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned wm = wave / WN, wn = wave % WN;
  const unsigned tiles = (unsigned)p.tiles_m * (unsigned)p.tiles_n;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned b = lid / tiles, trem = lid - b * tiles;
  const unsigned tile_m = trem / (unsigned)p.tiles_n, tile_n = trem - tile_m * (unsigned)p.tiles_n;
  const int m0 = (int)tile_m * BM, n0 = (int)tile_n * BN;
  const size_t row_base = (size_t)b * p.m;
  const uint8_t* B = p.B + (size_t)b * p.sB;
  const int mlast = p.Mrows - 1, nlast = p.N - 1;
  const int nkt = (p.nplanes + 1) / 2;
  const bool odd = (p.nplanes & 1) != 0;  // the last stage then has one plane: its second half meets zeros

  // per slot: source of stage 0, per-stage step, LDS offset, and whether it belongs to the stage's second plane / half
  const char* src[SL];
  size_t step[SL];
  unsigned loff[SL];
  bool second[SL];
#pragma unroll
  for (int i = 0; i < SL; ++i) {
    const unsigned t = wave + (unsigned)NW * i;
    src[i] = nullptr; step[i] = 0; loff[i] = 0; second[i] = false;
    if (DA && t < (unsigned)A_N) {  // 8 rows x 128 B of the dense A
      const unsigned row = 8u * t + (lane >> 3), cs = (lane & 7u) ^ (row & 7u);
      int gr = m0 + (int)row;
      gr = gr < mlast ? gr : mlast;
      src[i] = reinterpret_cast<const char*>(p.Ad + (size_t)b * p.sA + (size_t)gr * p.lda) + 16u * cs;
      step[i] = 128;
      loff[i] = t * 1024u;
      second[i] = cs >= 4u;  // k 64 .. 127 of the stage
    } else if (t < (unsigned)A_N) {  // 16 rows x 64 B of kept values: lane -> row 16 t + lane / 4, LDS chunk lane % 4
      const unsigned row = 16u * t + (lane >> 2), cs = (lane & 3u) ^ a64_swz(row);  // source chunk: plane cs >> 1, half cs & 1
      int gr = m0 + (int)row;
      gr = gr < mlast ? gr : mlast;
      src[i] = p.vals + ((size_t)(cs >> 1) * p.Mtot + row_base + (size_t)gr) * 32 + 16u * (cs & 1u);
      step[i] = 2 * p.Mtot * 32;
      loff[i] = t * 1024u;
      second[i] = (cs >> 1) != 0;  // per lane
    } else if (t < (unsigned)(A_N + M_N)) {  // metadata of plane pl: lane -> rows 2 lane, 2 lane + 1
      const unsigned pl = t - A_N;
      int gr = m0 + 2 * (int)lane;
      gr = gr < mlast ? gr : (mlast & ~1);
      src[i] = p.meta + ((size_t)pl * p.Mtot + row_base + (size_t)gr) * 8;
      step[i] = 2 * p.Mtot * 8;
      loff[i] = SA + pl * (BM * 8);
      second[i] = pl != 0;
    } else if (t < (unsigned)W) {  // B: 8 columns x 128 B (k-contiguous)
      const unsigned j = t - A_N - M_N, col = 8u * j + (lane >> 3), cs = (lane & 7u) ^ (col & 7u);
      int gn = n0 + (int)col;
      gn = gn < nlast ? gn : nlast;
      src[i] = reinterpret_cast<const char*>(B + (size_t)gn * p.K) + 16u * cs;
      step[i] = 128;
      loff[i] = SA + SM_ + j * 1024u;
      second[i] = cs >= 4u;
    }
  }
  auto stage = [&](int kt, int buf) {
    char* base = smem + buf * STAGE;
    const bool tail = odd && kt == nkt - 1;
#pragma unroll
    for (int i = 0; i < SL; ++i) {
      const unsigned t = wave + (unsigned)NW * i;  // wave-uniform
      if (t >= (unsigned)W) continue;
      const char* g = src[i] + (size_t)kt * step[i];
      // one-plane tail: the absent plane's values and metadata come from a zero page, and B's k 64 .. 127 (past the end
      // of the column) from the same page -- 0 x 0 = 0 in integers and in fp8 alike
      if (tail && second[i]) g = reinterpret_cast<const char*>(sm_zero_page_b8) + 16u * (lane & 7u);
      __builtin_amdgcn_global_load_lds((gptr_t*)g, (lptr_t*)(base + loff[i]), 16, 0, 0);
    }
  };

  acc_t acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = acc_t{0, 0, 0, 0};

  if (nkt > 0) stage(0, 0);
  const unsigned g = lane >> 4, r = lane & 15u;
  for (int kt = 0; kt < nkt; ++kt) {
    wait_dma_and_barrier<0>();  // ring of 2: nothing newer than this stage is in flight
    if (kt + 1 < nkt) stage(kt + 1, (kt + 1) & 1);
    const char* As = smem + (kt & 1) * STAGE;
    const char* Ms = As + SA;
    const char* Bs = Ms + SM_;
    i4v af[FM];
    int idx[FM];
    i8v ad[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const unsigned row = wm * TM + i * 16 + r;
      if constexpr (DENSE) {
        ad[i] = frag_b8(As, row, g);
        continue;
      }
      if constexpr (FUSED) {
        const u4 lo = *reinterpret_cast<const u4*>(As + a_off(row, 2u * g));
        const u4 hi = *reinterpret_cast<const u4*>(As + a_off(row, 2u * g + 1u));
        uint32_t kp[8], nb[8];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          strip_select_b8<E>(lo[t], kp[t], nb[t]);
          strip_select_b8<E>(hi[t], kp[4 + t], nb[4 + t]);
        }
        af[i] = i4v{(int)(kp[0] | (kp[1] << 16)), (int)(kp[2] | (kp[3] << 16)), (int)(kp[4] | (kp[5] << 16)), (int)(kp[6] | (kp[7] << 16))};
        idx[i] = (int)(nb[0] | (nb[1] << 4) | (nb[2] << 8) | (nb[3] << 12) | (nb[4] << 16) | (nb[5] << 20) | (nb[6] << 24) | (nb[7] << 28));
        continue;
      }
      af[i] = *reinterpret_cast<const i4v*>(As + row * 64u + 16u * (g ^ a64_swz(row)));
      idx[i] = *reinterpret_cast<const int*>(Ms + (g >> 1) * (BM * 8) + row * 8u + 4u * (g & 1u));
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const i8v bf = frag_b8(Bs, wn * TN + j * 16 + r, g);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if constexpr (DENSE) acc[i][j] = MM::mma(ad[i], bf, acc[i][j]);
        else acc[i][j] = MM::mma(af[i], bf, acc[i][j], idx[i]);
      }
    }
  }
  __syncthreads();

  // ---- epilogue: a lane holds 4 consecutive ROWS of one column; transpose through LDS, store 16-byte row pieces
  if constexpr (MM::kFloat) {
    if (p.out_type == SM_OUT_F32) store_c_f8<SM_OUT_F32, BM, BN, TM, TN, FM, FN, 64 * NW>(p, smem, acc, b, wm, wn, m0, n0, tid);
    else if (p.out_type == SM_OUT_F16) store_c_f8<SM_OUT_F16, BM, BN, TM, TN, FM, FN, 64 * NW>(p, smem, acc, b, wm, wn, m0, n0, tid);
    else store_c_f8<SM_OUT_BF16, BM, BN, TM, TN, FM, FN, 64 * NW>(p, smem, acc, b, wm, wn, m0, n0, tid);
    return;
  } else {
    int* C = p.C ? p.C + (size_t)b * p.sC : nullptr;
    int8_t* C8 = p.C8 ? p.C8 + (size_t)b * p.sC : nullptr;
    constexpr int CP = BN * 4 + 16;  // bytes per row of the image
    auto quant = [&](int a) -> int {   // sat_int8(rne(scale * acc)): one fp32 multiply, round to nearest even, clamp
      float f = __builtin_rintf(p.scale * (float)a);
      f = f < -128.0f ? -128.0f : (f > 127.0f ? 127.0f : f);
      return (int)f;
    };
    if (C8) {
      const bool q_vec = (p.N % 16 == 0) && ((reinterpret_cast<uintptr_t>(C8) & 15u) == 0);
      if (q_vec) {
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            const unsigned row = wm * TM + i * 16 + 4u * g, col = wn * TN + j * 16 + r;
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<int*>(smem + (row + q) * CP + col * 4) = acc[i][j][q];
          }
        __syncthreads();
        constexpr int NCH = BM * (BN / 16);
        for (unsigned q = tid; q < (unsigned)NCH; q += 64u * NW) {
          const unsigned row = q / (BN / 16), cn = q % (BN / 16);
          const int gr = m0 + (int)row, gc = n0 + 16 * (int)cn;
          if (gr >= p.Mrows || gc >= p.N) continue;  // N % 16 == 0: a chunk is all in or all out
          u4 o;
#pragma unroll
          for (int w4 = 0; w4 < 4; ++w4) {
            const i4v v = *reinterpret_cast<const i4v*>(smem + row * CP + cn * 64 + w4 * 16);
            o[w4] = (unsigned)(quant(v[0]) & 0xff) | ((unsigned)(quant(v[1]) & 0xff) << 8) | ((unsigned)(quant(v[2]) & 0xff) << 16) |
                    ((unsigned)(quant(v[3]) & 0xff) << 24);
          }
          __builtin_nontemporal_store(o, reinterpret_cast<u4*>(C8 + (size_t)gr * p.N + gc));
        }
      } else {
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) {
            const int gc = n0 + (int)(wn * TN + j * 16 + r);
            if (gc >= p.N) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int gr = m0 + (int)(wm * TM + i * 16 + 4u * g) + q;
              if (gr < p.Mrows) C8[(size_t)gr * p.N + gc] = (int8_t)quant(acc[i][j][q]);
            }
          }
      }
      return;
    }
    const bool c_vec = (p.N % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & 15u) == 0);
    if (c_vec) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const unsigned row = wm * TM + i * 16 + 4u * g, col = wn * TN + j * 16 + r;
#pragma unroll
          for (int q = 0; q < 4; ++q) *reinterpret_cast<int*>(smem + (row + q) * CP + col * 4) = acc[i][j][q];
        }
      __syncthreads();
      constexpr int NCH = BM * (BN / 4);
      for (unsigned q = tid; q < (unsigned)NCH; q += 64u * NW) {
        const unsigned row = q / (BN / 4), cn = q % (BN / 4);
        const int gr = m0 + (int)row, gc = n0 + 4 * (int)cn;
        if (gr >= p.Mrows || gc >= p.N) continue;
        i4v v = *reinterpret_cast<const i4v*>(smem + row * CP + cn * 16);
        int* dst = C + (size_t)gr * p.N + gc;
        if (p.accumulate) {
          const i4v old = *reinterpret_cast<const i4v*>(dst);
          v += old;
        }
        __builtin_nontemporal_store(v, reinterpret_cast<i4v*>(dst));
      }
    } else {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int gc = n0 + (int)(wn * TN + j * 16 + r);
          if (gc >= p.N) continue;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int gr = m0 + (int)(wm * TM + i * 16 + 4u * g) + q;
            if (gr >= p.Mrows) continue;
            int* dst = C + (size_t)gr * p.N + gc;
            *dst = p.accumulate ? *dst + acc[i][j][q] : acc[i][j][q];
          }
        }
    }
  }
}

template <class MM, int BN, int WM, int WN, bool FUSED = false>
static int launch_spmma_b8(const Spmma8Args& a0, hipStream_t st, const char* what) {
  Spmma8Args a = a0;
  a.tiles_m = (a.Mrows + 127) / 128;
  a.tiles_n = (a.N + BN - 1) / BN;
  const size_t nwg = (size_t)a.tiles_m * a.tiles_n * a.batch;
  constexpr size_t lds_main = 2 * ((FUSED || MM::kDense ? (size_t)128 * 128 : (size_t)128 * 64 + 2 * 128 * 8) + (size_t)BN * 128);
  constexpr size_t lds_epi = (size_t)128 * (BN * 4 + 16);
  constexpr size_t lds = lds_main > lds_epi ? lds_main : lds_epi;
  return launch_grid<&spmma_b8_kernel<MM, BN, WM, WN, FUSED>>(nwg, 64 * WM * WN, lds, lds, st, what, "spmma_b8_kernel", a);
}

}  // namespace sm
