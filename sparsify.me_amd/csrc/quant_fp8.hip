// quant_fp8.hip -- the front of the fp8 2:4 route: per-row quantisation of a 16-bit (fp16 / bf16) row-major A to OCP fp8
// (e4m3 / e5m2), dense (sm_quantize_rows_fp8_*) or fused with the STRIP selection and the blob write
// (sm_quantize_compress24_fp8_*: A is read once, no dense fp8 A exists), and the small weight operand's per-tensor
// quantisation + transpose (sm_quantize_transpose_fp8_*).
//   The rule (include/sparsifyme.h):  amax = max(max |a| over the finite elements of the row, 2^-100),
//   row_scale = amax / FMAX, inv = FMAX / amax (two correctly rounded fp32 divisions),  q = rne_fmt(fp32(a) * inv).
//   |fp32(a) * inv| <= FMAX (1 + 2^-23), which rounds to FMAX: a finite row never overflows.  NaN -> 0x7f, +-inf -> 0x7f
//   (e4m3) / 0x7c | sign (e5m2), by an explicit select on the SOURCE bits; they do not enter amax.
//   The row maximum is needed before the first byte is written, so the row is held on chip: 2^L lanes (8 .. 64) own a
//   row, a lane holds 8 elements (one 16-byte load) of every 8 * 2^L-element chunk, up to QMAXCH chunks (k <= 4608: 36
//   VGPRs), the maximum is reduced over the row's lanes on the magnitude BITS (integer maximum, exact), then the lane
//   converts, selects and stores from registers.  A workgroup (4 waves) owns 16 * 64 / 2^L consecutive rows; the blob
//   items of the block are staged in LDS in blob order and leave as 16-byte (values) / 8-byte (metadata) stores that
//   form one contiguous run per 64-k plane.  Longer rows take the same kernel with NCHMAX = 0: the second pass
//   re-reads the row (it is in L2 / Infinity Cache) and writes from the lanes; same bytes, no speed target.
#include "quant_fp8.h"
#include "spmma_b8.h"

using namespace sm;

namespace {

constexpr int QMAXCH = 9;  // chunks a lane holds: 9 x 512 = 4608 elements at 64 lanes per row

// (the fp8 rule itself -- Src16, quant4, mag_max8, row_reduce -- is in quant_fp8.h, shared with rmsnorm.hip)

struct QuantArgs {
  const uint16_t* A;
  size_t lda;
  uint8_t* Q;  // dense form
  size_t ldq;
  uint8_t* vals;  // compress form: the blob's sections, M = rows
  uint8_t* meta;
  float* row_scale;
  unsigned rows, k, lpr_log2, nch;
  unsigned gap, tail;  // compress form: bytes between the values and the 256-byte aligned metadata section, and after the metadata
  bool qvec;           // 8-byte stores into Q are aligned
};

// 8 elements of a row at column col: one 16-byte load, or per element where the row ends inside them (zeros beyond k)
__device__ __forceinline__ u4 load8(const uint16_t* row, unsigned col, unsigned k, bool valid) {
  u4 d = {0u, 0u, 0u, 0u};
  if (!valid || col >= k) return d;
  if (col + 8u <= k) return *reinterpret_cast<const u4*>(row + col);
#pragma unroll
  for (unsigned t = 0; t < 8; ++t)
    if (col + t < k) d[t >> 1] |= (uint32_t)row[col + t] << (16u * (t & 1u));
  return d;
}

// NCHMAX: the chunks of a row a lane may hold, 2, 4 or QMAXCH; a wave makes 4 passes of 64 / 2^L rows and holds PB = 4, 2 or 1
// of them at once, so that at least 4 KiB of loads per wave are in flight before the first maximum is reduced (with one pass
// at a time the short rows ran at a third of the copy rate: latency, not bytes).  NCHMAX = 0: the re-reading form.
template <bool BF, int FMT, bool COMPRESS, int NCHMAX>
__global__ __launch_bounds__(256) void quant_rows_kernel(const QuantArgs p) {
  using E = ElemF8<FMT>;
  constexpr bool HOLD = NCHMAX > 0;
  constexpr int PB = NCHMAX == 0 ? 1 : (NCHMAX <= 2 ? 4 : (NCHMAX <= 4 ? 2 : 1)), NV = HOLD ? NCHMAX : 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned lpr = 1u << p.lpr_log2, rpp = 64u >> p.lpr_log2, l = lane & (lpr - 1u), rs = lane >> p.lpr_log2;
  const unsigned br = 16u * rpp;  // rows of the block: every wave makes 4 passes of rpp rows
  const size_t row0 = (size_t)blockIdx.x * br;
  const unsigned nplanes = p.k / 64u;
  const unsigned ps = br * 32u + 32u;  // LDS plane stride of the values: the 32 spare bytes spread the planes over the banks
  char* lmeta = smem + (size_t)nplanes * ps;

  if constexpr (COMPRESS) {
    // the gap and the tail are zero in the blob sm_compress24_fp8 writes (each below 256 bytes, a multiple of 8): written here,
    // so that the entry point is one kernel node and nothing else
    if (blockIdx.x == 0 && tid < 32u) {
      if (8u * tid < p.gap) *reinterpret_cast<u2*>(p.vals + (size_t)p.rows * nplanes * 32u + 8u * tid) = u2{0u, 0u};
      if (8u * tid < p.tail) *reinterpret_cast<u2*>(p.meta + (size_t)p.rows * nplanes * 8u + 8u * tid) = u2{0u, 0u};
    }
  }

  for (unsigned pass0 = 0; pass0 < 4; pass0 += PB) {
    unsigned rb[PB];
    bool valid[PB];
    const uint16_t* src[PB];
    u4 v[PB][NV];
    uint32_t mx[PB];
#pragma unroll
    for (int b = 0; b < PB; ++b) {
      rb[b] = (4u * (pass0 + b) + wave) * rpp + rs;
      valid[b] = row0 + rb[b] < p.rows;
      src[b] = p.A + (row0 + rb[b]) * p.lda;
      mx[b] = 0;
    }
    if constexpr (HOLD) {
#pragma unroll
      for (int b = 0; b < PB; ++b)
#pragma unroll
        for (unsigned c = 0; c < (unsigned)NV; ++c)
          if (c < p.nch) v[b][c] = load8(src[b], (c * lpr + l) * 8u, p.k, valid[b]);
#pragma unroll
      for (int b = 0; b < PB; ++b)
#pragma unroll
        for (unsigned c = 0; c < (unsigned)NV; ++c)
          if (c < p.nch) mx[b] = mag_max8<BF, false>(mx[b], v[b][c]);
    } else {
      for (unsigned c = 0; c < p.nch; ++c) mx[0] = mag_max8<BF, false>(mx[0], load8(src[0], (c * lpr + l) * 8u, p.k, valid[0]));
    }
    row_reduce<PB>(mx, lpr);

#pragma unroll
    for (int b = 0; b < PB; ++b) {
      const size_t R = row0 + rb[b];
      const bool fix = mx[b] >= Src16<BF>::inf;  // the row holds a NaN or an infinity: they do not enter amax
      if (fix) {  // uniform over the row's lanes
        uint32_t fin[1] = {0};
        if constexpr (HOLD) {
#pragma unroll
          for (unsigned c = 0; c < (unsigned)NV; ++c)
            if (c < p.nch) fin[0] = mag_max8<BF, true>(fin[0], v[b][c]);
        } else {
          for (unsigned c = 0; c < p.nch; ++c) fin[0] = mag_max8<BF, true>(fin[0], load8(src[b], (c * lpr + l) * 8u, p.k, valid[b]));
        }
        row_reduce<1>(fin, lpr);
        mx[b] = fin[0];
      }
      const float amax = __builtin_fmaxf(Src16<BF>::f32(mx[b]), 0x1p-100f);
      const float scale = amax / F8Lim<FMT>::fmax, inv = F8Lim<FMT>::fmax / amax;
      if (valid[b] && l == 0) p.row_scale[R] = scale;

      auto emit = [&](unsigned c, const u4& d) {
        const unsigned col = (c * lpr + l) * 8u;
        if (!valid[b] || col >= p.k) return;
        const uint32_t q0 = quant4<BF, FMT, false>(d[0], d[1], inv, fix), q1 = quant4<BF, FMT, false>(d[2], d[3], inv, fix);
        if constexpr (!COMPRESS) {
          uint8_t* dst = p.Q + R * p.ldq + col;
          if (p.qvec && col + 8u <= p.k) {
            *reinterpret_cast<u2*>(dst) = u2{q0, q1};
          } else {
#pragma unroll
            for (unsigned t = 0; t < 8; ++t)
              if (col + t < p.k) dst[t] = (uint8_t)((t < 4 ? q0 : q1) >> (8u * (t & 3u)));
          }
        } else {
          uint32_t k0, k1, n0, n1;
          strip_select_b8<E>(q0, k0, n0);
          strip_select_b8<E>(q1, k1, n1);
          const uint32_t kept = k0 | (k1 << 16), mb = n0 | (n1 << 4);
          const unsigned s = col >> 6, j = (col >> 3) & 7u;  // plane, eighth of the plane: 4 value bytes + 1 metadata byte
          if constexpr (HOLD) {
            *reinterpret_cast<uint32_t*>(smem + (size_t)s * ps + rb[b] * 32u + 4u * j) = kept;
            *reinterpret_cast<uint8_t*>(lmeta + ((size_t)s * br + rb[b]) * 8u + j) = (uint8_t)mb;
          } else {
            *reinterpret_cast<uint32_t*>(p.vals + ((size_t)s * p.rows + R) * 32u + 4u * j) = kept;
            p.meta[((size_t)s * p.rows + R) * 8u + j] = (uint8_t)mb;
          }
        }
      };
      if constexpr (HOLD) {
#pragma unroll
        for (unsigned c = 0; c < (unsigned)NV; ++c)
          if (c < p.nch) emit(c, v[b][c]);
      } else {
        for (unsigned c = 0; c < p.nch; ++c) emit(c, load8(src[b], (c * lpr + l) * 8u, p.k, valid[b]));
      }
    }
  }

  if constexpr (COMPRESS && HOLD) {
    __syncthreads();
    // per plane the block's items are one run in the blob: br * 32 B of values, br * 8 B of metadata
    const unsigned vper = br * 2u, nv = nplanes * vper;
    for (unsigned i = tid; i < nv; i += 256u) {
      const unsigned s = i / vper, q = i - s * vper;
      if (row0 + (q >> 1) >= p.rows) continue;
      *reinterpret_cast<u4*>(p.vals + ((size_t)s * p.rows + row0) * 32u + q * 16u) = *reinterpret_cast<const u4*>(smem + (size_t)s * ps + q * 16u);
    }
    const unsigned nm = nplanes * br;
    for (unsigned i = tid; i < nm; i += 256u) {
      const unsigned s = i / br, q = i - s * br;
      if (row0 + q >= p.rows) continue;
      *reinterpret_cast<u2*>(p.meta + ((size_t)s * p.rows + row0 + q) * 8u) = *reinterpret_cast<const u2*>(lmeta + (size_t)i * 8u);
    }
  }
}

template <bool BF, int FMT, bool COMPRESS>
int launch_quant_rows(QuantArgs a, hipStream_t st) {
  // lanes per row: the smallest power of two in 8 .. 64 that covers the row with one chunk, 64 beyond 512 elements
  unsigned L = 3;
  while (L < 6 && (size_t)(8u << L) < a.k) ++L;
  a.lpr_log2 = L;
  a.nch = (unsigned)ceil_div(a.k, (size_t)(8u << L));
  const unsigned br = 16u * (64u >> L);
  const unsigned grid = (unsigned)ceil_div((size_t)a.rows, (size_t)br);
  const size_t lds = COMPRESS && a.nch <= (unsigned)QMAXCH ? (size_t)(a.k / 64u) * (br * 32u + 32u + br * 8u) : 0;  // <= 72 planes x 672 B
  if (a.nch <= 2) quant_rows_kernel<BF, FMT, COMPRESS, 2><<<grid, 256, lds, st>>>(a);
  else if (a.nch <= 4) quant_rows_kernel<BF, FMT, COMPRESS, 4><<<grid, 256, lds, st>>>(a);
  else if (a.nch <= (unsigned)QMAXCH) quant_rows_kernel<BF, FMT, COMPRESS, QMAXCH><<<grid, 256, lds, st>>>(a);
  else quant_rows_kernel<BF, FMT, COMPRESS, 0><<<grid, 256, 0, st>>>(a);
  return check_launch("quant_rows_kernel");
}

template <bool COMPRESS>
int dispatch_quant_rows(const QuantArgs& a, bool bf, int fmt, hipStream_t st) {
  if (bf) return fmt == SM_FP8_E4M3 ? launch_quant_rows<true, SM_FP8_E4M3, COMPRESS>(a, st) : launch_quant_rows<true, SM_FP8_E5M2, COMPRESS>(a, st);
  return fmt == SM_FP8_E4M3 ? launch_quant_rows<false, SM_FP8_E4M3, COMPRESS>(a, st) : launch_quant_rows<false, SM_FP8_E5M2, COMPRESS>(a, st);
}

// rows of A as 16-byte pieces, every dimension below 2^31
bool rows_supported(const void* A, size_t rows, size_t k, size_t lda, const char* what) {
  if (rows > 0x7fffffffull || k > 0x7fffffffull || lda > 0x7fffffffull) {
    set_error("%s: dimension exceeds 2^31-1", what);
    return false;
  }
  if (!aligned16(A) || lda % 8 != 0) {
    set_error("%s: needs 16-byte aligned rows of A (pointer, lda %% 8 == 0)", what);
    return false;
  }
  return true;
}

int quantize_rows(const void* A, size_t rows, size_t k, size_t lda, void* Q, size_t ldq, float* row_scale, int fmt, bool bf, hipStream_t st) {
  const char* what = bf ? "sm_quantize_rows_fp8_bf16" : "sm_quantize_rows_fp8_f16";
  if (!A || !Q || !row_scale || !fmt_ok(fmt) || lda < k || ldq < k) {
    set_error("%s: invalid argument (fmt SM_FP8_*, lda >= k, ldq >= k)", what);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!rows_supported(A, rows, k, lda, what)) return SM_STATUS_NOT_SUPPORTED;
  if (ldq > 0x7fffffffull) {
    set_error("%s: dimension exceeds 2^31-1", what);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (rows == 0 || k == 0) return SM_STATUS_SUCCESS;
  QuantArgs a = {};
  a.A = (const uint16_t*)A; a.lda = lda; a.Q = (uint8_t*)Q; a.ldq = ldq; a.row_scale = row_scale;
  a.rows = (unsigned)rows; a.k = (unsigned)k;
  a.qvec = (reinterpret_cast<uintptr_t>(Q) & 7u) == 0 && ldq % 8 == 0;
  return dispatch_quant_rows<false>(a, bf, fmt, st);
}

int quantize_compress(const void* A, size_t rows, size_t k, size_t lda, void* blob, float* row_scale, int fmt, bool bf, hipStream_t st) {
  const char* what = bf ? "sm_quantize_compress24_fp8_bf16" : "sm_quantize_compress24_fp8_f16";
  if (!A || !blob || !row_scale || !fmt_ok(fmt) || lda < k || !aligned16(blob)) {
    set_error("%s: invalid argument (fmt SM_FP8_*, lda >= k, blob 16-byte aligned)", what);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!rows_supported(A, rows, k, lda, what)) return SM_STATUS_NOT_SUPPORTED;
  if (k % 64 != 0) {
    set_error("%s: needs k %% 64 == 0 (use sm_quantize_rows_fp8 + sm_compress24_fp8)", what);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (rows == 0 || k == 0) return SM_STATUS_SUCCESS;
  const BlobLayout L = blob_layout(rows, k, 1, 1);
  QuantArgs a = {};
  // the gap before the 256-byte aligned metadata section and the tail, zero as sm_compress24_fp8 leaves them
  a.gap = (unsigned)(L.meta_off - L.M * (L.kc / 2));
  a.tail = (unsigned)(L.total - L.meta_off - L.M * (L.kc / 8));
  a.A = (const uint16_t*)A; a.lda = lda; a.vals = (uint8_t*)blob; a.meta = (uint8_t*)blob + L.meta_off; a.row_scale = row_scale;
  a.rows = (unsigned)rows; a.k = (unsigned)k;
  return dispatch_quant_rows<true>(a, bf, fmt, st);
}

// B (k x n, row-major, ldb) -> Bt [n][k] fp8: 64 x 64 tiles through LDS (+ 4 bytes per row against bank conflicts)
template <bool BF, int FMT>
__global__ __launch_bounds__(256) void quant_transpose_kernel(const uint16_t* B, unsigned k, unsigned n, size_t ldb, float inv, uint8_t* Bt, bool vec) {
  __shared__ __attribute__((aligned(4))) uint8_t tile[64][68];  // [n][k]
  const unsigned tid = threadIdx.x, n0 = blockIdx.x * 64u, k0 = blockIdx.y * 64u;
  const unsigned c = tid & 63u;
  for (unsigned r = tid >> 6; r < 64u; r += 4u) {
    uint32_t h = 0;
    if (k0 + r < k && n0 + c < n) h = B[(size_t)(k0 + r) * ldb + n0 + c];
    tile[c][r] = (uint8_t)quant4<BF, FMT, true>(h, 0u, inv, (h & 0x7fffu) >= Src16<BF>::inf);
  }
  __syncthreads();
  const unsigned q = tid & 15u;  // 4 k of a row of Bt
  for (unsigned r = tid >> 4; r < 64u; r += 16u) {
    if (n0 + r >= n || k0 + 4u * q >= k) continue;
    uint8_t* dst = Bt + (size_t)(n0 + r) * k + k0 + 4u * q;
    if (vec) {  // k % 4 == 0: the four are all inside
      *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(&tile[r][4u * q]);
    } else {
#pragma unroll
      for (unsigned t = 0; t < 4; ++t)
        if (k0 + 4u * q + t < k) dst[t] = tile[r][4u * q + t];
    }
  }
}

int quantize_transpose(const void* B, size_t k, size_t n, size_t ldb, float inv_scale, void* Bt, int fmt, bool bf, hipStream_t st) {
  const char* what = bf ? "sm_quantize_transpose_fp8_bf16" : "sm_quantize_transpose_fp8_f16";
  if (!B || !Bt || !fmt_ok(fmt) || ldb < n) {
    set_error("%s: invalid argument (fmt SM_FP8_*, ldb >= n)", what);
    return SM_STATUS_INVALID_VALUE;
  }
  if (k > 0x7fffffffull || n > 0x7fffffffull || ldb > 0x7fffffffull || ceil_div(k, (size_t)64) > 65535) {
    set_error("%s: dimension too large", what);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (k == 0 || n == 0) return SM_STATUS_SUCCESS;
  const dim3 grid((unsigned)ceil_div(n, (size_t)64), (unsigned)ceil_div(k, (size_t)64));
  const bool vec = (reinterpret_cast<uintptr_t>(Bt) & 3u) == 0 && k % 4 == 0;
  const uint16_t* b = (const uint16_t*)B;
  uint8_t* o = (uint8_t*)Bt;
  if (bf) {
    if (fmt == SM_FP8_E4M3) quant_transpose_kernel<true, SM_FP8_E4M3><<<grid, 256, 0, st>>>(b, (unsigned)k, (unsigned)n, ldb, inv_scale, o, vec);
    else quant_transpose_kernel<true, SM_FP8_E5M2><<<grid, 256, 0, st>>>(b, (unsigned)k, (unsigned)n, ldb, inv_scale, o, vec);
  } else {
    if (fmt == SM_FP8_E4M3) quant_transpose_kernel<false, SM_FP8_E4M3><<<grid, 256, 0, st>>>(b, (unsigned)k, (unsigned)n, ldb, inv_scale, o, vec);
    else quant_transpose_kernel<false, SM_FP8_E5M2><<<grid, 256, 0, st>>>(b, (unsigned)k, (unsigned)n, ldb, inv_scale, o, vec);
  }
  return check_launch("quant_transpose_kernel");
}

}  // namespace

extern "C" {

int sm_quantize_rows_fp8_f16(const void* A, size_t rows, size_t k, size_t lda, void* Q, size_t ldq, float* row_scale, int fmt, sm_stream_t s) {
  return quantize_rows(A, rows, k, lda, Q, ldq, row_scale, fmt, false, (hipStream_t)s);
}
int sm_quantize_rows_fp8_bf16(const void* A, size_t rows, size_t k, size_t lda, void* Q, size_t ldq, float* row_scale, int fmt, sm_stream_t s) {
  return quantize_rows(A, rows, k, lda, Q, ldq, row_scale, fmt, true, (hipStream_t)s);
}
int sm_quantize_compress24_fp8_f16(const void* A, size_t rows, size_t k, size_t lda, void* blob, float* row_scale, int fmt, sm_stream_t s) {
  return quantize_compress(A, rows, k, lda, blob, row_scale, fmt, false, (hipStream_t)s);
}
int sm_quantize_compress24_fp8_bf16(const void* A, size_t rows, size_t k, size_t lda, void* blob, float* row_scale, int fmt, sm_stream_t s) {
  return quantize_compress(A, rows, k, lda, blob, row_scale, fmt, true, (hipStream_t)s);
}
int sm_quantize_transpose_fp8_f16(const void* B, size_t k, size_t n, size_t ldb, float inv_scale, void* Bt, int fmt, sm_stream_t s) {
  return quantize_transpose(B, k, n, ldb, inv_scale, Bt, fmt, false, (hipStream_t)s);
}
int sm_quantize_transpose_fp8_bf16(const void* B, size_t k, size_t n, size_t ldb, float inv_scale, void* Bt, int fmt, sm_stream_t s) {
  return quantize_transpose(B, k, n, ldb, inv_scale, Bt, fmt, true, (hipStream_t)s);
}

}  // extern "C"
