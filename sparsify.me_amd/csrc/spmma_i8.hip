// spmma_i8.hip -- int8 forms of the 2:4 path (extension; SURVEY.md 8(f) rank 2: the vendor call behind
// include/sparsify.me/spmma.hxx:40-113 lists int8 among its 2:4 types, examples/libcusparse_lt/include/cusparseLt.h:164-169).
//   sm_prune24_i8 (STRIP and TILE) / sm_prune24_check_i8 / sm_compress24_i8 / sm_decompress24_i8: the fp16 rules on |x| of a
//     signed byte (|-128| = 128 > 127; ties keep the lower k index); same blob geometry with 1-byte elements: values
//     [kc/64][M][32 B], metadata [kc/64][M][8 B] (include/sparsifyme.h).
//   sm_spmma_i8: C (int32) = A_2:4 . B (+ C), exact integer arithmetic on v_smfmac_i32_16x16x128_i8.  B is given
//     K-CONTIGUOUS per output column ([n][k], "TN", the layout int8 matrix cores are fed in): a column's 128-k stage
//     piece is one 128-byte row of the LDS image and a lane's operand is two 16-byte chunks of it.
// The kernels are the 1-byte ones of spmma_b8.h over ElemI8 / MmaI8 (operand maps and stage layout described there).
#include "spmma_b8.h"

namespace sm {

// B of the reference's spmma is row-major k x n (spmma.hxx:40-64); sm_spmma_i8 wants it [n][k].  One-off helper for
// the (small, reused) weight operand: 64 x 64 byte tiles through LDS.
__global__ __launch_bounds__(256) void transpose_i8_kernel(const uint8_t* in, uint8_t* out, size_t rows, size_t cols) {
  __shared__ uint8_t tile[64][65];
  const size_t r0 = (size_t)blockIdx.y * 64, c0 = (size_t)blockIdx.x * 64;
  for (unsigned i = threadIdx.x; i < 64 * 64; i += 256) {
    const unsigned r = i >> 6, c = i & 63u;
    tile[r][c] = (r0 + r < rows && c0 + c < cols) ? in[(r0 + r) * cols + c0 + c] : (uint8_t)0;
  }
  __syncthreads();
  for (unsigned i = threadIdx.x; i < 64 * 64; i += 256) {
    const unsigned c = i >> 6, r = i & 63u;
    if (r0 + r < rows && c0 + c < cols) out[(c0 + c) * rows + r0 + r] = tile[r][c];
  }
}

}  // namespace sm

using namespace sm;

extern "C" {

int sm_transpose_i8(const void* in, void* out, size_t rows, size_t cols, sm_stream_t s) {
  if (!in || !out || in == out) {
    set_error("sm_transpose_i8: invalid argument (out of place only)");
    return SM_STATUS_INVALID_VALUE;
  }
  if (rows == 0 || cols == 0) return SM_STATUS_SUCCESS;
  if (ceil_div(rows, (size_t)64) > 65535 || ceil_div(cols, (size_t)64) > 0x7fffffffull) {
    set_error("sm_transpose_i8: matrix too large");
    return SM_STATUS_NOT_SUPPORTED;
  }
  transpose_i8_kernel<<<dim3((unsigned)ceil_div(cols, (size_t)64), (unsigned)ceil_div(rows, (size_t)64)), 256, 0, (hipStream_t)s>>>(
      (const uint8_t*)in, (uint8_t*)out, rows, cols);
  return check_launch("transpose_i8_kernel");
}

int sm_prune24_i8(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, int alg, sm_stream_t s) {
  if (!A_in || !A_out || ld < k) {
    set_error("sm_prune24_i8: invalid argument");
    return SM_STATUS_INVALID_VALUE;
  }
  if (alg != SM_PRUNE_STRIP && alg != SM_PRUNE_TILE) {
    set_error("sm_prune24_i8: invalid rule");
    return SM_STATUS_INVALID_VALUE;
  }
  if (m == 0 || k == 0) return SM_STATUS_SUCCESS;
  return launch_prune24_b8<ElemI8>(A_in, A_out, m, k, ld, alg, (hipStream_t)s);
}

int sm_prune24_check_i8(const void* A, size_t m, size_t k, size_t ld, int* d_valid, sm_stream_t s) {
  if (!A || !d_valid || ld < k) {
    set_error("sm_prune24_check_i8: invalid argument");
    return SM_STATUS_INVALID_VALUE;
  }
  return launch_prune24_check_b8<ElemI8>(A, m, k, ld, d_valid, (hipStream_t)s);
}

int sm_compress24_i8(const void* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* blob, sm_stream_t s) {
  if (!A || !blob || ld < k || !aligned16(blob)) {
    set_error("sm_compress24_i8: invalid argument (blob must be 16-byte aligned)");
    return SM_STATUS_INVALID_VALUE;
  }
  return launch_compress24_b8<ElemI8>(A, m, k, ld, batch, strideA, blob, (hipStream_t)s, "sm_compress24_i8");
}

int sm_decompress24_i8(const void* blob, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* A, sm_stream_t s) {
  if (!A || !blob || ld < k) {
    set_error("sm_decompress24_i8: invalid argument");
    return SM_STATUS_INVALID_VALUE;
  }
  return launch_decompress24_b8(blob, m, k, ld, batch, strideA, A, (hipStream_t)s);
}

}  // extern "C"

static int spmma_i8_entry(const void* blob, const void* B, int32_t* C, int8_t* C8, float scale, size_t m, size_t n, size_t k, size_t batch,
                          size_t strideB, size_t strideC, int accumulate, sm_stream_t stream) {
  if (!blob || !B || (!C && !C8) || !aligned16(blob)) {
    set_error("sm_spmma_i8: invalid argument (blob must be 16-byte aligned)");
    return SM_STATUS_INVALID_VALUE;
  }
  if (m == 0 || n == 0 || batch == 0) return SM_STATUS_SUCCESS;
  if (m * batch > 0x7fffffffull || n > 0x7fffffffull || k > 0x7fffffffull) {
    set_error("sm_spmma_i8: dimension exceeds 2^31-1");
    return SM_STATUS_NOT_SUPPORTED;
  }
  // whole 64-k planes of 16-byte chunks; metadata moves as 16-byte row pairs: even row counts
  if (k % 64 != 0 || m % 2 != 0 || !aligned16(B) || strideB % 16 != 0) {
    set_error("sm_spmma_i8: needs k %% 64 == 0, an even m and a 16-byte aligned B ([n][k], k-contiguous)");
    return SM_STATUS_NOT_SUPPORTED;
  }
  const BlobLayout L = blob_layout(m, k, 1, batch);
  Spmma8Args a = {};
  a.vals = (const char*)blob;
  a.meta = (const char*)blob + L.meta_off;
  a.Mtot = L.M;
  a.B = (const uint8_t*)B;
  a.C = C;
  a.C8 = C8;
  a.scale = scale;
  a.sB = strideB; a.sC = strideC;
  a.m = (int)m; a.Mrows = (int)m; a.N = (int)n; a.K = (int)k; a.nplanes = (int)(L.kc / 64);
  a.batch = (int)batch; a.accumulate = accumulate != 0;
  if (batch > 1 && strideB == 0 && strideC == m * n) {  // shared B + contiguous C: one tall matrix
    a.Mrows = (int)(m * batch);
    a.batch = 1;
  }
  hipStream_t st = (hipStream_t)stream;
  // narrow outputs: 128 x 64 tiles over 4 waves (more tiles); otherwise 128 x 128 over 8 (tools/archive/i8_probe.py)
  return n <= 128 ? launch_spmma_b8<MmaI8, 64, 4, 1>(a, st, "sm_spmma_i8") : launch_spmma_b8<MmaI8, 128, 2, 4>(a, st, "sm_spmma_i8");
}

static int spmma_fused_i8_entry(const void* A, const void* B, int32_t* C, int8_t* C8, float scale, size_t m, size_t n, size_t k, size_t lda,
                                size_t batch, size_t strideA, size_t strideB, size_t strideC, int accumulate, sm_stream_t stream) {
  if (!A || !B || (!C && !C8) || lda < k) {
    set_error("sm_spmma_fused_i8: invalid argument");
    return SM_STATUS_INVALID_VALUE;
  }
  if (m == 0 || n == 0 || batch == 0) return SM_STATUS_SUCCESS;
  if (m * batch > 0x7fffffffull || n > 0x7fffffffull || k > 0x7fffffffull || lda > 0x7fffffffull) {
    set_error("sm_spmma_fused_i8: dimension exceeds 2^31-1");
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (k % 64 != 0 || lda % 16 != 0 || strideA % 16 != 0 || strideB % 16 != 0 || !aligned16(A) || !aligned16(B)) {
    set_error("sm_spmma_fused_i8: needs k %% 64 == 0 and 16-byte aligned rows of A and B (use sm_compress24_i8 + sm_spmma_i8)");
    return SM_STATUS_NOT_SUPPORTED;
  }
  Spmma8Args a = {};
  a.Ad = (const uint8_t*)A; a.sA = strideA; a.lda = (int)lda;
  a.B = (const uint8_t*)B;
  a.C = C; a.C8 = C8; a.scale = scale;
  a.sB = strideB; a.sC = strideC;
  a.m = (int)m; a.Mrows = (int)m; a.N = (int)n; a.K = (int)k; a.nplanes = (int)(k / 64);
  a.batch = (int)batch; a.accumulate = accumulate != 0;
  if (batch > 1 && strideB == 0 && strideA == m * lda && strideC == m * n) {
    a.Mrows = (int)(m * batch);
    a.batch = 1;
  }
  hipStream_t st = (hipStream_t)stream;
  return n <= 64 ? launch_spmma_b8<MmaI8, 64, 4, 1, true>(a, st, "sm_spmma_fused_i8") : launch_spmma_b8<MmaI8, 128, 4, 2, true>(a, st, "sm_spmma_fused_i8");
}

extern "C" {

int sm_spmma_fused_i8(const void* A, const void* B, int32_t* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                      size_t strideB, size_t strideC, int accumulate, sm_stream_t stream) {
  return spmma_fused_i8_entry(A, B, C, nullptr, 1.0f, m, n, k, lda, batch, strideA, strideB, strideC, accumulate, stream);
}
int sm_spmma_fused_i8_q(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                        size_t strideB, size_t strideC, float scale, sm_stream_t stream) {
  return spmma_fused_i8_entry(A, B, nullptr, (int8_t*)C, scale, m, n, k, lda, batch, strideA, strideB, strideC, 0, stream);
}

int sm_spmma_i8(const void* blob, const void* B, int32_t* C, size_t m, size_t n, size_t k, size_t batch, size_t strideB, size_t strideC,
                int accumulate, sm_stream_t stream) {
  return spmma_i8_entry(blob, B, C, nullptr, 1.0f, m, n, k, batch, strideB, strideC, accumulate, stream);
}
int sm_spmma_i8_q(const void* blob, const void* B, void* C, size_t m, size_t n, size_t k, size_t batch, size_t strideB, size_t strideC,
                  float scale, sm_stream_t stream) {
  return spmma_i8_entry(blob, B, nullptr, (int8_t*)C, scale, m, n, k, batch, strideB, strideC, 0, stream);
}

}  // extern "C"
