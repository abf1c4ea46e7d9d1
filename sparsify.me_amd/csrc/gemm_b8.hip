// gemm_b8.hip -- dense fp8 and int8 GEMM on the 1-byte matrix cores: the like-for-like dense denominator of sm_spmma_fp8 /
// sm_spmma_i8 (same layouts, same epilogues), as sm_gemm_rowmajor_f16 is for the 16-bit 2:4 kernels.
//   sm_gemm_rowmajor_fp8: C = alpha * row_scale[i] * (A . B) + beta * C on v_mfma_f32_16x16x128_f8f6f4 (any A/B format pair,
//   fp32 / fp16 / bf16 out); sm_gemm_rowmajor_i8[_q]: C (int32, + C when accumulating) = A . B, or requantised int8, on
//   v_mfma_i32_16x16x64_i8.  A is row-major m x k (lda), B [n][k] k-contiguous, C row-major m x n.
// The kernel is spmma_b8_kernel's DENSE A mode (spmma_b8.h): the fused form's staging of the dense A tile and its
// epilogues, with the dense instruction in place of the selection and the sparse instruction.
#include "spmma_b8.h"

using namespace sm;

namespace {

bool fmt_ok(int f) { return f == SM_FP8_E4M3 || f == SM_FP8_E5M2; }
bool out_ok(int o) { return o == SM_OUT_F32 || o == SM_OUT_F16 || o == SM_OUT_BF16; }

// the fused 1-byte form's tiles: 128 x 64 over 4 x 1 waves for n <= 64, otherwise 128 x 128 over 4 x 2
template <class MM>
int gemm_b8_launch(const Spmma8Args& a, size_t n, hipStream_t st, const char* what) {
  return n <= 64 ? launch_spmma_b8<MM, 64, 4, 1>(a, st, what) : launch_spmma_b8<MM, 128, 4, 2>(a, st, what);
}

// validation shared by the three entries (C: the output, whatever its type); SM_STATUS_SUCCESS = go on, -1 = nothing to do
int gemm_b8_check(const void* A, const void* B, const void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                  size_t strideB, const char* what) {
  if (!A || !B || !C || lda < k) {
    set_error("%s: invalid argument", what);
    return SM_STATUS_INVALID_VALUE;
  }
  if (m == 0 || n == 0 || batch == 0) return -1;
  if (m * batch > 0x7fffffffull || n > 0x7fffffffull || k > 0x7fffffffull || lda > 0x7fffffffull) {
    set_error("%s: dimension exceeds 2^31-1", what);
    return SM_STATUS_NOT_SUPPORTED;
  }
  // whole 64-k planes of 16-byte chunks, 16-byte aligned rows (no even-m rule: no metadata row pairs here)
  if (k % 64 != 0 || lda % 16 != 0 || strideA % 16 != 0 || strideB % 16 != 0 || !aligned16(A) || !aligned16(B)) {
    set_error("%s: needs k %% 64 == 0 and 16-byte aligned rows of A and B", what);
    return SM_STATUS_NOT_SUPPORTED;
  }
  return SM_STATUS_SUCCESS;
}

// the geometry of a checked call; shared B + contiguous A and C fold into one tall matrix (row_scale indexed by row % m)
Spmma8Args gemm_b8_args(const void* A, const void* B, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA, size_t strideB,
                        size_t strideC) {
  Spmma8Args a = {};
  a.Ad = (const uint8_t*)A; a.sA = strideA; a.lda = (int)lda;
  a.B = (const uint8_t*)B;
  a.sB = strideB; a.sC = strideC;
  a.m = (int)m; a.Mrows = (int)m; a.N = (int)n; a.K = (int)k; a.nplanes = (int)(k / 64);
  a.batch = (int)batch;
  if (batch > 1 && strideB == 0 && strideA == m * lda && strideC == m * n) {
    a.Mrows = (int)(m * batch);
    a.batch = 1;
  }
  return a;
}

template <int FA, int FB>
int gemm_fp8_pair(const Spmma8Args& a, size_t n, hipStream_t st) {
  return gemm_b8_launch<MmaF8Dense<FA, FB>>(a, n, st, "sm_gemm_rowmajor_fp8");
}

int gemm_i8_entry(const void* A, const void* B, int32_t* C, int8_t* C8, float scale, size_t m, size_t n, size_t k, size_t lda, size_t batch,
                  size_t strideA, size_t strideB, size_t strideC, int accumulate, sm_stream_t stream, const char* what) {
  const int rc = gemm_b8_check(A, B, C ? (const void*)C : (const void*)C8, m, n, k, lda, batch, strideA, strideB, what);
  if (rc != SM_STATUS_SUCCESS) return rc < 0 ? SM_STATUS_SUCCESS : rc;
  Spmma8Args a = gemm_b8_args(A, B, m, n, k, lda, batch, strideA, strideB, strideC);
  a.C = C; a.C8 = C8; a.scale = scale; a.accumulate = accumulate != 0;
  return gemm_b8_launch<MmaI8Dense>(a, n, (hipStream_t)stream, what);
}

}  // namespace

extern "C" {

int sm_gemm_rowmajor_fp8(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                         size_t strideB, size_t strideC, int fmt_a, int fmt_b, int out_type, float alpha, float beta, const float* row_scale,
                         sm_stream_t stream) {
  if (!fmt_ok(fmt_a) || !fmt_ok(fmt_b) || !out_ok(out_type)) {
    set_error("sm_gemm_rowmajor_fp8: invalid argument (fmt SM_FP8_*, out_type SM_OUT_*)");
    return SM_STATUS_INVALID_VALUE;
  }
  const int rc = gemm_b8_check(A, B, C, m, n, k, lda, batch, strideA, strideB, "sm_gemm_rowmajor_fp8");
  if (rc != SM_STATUS_SUCCESS) return rc < 0 ? SM_STATUS_SUCCESS : rc;
  Spmma8Args a = gemm_b8_args(A, B, m, n, k, lda, batch, strideA, strideB, strideC);
  a.Cf = C; a.out_type = out_type; a.alpha = alpha; a.beta = beta; a.row_scale = row_scale;
  const hipStream_t st = (hipStream_t)stream;
  if (fmt_a == SM_FP8_E4M3) return fmt_b == SM_FP8_E4M3 ? gemm_fp8_pair<SM_FP8_E4M3, SM_FP8_E4M3>(a, n, st) : gemm_fp8_pair<SM_FP8_E4M3, SM_FP8_E5M2>(a, n, st);
  return fmt_b == SM_FP8_E4M3 ? gemm_fp8_pair<SM_FP8_E5M2, SM_FP8_E4M3>(a, n, st) : gemm_fp8_pair<SM_FP8_E5M2, SM_FP8_E5M2>(a, n, st);
}

int sm_gemm_rowmajor_i8(const void* A, const void* B, int32_t* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                        size_t strideB, size_t strideC, int accumulate, sm_stream_t stream) {
  return gemm_i8_entry(A, B, C, nullptr, 1.0f, m, n, k, lda, batch, strideA, strideB, strideC, accumulate, stream, "sm_gemm_rowmajor_i8");
}

int sm_gemm_rowmajor_i8_q(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA,
                          size_t strideB, size_t strideC, float scale, sm_stream_t stream) {
  return gemm_i8_entry(A, B, nullptr, (int8_t*)C, scale, m, n, k, lda, batch, strideA, strideB, strideC, 0, stream, "sm_gemm_rowmajor_i8_q");
}

}  // extern "C"
