// spmma_fp8.hip -- OCP fp8 (e4m3 / e5m2) forms of the 2:4 path: prune STRIP / TILE, check, compress, decompress, and the
// matmul on v_smfmac_f32_16x16x128_{fp8,bf8}_{fp8,bf8} (twice the 16-bit sparse rate per instruction: 128 dense k).
//   The rules are the fp16 rules on the exact fp16 image (ElemF8 in spmma_b8.h): fp8 is sign-magnitude with monotone
//   encodings, so bits & 0x7f orders |x| as bits & 0x7fff orders the image.  The blob is the int8 one (1-byte elements).
//   sm_spmma_fp8: C (fp32 / fp16 / bf16) = alpha * row_scale[i] * (A_2:4 . B) + beta * C, fp32 accumulation; B [n][k]
//   (k-contiguous per output column) as for int8.  The kernels are those of spmma_b8.h over ElemF8 / MmaF8: the operand
//   registers of the fp8 sparse instruction are the int8 one's, only the accumulator is fp32.
#include "spmma_b8.h"

using namespace sm;

namespace {

bool fmt_ok(int f) { return f == SM_FP8_E4M3 || f == SM_FP8_E5M2; }
bool out_ok(int o) { return o == SM_OUT_F32 || o == SM_OUT_F16 || o == SM_OUT_BF16; }

// the shape dispatch of the int8 entries (narrow outputs: 128 x 64 tiles over 4 waves; otherwise 128 x 128 over 8 / the
// fused form's 128 x 128 over 4 x 2), per format pair
template <int FA, int FB>
int spmma_fp8_launch(const Spmma8Args& a, size_t n, bool fused, hipStream_t st) {
  typedef MmaF8<FA, FB> MM;
  if (fused) return n <= 64 ? launch_spmma_b8<MM, 64, 4, 1, true>(a, st, "sm_spmma_fused_fp8") : launch_spmma_b8<MM, 128, 4, 2, true>(a, st, "sm_spmma_fused_fp8");
  return n <= 128 ? launch_spmma_b8<MM, 64, 4, 1>(a, st, "sm_spmma_fp8") : launch_spmma_b8<MM, 128, 2, 4>(a, st, "sm_spmma_fp8");
}

int spmma_fp8_dispatch(const Spmma8Args& a, int fa, int fb, size_t n, bool fused, hipStream_t st) {
  if (fa == SM_FP8_E4M3) return fb == SM_FP8_E4M3 ? spmma_fp8_launch<SM_FP8_E4M3, SM_FP8_E4M3>(a, n, fused, st)
                                                  : spmma_fp8_launch<SM_FP8_E4M3, SM_FP8_E5M2>(a, n, fused, st);
  return fb == SM_FP8_E4M3 ? spmma_fp8_launch<SM_FP8_E5M2, SM_FP8_E4M3>(a, n, fused, st) : spmma_fp8_launch<SM_FP8_E5M2, SM_FP8_E5M2>(a, n, fused, st);
}

}  // namespace

extern "C" {

int sm_prune24_fp8(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, int alg, int fmt, sm_stream_t s) {
  if (!A_in || !A_out || ld < k || (alg != SM_PRUNE_STRIP && alg != SM_PRUNE_TILE) || !fmt_ok(fmt)) {
    set_error("sm_prune24_fp8: invalid argument");
    return SM_STATUS_INVALID_VALUE;
  }
  if (m == 0 || k == 0) return SM_STATUS_SUCCESS;
  return fmt == SM_FP8_E4M3 ? launch_prune24_b8<ElemF8<SM_FP8_E4M3>>(A_in, A_out, m, k, ld, alg, (hipStream_t)s)
                            : launch_prune24_b8<ElemF8<SM_FP8_E5M2>>(A_in, A_out, m, k, ld, alg, (hipStream_t)s);
}

int sm_prune24_check_fp8(const void* A, size_t m, size_t k, size_t ld, int* d_valid, sm_stream_t s) {
  if (!A || !d_valid || ld < k) {
    set_error("sm_prune24_check_fp8: invalid argument");
    return SM_STATUS_INVALID_VALUE;
  }
  // the zero test is (v & 0x7f) == 0 for both formats
  return launch_prune24_check_b8<ElemF8<SM_FP8_E4M3>>(A, m, k, ld, d_valid, (hipStream_t)s);
}

int sm_compress24_fp8(const void* A, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* blob, int fmt, sm_stream_t s) {
  if (!A || !blob || ld < k || !aligned16(blob) || !fmt_ok(fmt)) {
    set_error("sm_compress24_fp8: invalid argument (blob must be 16-byte aligned)");
    return SM_STATUS_INVALID_VALUE;
  }
  return fmt == SM_FP8_E4M3 ? launch_compress24_b8<ElemF8<SM_FP8_E4M3>>(A, m, k, ld, batch, strideA, blob, (hipStream_t)s, "sm_compress24_fp8")
                            : launch_compress24_b8<ElemF8<SM_FP8_E5M2>>(A, m, k, ld, batch, strideA, blob, (hipStream_t)s, "sm_compress24_fp8");
}

int sm_decompress24_fp8(const void* blob, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, void* A, sm_stream_t s) {
  if (!A || !blob || ld < k) {
    set_error("sm_decompress24_fp8: invalid argument");
    return SM_STATUS_INVALID_VALUE;
  }
  return launch_decompress24_b8(blob, m, k, ld, batch, strideA, A, (hipStream_t)s);
}

int sm_spmma_fp8(const void* blob, const void* B, void* C, size_t m, size_t n, size_t k, size_t batch, size_t strideB, size_t strideC, int fmt_a,
                 int fmt_b, int out_type, float alpha, float beta, const float* row_scale, sm_stream_t stream) {
  if (!blob || !B || !C || !aligned16(blob) || !fmt_ok(fmt_a) || !fmt_ok(fmt_b) || !out_ok(out_type)) {
    set_error("sm_spmma_fp8: invalid argument (blob must be 16-byte aligned; fmt SM_FP8_*, out_type SM_OUT_*)");
    return SM_STATUS_INVALID_VALUE;
  }
  if (m == 0 || n == 0 || batch == 0) return SM_STATUS_SUCCESS;
  if (m * batch > 0x7fffffffull || n > 0x7fffffffull || k > 0x7fffffffull) {
    set_error("sm_spmma_fp8: dimension exceeds 2^31-1");
    return SM_STATUS_NOT_SUPPORTED;
  }
  // whole 64-k planes of 16-byte chunks; metadata moves as 16-byte row pairs: even row counts
  if (k % 64 != 0 || m % 2 != 0 || !aligned16(B) || strideB % 16 != 0) {
    set_error("sm_spmma_fp8: needs k %% 64 == 0, an even m and a 16-byte aligned B ([n][k], k-contiguous)");
    return SM_STATUS_NOT_SUPPORTED;
  }
  const BlobLayout L = blob_layout(m, k, 1, batch);
  Spmma8Args a = {};
  a.vals = (const char*)blob;
  a.meta = (const char*)blob + L.meta_off;
  a.Mtot = L.M;
  a.B = (const uint8_t*)B;
  a.Cf = C; a.out_type = out_type; a.alpha = alpha; a.beta = beta; a.row_scale = row_scale;
  a.sB = strideB; a.sC = strideC;
  a.m = (int)m; a.Mrows = (int)m; a.N = (int)n; a.K = (int)k; a.nplanes = (int)(L.kc / 64);
  a.batch = (int)batch;
  if (batch > 1 && strideB == 0 && strideC == m * n) {  // shared B + contiguous C: one tall matrix (row_scale indexed by row % m)
    a.Mrows = (int)(m * batch);
    a.batch = 1;
  }
  return spmma_fp8_dispatch(a, fmt_a, fmt_b, n, false, (hipStream_t)stream);
}

int sm_spmma_fused_fp8(const void* A, const void* B, void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA, size_t strideB,
                       size_t strideC, int fmt_a, int fmt_b, int out_type, float alpha, float beta, const float* row_scale, sm_stream_t stream) {
  if (!A || !B || !C || lda < k || !fmt_ok(fmt_a) || !fmt_ok(fmt_b) || !out_ok(out_type)) {
    set_error("sm_spmma_fused_fp8: invalid argument (fmt SM_FP8_*, out_type SM_OUT_*)");
    return SM_STATUS_INVALID_VALUE;
  }
  if (m == 0 || n == 0 || batch == 0) return SM_STATUS_SUCCESS;
  if (m * batch > 0x7fffffffull || n > 0x7fffffffull || k > 0x7fffffffull || lda > 0x7fffffffull) {
    set_error("sm_spmma_fused_fp8: dimension exceeds 2^31-1");
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (k % 64 != 0 || m % 2 != 0 || lda % 16 != 0 || strideA % 16 != 0 || strideB % 16 != 0 || !aligned16(A) || !aligned16(B)) {
    set_error("sm_spmma_fused_fp8: needs k %% 64 == 0, an even m and 16-byte aligned rows of A and B (use sm_compress24_fp8 + sm_spmma_fp8)");
    return SM_STATUS_NOT_SUPPORTED;
  }
  Spmma8Args a = {};
  a.Ad = (const uint8_t*)A; a.sA = strideA; a.lda = (int)lda;
  a.B = (const uint8_t*)B;
  a.Cf = C; a.out_type = out_type; a.alpha = alpha; a.beta = beta; a.row_scale = row_scale;
  a.sB = strideB; a.sC = strideC;
  a.m = (int)m; a.Mrows = (int)m; a.N = (int)n; a.K = (int)k; a.nplanes = (int)(k / 64);
  a.batch = (int)batch;
  if (batch > 1 && strideB == 0 && strideA == m * lda && strideC == m * n) {
    a.Mrows = (int)(m * batch);
    a.batch = 1;
  }
  return spmma_fp8_dispatch(a, fmt_a, fmt_b, n, true, (hipStream_t)stream);
}

}  // extern "C"
