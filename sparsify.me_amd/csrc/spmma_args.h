// spmma_args.h -- argument block shared by the 2:4 matmul kernels (spmma_f16.hip, spmma_f16_pc.hip).
#pragma once
#include "mma_tile.h"

namespace sm {

// A launch serves up to SPMMA_MAXG same-shape problems (sm_spmma_*_grouped: the 3-6 instances of one layer shape in a network as ONE
// grid, so that a few-tile shape's last partial round is filled by the next instance): the operand pointers are tables indexed by the
// problem a workgroup belongs to, block -> (problem, grid batch, tile).  A single call is a group of one.
constexpr int SPMMA_MAXG = 8;
struct SpmmaArgs {
  const char* vals[SPMMA_MAXG];   // stage-major [kc/64][Mtot][32] halves (64 B per row per plane)
  const char* meta[SPMMA_MAXG];   // stage-major [kc/64][Mtot][8 B]
  size_t Mtot;        // rows of the whole blob (m * batch)
  const half_t* B[SPMMA_MAXG];
  half_t* C[SPMMA_MAXG];
  int ngroup;
  size_t sB, sC;      // batch strides (elements); rows of batch b are [b*m, (b+1)*m)
  int m;              // rows per batch
  int Mrows;          // rows this launch treats as one matrix (m, or m*batch when stacked)
  int N, K, kc;
  int batch;          // grid batches (1 when stacked)
  int tiles_m, tiles_n;
  float alpha, beta;
};

// The argument block of the kernels' epilogue instantiations (sm_spmma_*_ex): the plain block + the epilogue.  The plain
// instantiations keep taking SpmmaArgs itself, so their code is what it was.
struct SpmmaArgsEpi : SpmmaArgs {
  EpiArgs e;
};
template <bool EPI> struct SpmmaArgsSel { typedef SpmmaArgs type; };
template <> struct SpmmaArgsSel<true> { typedef SpmmaArgsEpi type; };

// sm_epilogue_t -> EpiArgs for one problem (D, strideD, rows per batch m), with the argument checks of the _ex entry points
// (include/sparsifyme.h).  *plain: the epilogue is the plain entry point's (no bias, no activation, R == D or not read).
inline int epilogue_args(const sm_epilogue_t* ep, const void* D, size_t strideD, size_t m, float beta, EpiArgs& e, bool* plain, const char* who) {
  e = EpiArgs{nullptr, (const half_t*)D, strideD, SM_BIAS_COL, SM_ACT_NONE, 0.0f, (int)(m ? m : 1)};
  *plain = true;
  if (!ep) return SM_STATUS_SUCCESS;
  if (ep->act < SM_ACT_NONE || ep->act > SM_ACT_HARDSWISH || (ep->bias_dim != SM_BIAS_COL && ep->bias_dim != SM_BIAS_ROW)) {
    set_error("%s: invalid epilogue (unknown act or bias_dim)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (beta != 0.0f && !ep->R) {
    set_error("%s: invalid epilogue (beta != 0 needs the residual operand R)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (ep->act == SM_ACT_CLIPPED_RELU && !(ep->act_arg >= 0.0f && ep->act_arg <= 3.4028234663852886e38f)) {
    set_error("%s: invalid epilogue (the clipped ReLU needs a finite act_arg >= 0)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  e.bias = ep->bias;
  e.bias_dim = ep->bias_dim;
  e.act = ep->act;
  e.act_arg = ep->act_arg;
  if (beta != 0.0f) {
    e.R = (const half_t*)ep->R;
    e.sR = ep->strideR;
  }
  *plain = !ep->bias && ep->act == SM_ACT_NONE && (beta == 0.0f || (ep->R == D && ep->strideR == strideD));
  return SM_STATUS_SUCCESS;
}

// The dense twin (spmma_f16_fused.hip): C = alpha * A * B + beta * C, row-major, dense, through the pipelines of the fused 2:4
// kernels (direct / big / span) with dense MFMA in place of selection + SMFMAC -- so that the dense GEMM the 2:4 path is measured
// against is not held back by a weaker pipeline on the shapes where those pipelines are the better ones (ragged k: the span form;
// n > 128: 256 x 256 tiles).  SM_STATUS_NOT_SUPPORTED: not a shape it serves; the caller runs gemm_f16.hip's own kernels.
struct DenseTwinCall {
  const half_t* A; const half_t* B; half_t* C;
  const half_t* const* Ap; const half_t* const* Bp; half_t* const* Cp;  // optional device pointer arrays (batch entries)
  size_t sA, sB, sC;
  int M, N, K, lda, batch;
  float alpha, beta;
  bool bf;
  void* workspace;         // sm_gemm_*_ws: the stream-K form may run (sm_spmma_fused_workspace_size bytes, zero flag page); else null
  size_t workspace_bytes;
};
int gemm_dense_twin(const DenseTwinCall& c, hipStream_t st);

// spmma_f16_thin.hip: the fused 2:4 product for n < 8, k <= 64 (depthwise convolutions as im2col products) on the vector ALUs;
// SM_STATUS_NOT_SUPPORTED for anything else
// the shapes it takes (ONE statement: asked by spmma_fused_thin itself and by the fused dispatch rule, spmma_f16_fused.hip: fused_form);
// on top of these A is 16-byte aligned
inline bool thin_form_takes(size_t ngroup, size_t rows, size_t n, size_t k) {
  return !(n == 0 || n >= 8 || k == 0 || k > 64 || ngroup < 1 || ngroup > 8 || (rows * k * 2) % 16 != 0 || rows * k * 2 < 16) &&
         (rows + 1023) / 1024 <= 0x7fffffffu;  // (its grid: 1024 rows per workgroup)
}
int spmma_fused_thin(bool bf, int ngroup, const void* const* A, const void* const* B, void* const* C, size_t rows, size_t n, size_t k,
                     float alpha, float beta, hipStream_t st);

// spmma_f16_fused.hip: does sm_spmma_fused_{f16,bf16} take this single problem with one of its EXACT forms (bit-identical to
// sm_compress24 + sm_spmma; the thin form is excluded)?  Asked by the prune-in-place + multiply entry points before they touch A.
bool spmma_fused16_takes_exact(const void* A, const void* B, const void* C, size_t m, size_t n, size_t k, size_t lda, size_t batch, size_t strideA, size_t strideB,
                               size_t strideC);

}  // namespace sm
