// spmm.hxx -- sparsifyme::batched::spmm (Blocked-ELL x dense) and batched::strided_coo (one COO
// matrix x a strided batch of dense matrices).
// Signatures of the reference's include/sparsify.me/spmm.hxx:30-41 and :140-153.  There: one
// cuSPARSE call per batch from one OpenMP host thread per batch on per-batch streams (:94-111), and
// a strided-batch COO call that does not compile as committed (:172,175,187).  Here: one batched
// kernel launch each.  Dense operands are column-major as the reference declares them
// (B k x n ld k, C_i m x n ld m: spmm.hxx:63,67); `As` and `Cs` are HOST arrays
// (examples/spmm.cu:96,102,115), `B` is shared by all batches.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstddef>
#include <cstdint>
#include <iostream>
#include <type_traits>
#include <vector>

#include <sparsifyme.h>
#include <sparsify.me/containers/ell.hxx>
#include <sparsify.me/gemm.hxx>  // operation_t
#include <sparsify.me/util/trace.hxx>
#include <sparsify.me/util/util.hxx>

namespace sparsifyme {
namespace batched {
namespace detail {
// The 16-bit element types of batched::spmm (the spellings spmma_fns<> accepts): fp16 and bfloat16 storage, fp32 accumulation.
template <typename type_t>
struct bell16_type {
  static constexpr bool bf16 = std::is_same<type_t, __bf16>::value || std::is_same<type_t, __hip_bfloat16>::value;
  static constexpr bool f16 = std::is_same<type_t, __half>::value || std::is_same<type_t, _Float16>::value;
  static_assert(bf16 || f16, "batched::spmm: 2-byte element types are __half, _Float16, __bf16 and __hip_bfloat16");
  static int batched(const void* const* v, const std::uint64_t* const* i, std::size_t rows, std::size_t cols, std::size_t bs,
                     std::size_t ell_cols, const void* B, void* const* C, std::size_t n, std::size_t batch, float al, float be) {
    return bf16 ? sm_spmm_bell_batched_bf16(v, i, rows, cols, bs, ell_cols, B, C, n, batch, al, be, nullptr)
                : sm_spmm_bell_batched_f16(v, i, rows, cols, bs, ell_cols, B, C, n, batch, al, be, nullptr);
  }
  static int single(const void* v, const std::uint64_t* i, std::size_t rows, std::size_t cols, std::size_t bs, std::size_t ell_cols,
                    const void* B, void* C, std::size_t n, float al, float be) {
    return bf16 ? sm_spmm_bell_bf16(v, i, rows, cols, bs, ell_cols, B, C, n, al, be, nullptr)
                : sm_spmm_bell_f16(v, i, rows, cols, bs, ell_cols, B, C, n, al, be, nullptr);
  }
};

// fp16 / bfloat16: the blocks are expanded inside the product (sm_spmm_bell_*_{f16,bf16}); no workspace
template <typename type_t>
float spmm16(ell_t<type_t, memory_space_t::device>* As, type_t* B, type_t** Cs, std::size_t n, std::size_t batch_size, float alpha,
             float beta) {
  using fns = bell16_type<type_t>;
  (void)hipDeviceSynchronize();
  util::timer_t t;
  int rc = SM_STATUS_SUCCESS;
  bool uniform = batch_size > 0;
  for (std::size_t b = 1; b < batch_size; ++b)
    uniform = uniform && As[b].rows == As[0].rows && As[b].cols == As[0].cols &&
              As[b].block_size == As[0].block_size && As[b].ell_cols == As[0].ell_cols;
  std::vector<const void*> vals(batch_size);
  std::vector<const std::uint64_t*> idx(batch_size);
  for (std::size_t b = 0; b < batch_size; ++b) {
    vals[b] = static_cast<const void*>(As[b].values.data().get());
    idx[b] = reinterpret_cast<const std::uint64_t*>(As[b].column_indices.data().get());
  }
  t.begin();
  util::range_t range("batched-SpMM");  // the reference's NVTX range (spmm.hxx:92,121)
  if (uniform) {
    rc = fns::batched(vals.data(), idx.data(), As[0].rows, As[0].cols, As[0].block_size, As[0].ell_cols, B,
                      reinterpret_cast<void* const*>(Cs), n, batch_size, alpha, beta);
  } else {
    for (std::size_t b = 0; b < batch_size; ++b) {
      auto& A = As[b];
      const int rb = fns::single(vals[b], idx[b], A.rows, A.cols, A.block_size, A.ell_cols, B, Cs[b], n, alpha, beta);
      if (rc == SM_STATUS_SUCCESS) rc = rb;  // the first failing status is the one reported
    }
  }
  t.end();
  if (rc != SM_STATUS_SUCCESS) std::cerr << "sparsifyme::batched::spmm: " << sm_last_error() << std::endl;
  return t.milliseconds();
}
}  // namespace detail

template <typename type_t>
float spmm(ell_t<type_t, memory_space_t::device>* As,
           type_t* B,
           type_t** Cs,
           std::size_t m,
           std::size_t n,
           std::size_t k,
           std::size_t batch_size,
           operation_t transpose_a = operation_t::N,
           operation_t transpose_b = operation_t::N,
           float alpha = 1.0f,
           float beta = 0.0f) {
  static_assert(sizeof(type_t) == 4 || sizeof(type_t) == 2, "Blocked-ELL SpMM: fp32, fp16 or bfloat16 elements");
  (void)transpose_a;
  (void)transpose_b;
  (void)m;
  (void)k;
  if constexpr (sizeof(type_t) == 2) {
    return detail::spmm16(As, B, Cs, n, batch_size, alpha, beta);
  } else {
    (void)hipDeviceSynchronize();
    util::timer_t t;
    int rc = SM_STATUS_SUCCESS;
    // The reference creates its per-batch cuSPARSE descriptors and buffers before its timed region (spmm.hxx:70-88);
    // the analogue here is the dense-expansion workspace.  Equal-shaped batches (what every driver builds) go down
    // in one submission; ragged ones batch by batch through a single reused workspace.
    bool uniform = batch_size > 0;
    for (std::size_t b = 1; b < batch_size; ++b)
      uniform = uniform && As[b].rows == As[0].rows && As[b].cols == As[0].cols &&
                As[b].block_size == As[0].block_size && As[b].ell_cols == As[0].ell_cols;
    std::size_t ws_bytes = 0;
    std::vector<const float*> vals(batch_size);
    std::vector<const std::uint64_t*> idx(batch_size);
    for (std::size_t b = 0; b < batch_size; ++b) {
      std::size_t w = 0;
      (void)sm_spmm_bell_workspace_size(As[b].rows, As[b].cols, &w);
      ws_bytes = w > ws_bytes ? w : ws_bytes;
      vals[b] = reinterpret_cast<const float*>(As[b].values.data().get());
      idx[b] = reinterpret_cast<const std::uint64_t*>(As[b].column_indices.data().get());
    }
    if (uniform) (void)sm_spmm_bell_batched_workspace_size(As[0].rows, As[0].cols, batch_size, &ws_bytes);
    device_vector<unsigned char> ws(ws_bytes);
    t.begin();
    util::range_t range("batched-SpMM");  // the reference's NVTX range (spmm.hxx:92,121)
    if (uniform) {
      rc = sm_spmm_bell_batched_f32(vals.data(), idx.data(), As[0].rows, As[0].cols, As[0].block_size, As[0].ell_cols,
                                    reinterpret_cast<const float*>(B), reinterpret_cast<float* const*>(Cs), n, batch_size,
                                    alpha, beta, ws.data().get(), nullptr);
    } else {
      for (std::size_t b = 0; b < batch_size; ++b) {
        auto& A = As[b];
        const int rb = sm_spmm_bell_f32_ws(vals[b], idx[b], A.rows, A.cols, A.block_size, A.ell_cols,
                                           reinterpret_cast<const float*>(B), reinterpret_cast<float*>(Cs[b]), n, alpha, beta,
                                           ws.data().get(), nullptr);
        if (rc == SM_STATUS_SUCCESS) rc = rb;  // the first failing status is the one reported
      }
    }
    t.end();
    if (rc != SM_STATUS_SUCCESS) std::cerr << "sparsifyme::batched::spmm: " << sm_last_error() << std::endl;
    return t.milliseconds();
  }
}

// strided_coo computes in full fp32 by default, as the reference's cusparseSpMM call does (CUDA_R_32F operands and compute type,
// spmm.hxx:165-187).  fast = true opts in to the dense-MFMA form first (operands rounded once to fp16: result within 2^-11 of
// sum|a||b| instead of fp32 arithmetic -- about 12 bits of operand precision traded for speed; see below)
struct strided_coo_options_t {
  bool fast = false;
};
inline strided_coo_options_t& strided_coo_options() {
  static strided_coo_options_t o;
  return o;
}

template <typename type_t>
float strided_coo(std::size_t A_num_rows,
                  std::size_t A_num_cols,
                  std::size_t A_nnz,
                  std::size_t B_num_rows,
                  std::size_t B_num_cols,
                  std::size_t num_batches,
                  int* dA_rows,
                  int* dA_cols,
                  type_t* dA_values,
                  type_t* dB,
                  type_t* dC,
                  type_t alpha = 1.0f,
                  type_t beta = 0.0f) {
  static_assert(sizeof(type_t) == 4, "this build implements the fp32 COO SpMM");
  (void)B_num_rows;  // == A_num_cols
  util::timer_t t;
  util::range_t range("strided-COO-SpMM");
  t.begin();  // the reference times its buffer allocation too (spmm.hxx:155-156,183)
  int rc = SM_STATUS_NOT_SUPPORTED;
  // Opt-in only (strided_coo_options().fast = true; round 5, ADVICE round 4: an fp32 caller must not lose operand precision
  // silently): first the matrix-core form (sm_spmm_coo_f32_fast: operands scaled by powers of two and rounded to fp16, fp32
  // accumulation; result within 2^-11 of sum|a||b|, include/sparsifyme.h; round 5: for beta == 0 and at most 20 % of A present the
  // product runs on the sparse matrix instruction from a 2:4 image of A, any A_num_cols) where it pays -- at least ~2 % of A's entries present:
  // below that the exact kernels' work, which follows nnz, is less than the dense product's -- and where the library takes the
  // shape.  It raises a flag on the device and leaves C untouched when an operand does not fit the fp16 range under its scales;
  // the exact form below then runs on the untouched operands.
  const bool dense_enough = A_nnz * 50 >= A_num_rows * A_num_cols;
  if (strided_coo_options().fast && dense_enough) {
    std::size_t fast_bytes = 0;
    if (sm_spmm_coo_fast_workspace_size(A_num_rows, A_num_cols, B_num_cols, num_batches, &fast_bytes) == SM_STATUS_SUCCESS) {
      device_vector<unsigned char> fws(fast_bytes);
      rc = sm_spmm_coo_f32_fast(A_num_rows, A_num_cols, A_nnz, B_num_cols, num_batches, dA_rows, dA_cols,
                                reinterpret_cast<const float*>(dA_values), reinterpret_cast<const float*>(dB),
                                reinterpret_cast<float*>(dC), alpha, beta, fws.data().get(), fast_bytes, nullptr);
      if (rc == SM_STATUS_SUCCESS) {
        int flag = 1;
        if (sm_spmm_coo_fast_flag(fws.data().get(), &flag, nullptr) != SM_STATUS_SUCCESS || flag != 0) rc = SM_STATUS_NOT_SUPPORTED;
      }
    }
  }
  if (rc != SM_STATUS_SUCCESS) {
    // the packed form's workspace (the counterpart of cusparseSpMM's buffer, spmm.hxx:178-183); the call itself picks the
    // kernel: packed CSR for row-sorted input that fits, the row-pointer form or the atomic kernels otherwise
    std::size_t ws_bytes = 0;
    (void)sm_spmm_coo_packed_workspace_size(A_num_rows, A_nnz, &ws_bytes);
    device_vector<unsigned char> ws(ws_bytes);
    rc = sm_spmm_coo_f32_packed(A_num_rows, A_num_cols, A_nnz, B_num_cols, num_batches, dA_rows, dA_cols,
                                reinterpret_cast<const float*>(dA_values), reinterpret_cast<const float*>(dB),
                                reinterpret_cast<float*>(dC), alpha, beta, ws.data().get(), ws_bytes, nullptr);
    (void)hipStreamSynchronize(nullptr);  // the workspace is released when this scope ends
  }
  t.end();
  if (rc != SM_STATUS_SUCCESS) std::cerr << "sparsifyme::batched::strided_coo: " << sm_last_error() << std::endl;
  return t.milliseconds();
}
}  // namespace batched
}  // namespace sparsifyme
