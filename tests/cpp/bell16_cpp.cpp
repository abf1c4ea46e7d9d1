// batched::spmm<__half> through the C++ headers on a uniform batch (one sm_spmm_bell_batched_f16 call) and a ragged batch (one
// sm_spmm_bell_f16 call per matrix), each checked against a double loop on the host.  Built and run by tests/test_gpu_bell16.py.
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include <sparsify.me/containers/ell.hxx>
#include <sparsify.me/spmm.hxx>

using namespace sparsifyme;

static ell_t<__half, memory_space_t::host> make(std::size_t rows, std::size_t cols, std::size_t bs, std::mt19937& gen) {
  std::uniform_real_distribution<float> u(-0.5f, 0.5f);
  ell_t<__half, memory_space_t::host> h;
  h.rows = rows; h.cols = cols; h.block_size = bs;
  const std::size_t nbc = cols / bs;
  h.blocked_rows = (rows + bs - 1) / bs; h.blocked_cols = nbc / 2 > 0 ? nbc / 2 : 1;
  h.ell_cols = h.blocked_cols * bs;
  h.num_blocks = h.blocked_rows * h.blocked_cols;
  h.values.resize(rows * h.ell_cols);
  for (auto& v : h.values) v = __float2half(u(gen));
  h.column_indices.resize(h.num_blocks);
  std::vector<std::size_t> all(nbc);
  std::iota(all.begin(), all.end(), std::size_t(0));
  for (std::size_t r = 0; r < h.blocked_rows; ++r) {
    std::shuffle(all.begin(), all.end(), gen);
    std::copy(all.begin(), all.begin() + h.blocked_cols, h.column_indices.begin() + r * h.blocked_cols);
    std::sort(h.column_indices.begin() + r * h.blocked_cols, h.column_indices.begin() + (r + 1) * h.blocked_cols);
  }
  return h;
}

// max |got - ref| / (sum |a||b| + tiny) over C
static double check(const ell_t<__half, memory_space_t::host>& A, const std::vector<__half>& B, const std::vector<__half>& C, std::size_t n) {
  double worst = 0.0;
  const std::size_t bcols = A.ell_cols / A.block_size, nbc = A.cols / A.block_size;
  for (std::size_t j = 0; j < n; ++j)
    for (std::size_t i = 0; i < A.rows; ++i) {
      double acc = 0.0, scale = 0.0;
      const std::size_t br = i / A.block_size;
      for (std::size_t e = 0; e < bcols; ++e) {
        const std::size_t bc = A.column_indices[br * bcols + e];
        if (bc >= nbc) continue;
        for (std::size_t t = 0; t < A.block_size; ++t) {
          const double a = __half2float(A.values[i * A.ell_cols + e * A.block_size + t]);
          const double b = __half2float(B[j * A.cols + bc * A.block_size + t]);
          acc += a * b;
          scale += std::fabs(a * b);
        }
      }
      const double err = std::fabs((double)__half2float(C[j * A.rows + i]) - acc) / (scale + 1e-6);
      worst = err > worst ? err : worst;
    }
  return worst;
}

static int run(const std::vector<std::size_t>& rows, std::size_t cols, std::size_t bs, std::size_t n, const char* what) {
  std::mt19937 gen(0xbe11);
  std::uniform_real_distribution<float> u(-0.5f, 0.5f);
  const std::size_t batch = rows.size();
  std::vector<ell_t<__half, memory_space_t::host>> hA(batch);
  std::vector<ell_t<__half, memory_space_t::device>> dA(batch);
  for (std::size_t b = 0; b < batch; ++b) {
    hA[b] = make(rows[b], cols, bs, gen);
    dA[b] = hA[b];
  }
  host_vector<__half> hB(cols * n);
  for (auto& v : hB) v = __float2half(u(gen));
  device_vector<__half> dB = hB;
  std::vector<device_vector<__half>> dC(batch);
  std::vector<__half*> Cs(batch);
  for (std::size_t b = 0; b < batch; ++b) {
    dC[b].resize(rows[b] * n);
    Cs[b] = dC[b].data().get();
  }
  const float ms = batched::spmm(dA.data(), dB.data().get(), Cs.data(), 0, n, cols, batch);
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  std::vector<__half> B(hB.begin(), hB.end());
  double worst = 0.0;
  for (std::size_t b = 0; b < batch; ++b) {
    host_vector<__half> hc;
    assign(hc, dC[b]);
    const double w = check(hA[b], B, std::vector<__half>(hc.begin(), hc.end()), n);
    worst = w > worst ? w : worst;
  }
  std::printf("%s: %.3f ms, max err / sum|a||b| = %.3e\n", what, ms, worst);
  return worst <= 1e-2 ? 0 : 1;
}

int main() {
  int rc = run({200, 200, 200}, 136, 2, 70, "uniform");
  rc |= run({130, 64, 257}, 136, 2, 37, "ragged");
  std::printf(rc ? "FAIL\n" : "OK\n");
  return rc;
}
