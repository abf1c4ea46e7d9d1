// spmm_f16 m n k b [bf16] -- the Blocked-ELL x dense batch of bin/spmm on 16-bit operands (the type the reference's
// descriptors declare, spmm.hxx:57-67): b matrices with 2x2 blocks and ell_cols = k/2 (50 % block-sparse), per block row
// sorted distinct random block columns, one shared dense B; values and B uniform in (-0.5, 0.5) (bin/spmm's 1, 2, 3, ...
// overflow fp16).  fp16 by default, bfloat16 with the fifth argument `bf16`.  Prints the elapsed milliseconds.
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdlib>
#include <iostream>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include <sparsify.me/containers/ell.hxx>
#include <sparsify.me/spmm.hxx>
#include <sparsify.me/util/util.hxx>

template <typename type_t>
static int run(std::size_t m, std::size_t n, std::size_t k, std::size_t batch_size) {
  using namespace sparsifyme;
  const std::size_t block_size = 2;
  std::mt19937 gen(0x5eed);
  std::uniform_real_distribution<float> u(-0.5f, 0.5f);
  std::vector<ell_t<type_t, memory_space_t::device>> d_As(batch_size);
  for (std::size_t b = 0; b < batch_size; ++b) {
    ell_t<type_t, memory_space_t::host> h;
    h.rows = m; h.cols = k; h.block_size = block_size; h.ell_cols = k / 2;
    h.blocked_rows = m / block_size; h.blocked_cols = h.ell_cols / block_size;
    h.num_blocks = h.blocked_rows * h.blocked_cols;
    h.values.resize(h.rows * h.ell_cols);
    for (auto& v : h.values) v = type_t(u(gen));
    h.column_indices.resize(h.num_blocks);
    std::vector<std::size_t> all(k / block_size);
    std::iota(all.begin(), all.end(), std::size_t(0));
    for (std::size_t r = 0; r < h.blocked_rows; ++r) {
      std::shuffle(all.begin(), all.end(), gen);
      std::copy(all.begin(), all.begin() + h.blocked_cols, h.column_indices.begin() + r * h.blocked_cols);
      std::sort(h.column_indices.begin() + r * h.blocked_cols, h.column_indices.begin() + (r + 1) * h.blocked_cols);
    }
    d_As[b] = h;
  }
  host_vector<type_t> h_B(k * n);
  for (auto& v : h_B) v = type_t(u(gen));
  device_vector<type_t> d_B = h_B;
  std::vector<device_vector<type_t>> d_C(batch_size);
  std::vector<type_t*> Cs(batch_size);
  for (std::size_t b = 0; b < batch_size; ++b) {
    d_C[b].resize(m * n);
    Cs[b] = d_C[b].data().get();
  }
  float elapsed = batched::spmm(d_As.data(), d_B.data().get(), Cs.data(), m, n, k, batch_size);
  if (hipDeviceSynchronize() != hipSuccess) return EXIT_FAILURE;
  std::cout << elapsed << std::endl;
  return EXIT_SUCCESS;
}

int main(int argc, char** argv) {
  if (argc != 5 && !(argc == 6 && std::string(argv[5]) == "bf16")) {
    std::cout << "Invalid # of arguments. Usage: ./spmm_f16 m n k b [bf16]" << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t m = std::stoi(argv[1]), n = std::stoi(argv[2]), k = std::stoi(argv[3]), b = std::stoi(argv[4]);
  return argc == 6 ? run<__bf16>(m, n, k, b) : run<__half>(m, n, k, b);
}
