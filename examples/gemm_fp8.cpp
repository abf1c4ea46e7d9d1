// gemm_fp8 m n k b -- the dense OCP fp8 (e4m3) GEMM through the C ABI, the dense counterpart of bin/spmma_fp8 with its
// operand roles: b matrices A (m x k, row-major), one shared B given [n][k] (k-contiguous per output column; made here from
// the row-major k x n B with sm_transpose_i8), bfloat16 C.
// Prints the time of one sm_gemm_rowmajor_fp8 call and a correctness line: sampled rows against the fp64 product, within
// 1e-2 of sum |a||b| (the tolerance of bin/spmma_fp8).
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include <sparsify.me/containers/vector.hxx>
#include <sparsify.me/util/util.hxx>
#include <sparsifyme.h>

// exact value of an e4m3 byte (no NaN is generated here)
static double e4m3_value(unsigned char v) {
  const int e = (v >> 3) & 15, mt = v & 7;
  const double mag = e == 0 ? std::ldexp(mt, -9) : std::ldexp(8 + mt, e - 10);
  return (v & 0x80) ? -mag : mag;
}
static double bf16_value(uint16_t v) {
  uint32_t w = static_cast<uint32_t>(v) << 16;
  float f;
  std::memcpy(&f, &w, 4);
  return f;
}

int main(int argc, char** argv) {
  using namespace sparsifyme;
  if (argc != 5) {
    std::cout << "Invalid # of arguments. Usage: ./gemm_fp8 m n k b" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t m = std::stoi(argv[1]), n = std::stoi(argv[2]), k = std::stoi(argv[3]), b = std::stoi(argv[4]);
  // finite e4m3 values of both signs: magnitude codes 0x00 .. 0x5f (|x| <= 30)
  host_vector<unsigned char> h_A(m * k * b), h_B(k * n);
  auto draw = [] {
    const unsigned mag = static_cast<unsigned>(util::get_random<float>(0.f, 95.99f));
    return static_cast<unsigned char>(mag | (util::get_random<float>(0.f, 1.f) < 0.5f ? 0x80u : 0u));
  };
  for (auto& a : h_A) a = draw();
  for (auto& x : h_B) x = draw();
  device_vector<unsigned char> A = h_A, B = h_B, Bt(k * n);
  device_vector<uint16_t> C(m * n * b);
  int rc = sm_transpose_i8(B.data().get(), Bt.data().get(), k, n, nullptr);
  // once untimed (first-launch costs), then the timed call
  rc |= sm_gemm_rowmajor_fp8(A.data().get(), Bt.data().get(), C.data().get(), m, n, k, k, b, m * k, 0, m * n, SM_FP8_E4M3, SM_FP8_E4M3,
                             SM_OUT_BF16, 1.0f, 0.0f, nullptr, nullptr);
  util::timer_t t;
  t.begin();
  rc |= sm_gemm_rowmajor_fp8(A.data().get(), Bt.data().get(), C.data().get(), m, n, k, k, b, m * k, 0, m * n, SM_FP8_E4M3, SM_FP8_E4M3,
                             SM_OUT_BF16, 1.0f, 0.0f, nullptr, nullptr);
  const float ms = t.end();
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "gemm_fp8: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  std::cout << "GEMM Time (ms): " << ms << std::endl;

  // sampled rows (first and last of every batch matrix) against the fp64 product
  (void)hipDeviceSynchronize();
  const auto hC = C.to_host();
  double worst = 0.0;
  for (std::size_t bi = 0; bi < b; ++bi)
    for (std::size_t r : {std::size_t(0), m - 1}) {
      const std::size_t row = bi * m + r;
      for (std::size_t j = 0; j < n; ++j) {
        double ref = 0.0, scale = 0.0;
        for (std::size_t q = 0; q < k; ++q) {
          const double a = e4m3_value(h_A[row * k + q]), x = e4m3_value(h_B[q * n + j]);
          ref += a * x;
          scale += std::fabs(a * x);
        }
        const double bound = 1e-2 * scale + std::ldexp(1.0, -133);
        worst = std::fmax(worst, std::fabs(bf16_value(hC[row * n + j]) - ref) / bound);
      }
    }
  const bool correct = worst <= 1.0;
  std::cout << "Max error / (1e-2 sum|a||b|): " << worst << std::endl;
  std::cout << "Correct: " << (correct ? "yes" : "NO") << std::endl;
  return correct ? EXIT_SUCCESS : EXIT_FAILURE;
}
