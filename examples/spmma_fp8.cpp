// spmma_fp8 m n k b -- the OCP fp8 (e4m3) 2:4 path through the C ABI.  Operand roles as in examples/spmma.cu:48-59 --
// b matrices A (m x k, row-major), one shared B -- except that B is given [n][k] (k-contiguous per output column; made
// here from the row-major k x n B with sm_transpose_i8) and C is bfloat16.
// Prints the stage times with the labels of the fp16 driver, a correctness line (sampled rows against the fp64 product
// of the pruned operand, within 1e-2 of sum |a||b|: the parity tolerance of the test suite) and checks that the fused
// kernel returns the same bytes.
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
    std::cout << "Invalid # of arguments. Usage: ./spmma_fp8 m n k b" << std::endl;
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
  device_vector<uint16_t> C(m * n * b), C2(m * n * b);
  int rc = sm_transpose_i8(B.data().get(), Bt.data().get(), k, n, nullptr);

  util::timer_t t;
  device_vector<int> valid(1);
  t.begin();
  rc |= sm_prune24_fp8(A.data().get(), A.data().get(), m * b, k, k, SM_PRUNE_STRIP, SM_FP8_E4M3, nullptr);
  rc |= sm_prune24_check_fp8(A.data().get(), m * b, k, k, valid.data().get(), nullptr);
  const float prune_ms = t.end();
  std::size_t bytes = 0;
  rc |= sm_compress24_size(m, k, 1, b, &bytes);
  device_vector<unsigned char> blob(bytes);
  t.begin();
  rc |= sm_compress24_fp8(A.data().get(), m, k, k, b, m * k, blob.data().get(), SM_FP8_E4M3, nullptr);
  const float compress_ms = t.end();
  t.begin();
  rc |= sm_spmma_fp8(blob.data().get(), Bt.data().get(), C.data().get(), m, n, k, b, 0, m * n, SM_FP8_E4M3, SM_FP8_E4M3, SM_OUT_BF16,
                     1.0f, 0.0f, nullptr, nullptr);
  const float mul_ms = t.end();
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "spmma_fp8: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  std::cout << "Pruning Time (ms): " << prune_ms << std::endl;
  std::cout << "Compression Time (ms): " << compress_ms << std::endl;
  std::cout << "SpMMA Time (ms): " << mul_ms << std::endl;

  // sampled rows (first and last of every batch matrix) against the fp64 product of the pruned operand
  (void)hipDeviceSynchronize();
  const auto hA = A.to_host();
  const auto hC = C.to_host();
  const auto hv = valid.to_host();
  double worst = 0.0;
  for (std::size_t bi = 0; bi < b; ++bi)
    for (std::size_t r : {std::size_t(0), m - 1}) {
      const std::size_t row = bi * m + r;
      for (std::size_t j = 0; j < n; ++j) {
        double ref = 0.0, scale = 0.0;
        for (std::size_t q = 0; q < k; ++q) {
          const double a = e4m3_value(hA[row * k + q]), x = e4m3_value(h_B[q * n + j]);
          ref += a * x;
          scale += std::fabs(a * x);
        }
        const double bound = 1e-2 * scale + std::ldexp(1.0, -133);
        worst = std::fmax(worst, std::fabs(bf16_value(hC[row * n + j]) - ref) / bound);
      }
    }
  const bool correct = worst <= 1.0 && hv[0] == 0;
  std::cout << "Max error / (1e-2 sum|a||b|): " << worst << std::endl;
  std::cout << "Correct: " << (correct ? "yes" : "NO") << std::endl;

  // the one-kernel form on the (already pruned, so identical) dense A
  t.begin();
  rc = sm_spmma_fused_fp8(A.data().get(), Bt.data().get(), C2.data().get(), m, n, k, k, b, m * k, 0, m * n, SM_FP8_E4M3, SM_FP8_E4M3,
                          SM_OUT_BF16, 1.0f, 0.0f, nullptr, nullptr);
  const float fused_ms = t.end();
  if (rc == SM_STATUS_SUCCESS) {
    (void)hipDeviceSynchronize();
    const auto h2 = C2.to_host();
    const bool same = std::memcmp(hC.data(), h2.data(), hC.size() * sizeof(uint16_t)) == 0;
    std::cout << "Fused Time (ms): " << fused_ms << std::endl;
    std::cout << "Fused matches: " << (same ? "yes" : "NO") << std::endl;
    if (!same) return EXIT_FAILURE;
  } else {
    std::cout << "Fused: not taken for this shape (" << sm_last_error() << ")" << std::endl;
  }
  return correct ? EXIT_SUCCESS : EXIT_FAILURE;
}
