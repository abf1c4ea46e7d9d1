// quantize_fp8 m n k b -- from 16-bit operands to the fp8 2:4 product through the C ABI.  Operand roles as in
// examples/spmma_fp8.cpp: b matrices A (m x k, row-major, fp16), one shared row-major k x n fp16 B.  A is quantised per
// row and compressed in one pass (sm_quantize_compress24_fp8_f16, all b m rows as one tall matrix), B per tensor into the
// [n][k] e4m3 operand (sm_quantize_transpose_fp8_f16), and sm_spmma_fp8 multiplies with the produced row_scale.
// Prints the stage times and the largest difference to sm_spmma_fused_f16 on the same fp16 operands, relative to the
// largest |C| (the two select on different values -- quantised bytes against fp16 -- so this is the accuracy of the
// fp8 route as a whole, a few percent, not a bit comparison).
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include <sparsify.me/containers/vector.hxx>
#include <sparsify.me/util/util.hxx>
#include <sparsifyme.h>

static uint16_t f16_bits(float x) {
  const _Float16 h = static_cast<_Float16>(x);
  uint16_t u;
  std::memcpy(&u, &h, 2);
  return u;
}
static double f16_value(uint16_t u) {
  _Float16 h;
  std::memcpy(&h, &u, 2);
  return static_cast<double>(h);
}

int main(int argc, char** argv) {
  using namespace sparsifyme;
  if (argc != 5) {
    std::cout << "Invalid # of arguments. Usage: ./quantize_fp8 m n k b" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t m = std::stoi(argv[1]), n = std::stoi(argv[2]), k = std::stoi(argv[3]), b = std::stoi(argv[4]);
  const std::size_t rows = m * b;
  host_vector<uint16_t> h_A(rows * k), h_B(k * n);
  for (std::size_t i = 0; i < rows; ++i) {
    const float row_amp = util::get_random<float>(0.05f, 8.0f);  // rows of different scales: what per-row scales are for
    for (std::size_t j = 0; j < k; ++j) h_A[i * k + j] = f16_bits(row_amp * util::get_random<float>(-1.f, 1.f));
  }
  for (auto& x : h_B) x = f16_bits(util::get_random<float>(-1.f, 1.f));
  device_vector<uint16_t> A = h_A, B = h_B, C(rows * n), C16(rows * n);
  device_vector<unsigned char> Bt(k * n);
  device_vector<float> row_scale(rows);
  std::size_t bytes = 0;
  int rc = sm_compress24_size(rows, k, 1, 1, &bytes);
  device_vector<unsigned char> blob(bytes);
  const float inv_b = 448.0f;  // |b| <= 1: the per-tensor scale of B, its reciprocal goes into alpha

  util::timer_t t;
  t.begin();
  rc |= sm_quantize_transpose_fp8_f16(B.data().get(), k, n, n, inv_b, Bt.data().get(), SM_FP8_E4M3, nullptr);
  const float weight_ms = t.end();
  t.begin();
  rc |= sm_quantize_compress24_fp8_f16(A.data().get(), rows, k, k, blob.data().get(), row_scale.data().get(), SM_FP8_E4M3, nullptr);
  const float quant_ms = t.end();
  t.begin();
  rc |= sm_spmma_fp8(blob.data().get(), Bt.data().get(), C.data().get(), rows, n, k, 1, 0, rows * n, SM_FP8_E4M3, SM_FP8_E4M3, SM_OUT_F16,
                     1.0f / inv_b, 0.0f, row_scale.data().get(), nullptr);
  const float mul_ms = t.end();
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "quantize_fp8: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  t.begin();
  rc = sm_spmma_fused_f16(A.data().get(), B.data().get(), C16.data().get(), m, n, k, k, b, m * k, 0, m * n, 1.0f, 0.0f, nullptr);
  const float f16_ms = t.end();
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "quantize_fp8: sm_spmma_fused_f16: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  std::cout << "Weight Quantisation Time (ms): " << weight_ms << std::endl;
  std::cout << "Quantise + Compression Time (ms): " << quant_ms << std::endl;
  std::cout << "SpMMA Time (ms): " << mul_ms << std::endl;
  std::cout << "Fused fp16 SpMMA Time (ms): " << f16_ms << std::endl;

  (void)hipDeviceSynchronize();
  const auto h8 = C.to_host();
  const auto h16 = C16.to_host();
  double worst = 0.0, top = 0.0;
  bool finite = true;
  for (std::size_t i = 0; i < h8.size(); ++i) {
    const double x = f16_value(h8[i]), y = f16_value(h16[i]);
    finite = finite && std::isfinite(x) && std::isfinite(y);
    worst = std::fmax(worst, std::fabs(x - y));
    top = std::fmax(top, std::fabs(y));
  }
  const double rel = top > 0.0 ? worst / top : worst;
  std::cout << "Max error vs fused fp16 / max |C|: " << rel << std::endl;
  // e4m3 keeps 4 significant bits per operand: a few percent of the largest output; an order of magnitude more is a bug
  const bool ok = finite && rel < 0.25;
  std::cout << "Plausible: " << (ok ? "yes" : "NO") << std::endl;
  return ok ? EXIT_SUCCESS : EXIT_FAILURE;
}
