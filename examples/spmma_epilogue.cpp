// spmma_epilogue m n k b [reps] -- the layer activation(conv(x) + bias [+ shortcut]) in the store of the fused 2:4 matmul
// (sparsifyme::spmma_fused with a spmma_epilogue_t, an extension of this build: sm_spmma_fused_*_ex).  Prints the time of the
// plain fused call, of the call with bias + ReLU, and of the call with bias + residual + ReLU, and checks on the device data
// that ReLU in the epilogue is max(plain result, 0) bit for bit (ReLU commutes with the one rounding).
#include <cstdlib>
#include <iostream>
#include <string>

#include <sparsify.me/containers/vector.hxx>
#include <sparsify.me/spmma.hxx>
#include <sparsify.me/util/util.hxx>

#ifndef SM_TYPE
#define SM_TYPE _Float16
#endif

int main(int argc, char** argv) {
  using namespace sparsifyme;
  using type_t = SM_TYPE;
  if (argc != 5 && argc != 6) {
    std::cout << "Invalid # of arguments. Usage: ./spmma_epilogue m n k b [reps]" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t m = std::stoi(argv[1]), n = std::stoi(argv[2]), k = std::stoi(argv[3]), b = std::stoi(argv[4]);
  const int reps = argc == 6 ? std::stoi(argv[5]) : 10;

  host_vector<type_t> h_A(m * k * b), h_B(k * n * b), h_R(m * n * b);
  host_vector<float> h_bias(n);
  for (auto& a : h_A) a = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& x : h_B) x = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& r : h_R) r = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& v : h_bias) v = util::get_random<float>() - 0.5f;
  device_vector<type_t> A = h_A, B = h_B, R = h_R, C(m * n * b), D(m * n * b);
  device_vector<float> bias = h_bias;

  spmma_epilogue_t relu, bias_relu, bias_res_relu;
  relu.act = SM_ACT_RELU;
  bias_relu.bias = bias.data().get();
  bias_relu.act = SM_ACT_RELU;
  bias_res_relu = bias_relu;
  bias_res_relu.residual = R.data().get();

  auto timed = [&](auto&& call) {
    call();  // warm-up
    float ms = 0.0f;
    for (int r = 0; r < reps; ++r) ms += call();
    return ms / (reps > 0 ? reps : 1);
  };
  type_t *pA = A.data().get(), *pB = B.data().get(), *pC = C.data().get(), *pD = D.data().get();
  const float t_plain = timed([&] { return spmma_fused(pA, pB, pC, m, n, k, b); });
  const float t_bias_relu = timed([&] { return spmma_fused(pA, pB, pD, m, n, k, b, bias_relu); });
  const float t_res = timed([&] { return spmma_fused(pA, pB, pD, m, n, k, b, bias_res_relu, 1.0f, 1.0f); });

  // ReLU alone against the plain result
  (void)spmma_fused(pA, pB, pD, m, n, k, b, relu);
  (void)hipDeviceSynchronize();
  const host_vector<type_t> h_C = C.to_host(), h_D = D.to_host();
  bool same = true;
  for (std::size_t i = 0; i < h_C.size() && same; ++i) {
    const float c = static_cast<float>(h_C[i]), d = static_cast<float>(h_D[i]);
    same = (c != c) ? (d != d) : (d == (c > 0.0f ? c : 0.0f));
  }
  std::cout << "Fused SpMMA Time (ms): " << t_plain << std::endl;
  std::cout << "Fused SpMMA + bias + ReLU Time (ms): " << t_bias_relu << std::endl;
  std::cout << "Fused SpMMA + bias + residual + ReLU Time (ms): " << t_res << std::endl;
  std::cout << "ReLU epilogue == max(plain, 0): " << (same ? "yes" : "NO") << std::endl;
  return same ? EXIT_SUCCESS : EXIT_FAILURE;
}
