// rmsnorm tokens hidden [e4m3|e5m2] -- the pre-norm in front of a W8A8 layer through the headers, without a framework op:
//     rmsnorm      h = H + D -> res_out;  n = rmsnorm(h) * gamma -> N;  n quantised per token -> Q, row_scale   (sm_rmsnorm_bf16, one launch)
//     linear24_fp8 Y[tokens][out] = (Q . W^T) with both scales, W a random fp8 2:4 compressed weight               (sm_linear24_fp8)
// bfloat16 operands from the integer class (|H| <= 8, |D| <= 7, |gamma| <= 4: every partial sum of the squares is an exact fp32 integer
// in any order, so the host's fp32 evaluation of the definition is the definition).  Checked on the host: res_out and N bit for bit; the
// layer's output bit for bit against the same layer fed by sm_quantize_rows_fp8_bf16 of N.  Exits non-zero on a miss.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <sparsify.me/spmma.hxx>
#include <sparsify.me/util/util.hxx>

static float bf16_to_float(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// round to nearest even (finite inputs)
static uint16_t float_to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

int main(int argc, char** argv) {
  using namespace sparsifyme;
  if (argc != 3 && argc != 4) {
    std::cout << "Invalid # of arguments. Usage: ./rmsnorm tokens hidden [e4m3|e5m2]" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t tokens = std::stoul(argv[1]), hidden = std::stoul(argv[2]), out = 128;
  const std::string how = argc == 4 ? argv[3] : "e4m3";
  if (tokens == 0 || hidden == 0 || hidden % 64 != 0 || hidden > SM_RMSNORM_MAX_HIDDEN || (how != "e4m3" && how != "e5m2")) {
    std::cout << "tokens >= 1, hidden a multiple of 64 (the layer's rule) up to " << SM_RMSNORM_MAX_HIDDEN << ", format e4m3 or e5m2" << std::endl;
    return EXIT_FAILURE;
  }
  const int fmt = how == "e4m3" ? SM_FP8_E4M3 : SM_FP8_E5M2;
  const float eps = 1e-6f;

  std::vector<uint16_t> h_H(tokens * hidden), h_D(tokens * hidden), h_g(hidden), h_W(out * hidden);
  auto integer = [](int lim) { return float_to_bf16(std::floor(util::get_random<float>() * (2 * lim + 1)) - lim); };
  for (auto& x : h_H) x = integer(8);
  for (auto& x : h_D) x = integer(7);
  for (auto& x : h_g) x = integer(4);
  for (auto& x : h_W) x = float_to_bf16(util::get_random<float>() - 0.5f);

  std::size_t blob_bytes = 0;
  if (sm_compress24_size(out, hidden, 1, 1, &blob_bytes) != SM_STATUS_SUCCESS) return EXIT_FAILURE;
  __bf16 *H = nullptr, *D = nullptr, *g = nullptr, *res = nullptr, *N = nullptr, *W = nullptr, *Y = nullptr, *Y2 = nullptr;
  void *blob = nullptr, *Q = nullptr, *Q2 = nullptr;
  float *w_scale = nullptr, *x_scale = nullptr, *x_scale2 = nullptr;
  const std::size_t nb = tokens * hidden * 2;
  const bool alloc = hipMalloc((void**)&H, nb) == hipSuccess && hipMalloc((void**)&D, nb) == hipSuccess && hipMalloc((void**)&g, hidden * 2) == hipSuccess &&
                     hipMalloc((void**)&res, nb) == hipSuccess && hipMalloc((void**)&N, nb) == hipSuccess && hipMalloc((void**)&W, out * hidden * 2) == hipSuccess &&
                     hipMalloc((void**)&Y, tokens * out * 2) == hipSuccess && hipMalloc((void**)&Y2, tokens * out * 2) == hipSuccess &&
                     hipMalloc(&blob, blob_bytes) == hipSuccess && hipMalloc(&Q, tokens * hidden) == hipSuccess && hipMalloc(&Q2, tokens * hidden) == hipSuccess &&
                     hipMalloc((void**)&w_scale, out * 4) == hipSuccess && hipMalloc((void**)&x_scale, tokens * 4) == hipSuccess &&
                     hipMalloc((void**)&x_scale2, tokens * 4) == hipSuccess;
  if (!alloc) {
    std::cerr << "rmsnorm: out of device memory" << std::endl;
    return EXIT_FAILURE;
  }
  (void)hipMemcpy(H, h_H.data(), nb, hipMemcpyHostToDevice);
  (void)hipMemcpy(D, h_D.data(), nb, hipMemcpyHostToDevice);
  (void)hipMemcpy(g, h_g.data(), hidden * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(W, h_W.data(), out * hidden * 2, hipMemcpyHostToDevice);

  int rc = SM_STATUS_SUCCESS;
  auto keep_first = [&rc](int status) {
    if (rc == SM_STATUS_SUCCESS) rc = status;
  };
  keep_first(sm_quantize_compress24_fp8_bf16(W, out, hidden, hidden, blob, w_scale, SM_FP8_E4M3, nullptr));  // once per weight
  // the fused front: add + norm + quantise, one launch; then the layer
  keep_first(rmsnorm<__bf16>(H, D, g, res, N, tokens, hidden, eps, Q, x_scale, fmt));
  keep_first(sm_linear24_fp8(blob, Q, Y, tokens, out, hidden, hidden, out, SM_FP8_E4M3, fmt, SM_OUT_BF16, 1.0f, 0.0f, w_scale, x_scale, nullptr, nullptr));
  // the same layer fed by the quantiser's pass over N
  keep_first(sm_quantize_rows_fp8_bf16(N, tokens, hidden, hidden, Q2, hidden, x_scale2, fmt, nullptr));
  keep_first(sm_linear24_fp8(blob, Q2, Y2, tokens, out, hidden, hidden, out, SM_FP8_E4M3, fmt, SM_OUT_BF16, 1.0f, 0.0f, w_scale, x_scale2, nullptr, nullptr));
  int form = SM_RMSNORM_FORM_INVALID;
  keep_first(sm_rmsnorm_form(hidden, &form));
  if (hipDeviceSynchronize() != hipSuccess) keep_first(SM_STATUS_LAUNCH_FAILED);
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "rmsnorm: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  std::vector<uint16_t> d_res(tokens * hidden), d_N(tokens * hidden), d_Y(tokens * out), d_Y2(tokens * out);
  (void)hipMemcpy(d_res.data(), res, nb, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_N.data(), N, nb, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_Y.data(), Y, tokens * out * 2, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_Y2.data(), Y2, tokens * out * 2, hipMemcpyDeviceToHost);

  std::size_t bad_res = 0, bad_n = 0;
  for (std::size_t t = 0; t < tokens; ++t) {
    float S = 0.0f;  // exact: integers, 225 * hidden < 2^24
    for (std::size_t j = 0; j < hidden; ++j) {
      const uint16_t h = float_to_bf16(bf16_to_float(h_H[t * hidden + j]) + bf16_to_float(h_D[t * hidden + j]));
      bad_res += h != d_res[t * hidden + j];
      S += bf16_to_float(h) * bf16_to_float(h);
    }
    const float ms = S / (float)hidden;
    const float r = 1.0f / std::sqrt(ms + eps);
    for (std::size_t j = 0; j < hidden; ++j) {
      const float hr = bf16_to_float(d_res[t * hidden + j]) * r;
      bad_n += float_to_bf16(hr * bf16_to_float(h_g[j])) != d_N[t * hidden + j];
    }
  }
  const bool layer_ok = d_Y == d_Y2;

  std::cout << "add + RMSNorm + " << how << ": " << tokens << " tokens, hidden " << hidden << ", form " << (form == SM_RMSNORM_FORM_LANES ? "lanes" : "block")
            << ", then linear24_fp8 to " << out << " features" << std::endl;
  std::cout << "res_out equal to the rounded fp32 add: " << (bad_res ? "NO" : "yes") << std::endl;
  std::cout << "N equal to the definition evaluated on the host: " << (bad_n ? "NO" : "yes") << std::endl;
  std::cout << "layer output equal to the layer fed by quantize_rows_fp8 of N: " << (layer_ok ? "yes" : "NO") << std::endl;
  for (void* p : {(void*)H, (void*)D, (void*)g, (void*)res, (void*)N, (void*)W, (void*)Y, (void*)Y2, blob, Q, Q2, (void*)w_scale, (void*)x_scale, (void*)x_scale2})
    (void)hipFree(p);
  return !bad_res && !bad_n && layer_ok ? EXIT_SUCCESS : EXIT_FAILURE;
}
