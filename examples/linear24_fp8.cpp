// linear24_fp8 out in tokens [reps] -- the W8A8 2:4 weight-sparse linear layer, token-major: a random 16-bit weight W[out][in] is
// quantised per output channel and compressed ONCE (sm_quantize_compress24_fp8_f16), random tokens are quantised per row
// (sm_quantize_rows_fp8_f16), and the layer runs in one launch (sm_linear24_fp8: Y[tokens][out] bf16, both scales applied in the
// store).  Checked on the device data against the route a caller ran before -- sm_spmma_fp8 (C[out][tokens], fp32, row_scale =
// w_scale) + sm_transpose, the token scale applied on the host.  A tile form has the route's accumulator; its fp32 value differs from
// the route's times x_scale[t] by the order of two multiplies only, so Y lies within half a bf16 ulp (at most |r| / 256) plus 4 fp32
// ulps of it.  The decode form adds its K slices in another order and is held to the accumulation bound on top.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include <sparsifyme.h>
#include <sparsify.me/util/timer.hxx>
#include <sparsify.me/util/util.hxx>

static float bf16_to_float(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int main(int argc, char** argv) {
  using namespace sparsifyme;
  if (argc != 4 && argc != 5) {
    std::cout << "Invalid # of arguments. Usage: ./linear24_fp8 out in tokens [reps]" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t out = std::stoul(argv[1]), in = std::stoul(argv[2]), tokens = std::stoul(argv[3]);
  const int reps = argc == 5 ? std::stoi(argv[4]) : 10;
  if (out % 2 != 0) {
    std::cerr << "linear24_fp8: the route it checks against (sm_spmma_fp8) needs an even out" << std::endl;
    return EXIT_FAILURE;
  }

  std::vector<_Float16> h_W(out * in), h_X(tokens * in);
  for (auto& w : h_W) w = static_cast<_Float16>(util::get_random<float>() - 0.5f);
  for (auto& x : h_X) x = static_cast<_Float16>(util::get_random<float>() - 0.5f);
  std::size_t blob_bytes = 0;
  if (sm_compress24_size(out, in, 1, 1, &blob_bytes) != SM_STATUS_SUCCESS) return EXIT_FAILURE;
  void *W = nullptr, *X = nullptr, *blob = nullptr, *Q = nullptr, *Y = nullptr, *C = nullptr, *Ct = nullptr;
  float *w_scale = nullptr, *x_scale = nullptr;
  bool alloc = hipMalloc(&W, out * in * 2) == hipSuccess && hipMalloc(&X, tokens * in * 2) == hipSuccess && hipMalloc(&blob, blob_bytes) == hipSuccess &&
               hipMalloc(&Q, tokens * in) == hipSuccess && hipMalloc(&Y, tokens * out * 2) == hipSuccess && hipMalloc(&C, out * tokens * 4) == hipSuccess &&
               hipMalloc(&Ct, tokens * out * 4) == hipSuccess && hipMalloc((void**)&w_scale, out * 4) == hipSuccess &&
               hipMalloc((void**)&x_scale, tokens * 4) == hipSuccess;
  if (!alloc) {
    std::cerr << "linear24_fp8: out of device memory" << std::endl;
    return EXIT_FAILURE;
  }
  (void)hipMemcpy(W, h_W.data(), out * in * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(X, h_X.data(), tokens * in * 2, hipMemcpyHostToDevice);

  int rc = SM_STATUS_SUCCESS;
  auto keep_first = [&rc](int status) {
    if (rc == SM_STATUS_SUCCESS) rc = status;
  };
  util::timer_t timer;
  timer.begin();
  keep_first(sm_quantize_compress24_fp8_f16(W, out, in, in, blob, w_scale, SM_FP8_E4M3, nullptr));  // once per weight
  (void)hipDeviceSynchronize();
  const float t_compress = timer.end();
  timer.begin();
  keep_first(sm_quantize_rows_fp8_f16(X, tokens, in, in, Q, in, x_scale, SM_FP8_E4M3, nullptr));
  (void)hipDeviceSynchronize();
  const float t_quant = timer.end();

  auto linear = [&] {
    keep_first(sm_linear24_fp8(blob, Q, Y, tokens, out, in, in, out, SM_FP8_E4M3, SM_FP8_E4M3, SM_OUT_BF16, 1.0f, 0.0f, w_scale, x_scale, nullptr, nullptr));
  };
  auto route = [&] {
    keep_first(sm_spmma_fp8(blob, Q, C, out, tokens, in, 1, 0, out * tokens, SM_FP8_E4M3, SM_FP8_E4M3, SM_OUT_F32, 1.0f, 0.0f, w_scale, nullptr));
    keep_first(sm_transpose(C, Ct, out, tokens, tokens, out, 4, 1, 0, 0, nullptr));
  };
  auto timed = [&](auto&& call) {
    call();  // warm-up
    (void)hipDeviceSynchronize();
    timer.begin();
    for (int r = 0; r < reps; ++r) call();
    (void)hipDeviceSynchronize();
    return timer.end() / (reps > 0 ? reps : 1);
  };
  const float t_linear = timed(linear), t_route = timed(route);
  int form = SM_LINEAR24_FORM_NOT_TAKEN;
  keep_first(sm_linear24_fp8_form(tokens, out, in, 0, &form));
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "linear24_fp8: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  std::vector<uint16_t> h_Y(tokens * out);
  std::vector<float> h_Ct(tokens * out), h_xs(tokens);
  (void)hipMemcpy(h_Y.data(), Y, tokens * out * 2, hipMemcpyDeviceToHost);
  (void)hipMemcpy(h_Ct.data(), Ct, tokens * out * 4, hipMemcpyDeviceToHost);
  (void)hipMemcpy(h_xs.data(), x_scale, tokens * 4, hipMemcpyDeviceToHost);
  const bool exact = form != SM_LINEAR24_FORM_DECODE;
  std::size_t bad = 0;
  for (std::size_t t = 0; t < tokens; ++t)
    for (std::size_t o = 0; o < out; ++o) {
      // the route's fp32 value is (1 * w_scale[o]) * acc, one rounding; the layer's is ((1 * w_scale[o]) * x_scale[t]) * acc, one
      // rounding: they differ by the order of two multiplies, i.e. by at most 2 ulp of fp32 before the bf16 rounding
      const float r = h_Ct[t * out + o] * h_xs[t], y = bf16_to_float(h_Y[t * out + o]);
      // the decode form's other K order: |w|, |x| <= 0.5 before quantisation, half of W kept: sum |w x| <= in / 8 (+ quantisation slack)
      // half a bf16 ulp is at most |r| * 2^-8 (8 significand bits)
      const double tol = std::fabs((double)r) * (std::ldexp(1.0, -8) + 4 * std::ldexp(1.0, -24)) + (exact ? 0.0 : 2.0 * in * std::ldexp(1.0, -24) * (in / 8.0) * 1.25);
      bad += !(std::fabs((double)y - (double)r) <= tol) && !(y != y && r != r);
    }
  std::cout << "Quantise + Compress Time (ms): " << t_compress << std::endl;
  std::cout << "Quantise Tokens Time (ms): " << t_quant << std::endl;
  std::cout << "Linear fp8 2:4 Time (ms): " << t_linear << std::endl;
  std::cout << "SpMMA fp8 + Transpose Time (ms): " << t_route << std::endl;
  std::cout << "linear == the route with the token scale applied on the host (within one bf16 rounding): " << (bad ? "NO" : "yes") << std::endl;
  for (void* p : {W, X, blob, Q, Y, C, Ct, (void*)w_scale, (void*)x_scale}) (void)hipFree(p);
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
