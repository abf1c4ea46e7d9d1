// linear24_headers [dump] -- spmma_plan_t<T>::linear (include/sparsify.me/spmma.hxx), with and without an epilogue, fp16 and
// bfloat16, against the three-call route through the same headers: transpose X, plan.multiply with W as A (SM_BIAS_ROW for the
// per-out-feature bias), transpose the result -- bit for bit (every case here runs the tile form: tokens > 16).  Also the error
// behaviour: a plan that is not compressed, or has a batch, returns SM_STATUS_INVALID_VALUE and does not throw.
// With a path argument the fp16 case's tokens, out, in (int64) and W (pruned), X, Y are written there for the Python side.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include <sparsify.me/containers/vector.hxx>
#include <sparsify.me/spmma.hxx>
#include <sparsify.me/util/util.hxx>

using namespace sparsifyme;

template <typename type_t>
static bool same_bits(const host_vector<type_t>& a, const host_vector<type_t>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(type_t)) == 0;
}

template <typename type_t>
static int run(const char* name, const char* dump) {
  const std::size_t tokens = 77, out = 328, in = 192;
  host_vector<type_t> h_W(out * in), h_X(tokens * in), h_R(tokens * out);
  host_vector<float> h_bias(out);
  for (auto& w : h_W) w = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& x : h_X) x = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& r : h_R) r = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& v : h_bias) v = util::get_random<float>() - 0.5f;
  device_vector<type_t> W = h_W, X = h_X, R = h_R, Y(tokens * out), Xt(in * tokens), C(out * tokens), Rt(out * tokens), Yr(tokens * out);
  device_vector<float> bias = h_bias;
  type_t *pX = X.data().get(), *pY = Y.data().get(), *pXt = Xt.data().get(), *pC = C.data().get(), *pYr = Yr.data().get();

  int fails = 0;
  auto expect = [&](bool ok, const char* what) {
    if (!ok) {
      std::cerr << name << ": " << what << " FAILED (" << sm_last_error() << ")" << std::endl;
      ++fails;
    }
  };
  spmma_plan_t<type_t> plan(out, in), batched(out, in, 2);
  expect(plan.linear(pX, pY, tokens) == SM_STATUS_INVALID_VALUE, "linear() before compress() is refused");
  expect(plan.compress(W.data().get(), true) == SM_STATUS_SUCCESS, "compress");
  expect(sm_transpose(pX, pXt, tokens, in, in, tokens, sizeof(type_t), 1, 0, 0, nullptr) == SM_STATUS_SUCCESS, "transpose X");
  expect(sm_transpose(R.data().get(), Rt.data().get(), tokens, out, out, tokens, sizeof(type_t), 1, 0, 0, nullptr) == SM_STATUS_SUCCESS, "transpose R");

  // plain
  expect(plan.linear(pX, pY, tokens) == SM_STATUS_SUCCESS, "linear");
  expect(plan.multiply(pXt, pC, tokens) == SM_STATUS_SUCCESS, "multiply");
  expect(sm_transpose(pC, pYr, out, tokens, tokens, out, sizeof(type_t), 1, 0, 0, nullptr) == SM_STATUS_SUCCESS, "transpose C");
  (void)hipDeviceSynchronize();
  const host_vector<type_t> h_Y = Y.to_host();
  expect(same_bits(h_Y, Yr.to_host()), "linear == transpose + multiply + transpose");

  // bias per out feature + residual + ReLU
  spmma_epilogue_t mine, theirs;
  mine.bias = bias.data().get();
  mine.bias_dim = SM_BIAS_COL;
  mine.act = SM_ACT_RELU;
  mine.residual = R.data().get();
  theirs = mine;
  theirs.bias_dim = SM_BIAS_ROW;
  theirs.residual = Rt.data().get();
  device_vector<type_t> Y2(tokens * out);
  expect(plan.linear(pX, Y2.data().get(), tokens, mine, 1.5f, 0.5f) == SM_STATUS_SUCCESS, "linear with an epilogue");
  expect(plan.multiply(pXt, pC, tokens, theirs, 1.5f, 0.5f) == SM_STATUS_SUCCESS, "multiply with an epilogue");
  expect(sm_transpose(pC, pYr, out, tokens, tokens, out, sizeof(type_t), 1, 0, 0, nullptr) == SM_STATUS_SUCCESS, "transpose D");
  (void)hipDeviceSynchronize();
  expect(same_bits(Y2.to_host(), Yr.to_host()), "linear with an epilogue == the route with the epilogue transposed");

  // a plan with a batch is not a linear layer's weight
  device_vector<type_t> W2(2 * out * in);
  expect(batched.compress(W2.data().get()) == SM_STATUS_SUCCESS, "compress (batch 2)");
  expect(batched.linear(pX, pY, tokens) == SM_STATUS_INVALID_VALUE, "linear() on a batched plan is refused");

  if (dump) {
    const host_vector<type_t> h_Wp = W.to_host();  // pruned in place by compress()
    FILE* f = std::fopen(dump, "wb");
    if (!f) return fails + 1;
    const std::int64_t dims[3] = {(std::int64_t)tokens, (std::int64_t)out, (std::int64_t)in};
    std::fwrite(dims, sizeof(dims), 1, f);
    std::fwrite(h_Wp.data(), sizeof(type_t), h_Wp.size(), f);
    std::fwrite(h_X.data(), sizeof(type_t), h_X.size(), f);
    std::fwrite(h_Y.data(), sizeof(type_t), h_Y.size(), f);
    std::fclose(f);
  }
  return fails;
}

int main(int argc, char** argv) {
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "no gfx950 device: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  int fails = run<_Float16>("fp16", argc > 1 ? argv[1] : nullptr);
  fails += run<__bf16>("bf16", nullptr);
  if (fails == 0) std::cout << "linear24_headers ok" << std::endl;
  return fails ? EXIT_FAILURE : EXIT_SUCCESS;
}
