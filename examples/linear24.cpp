// linear24 out in tokens [reps] -- a 2:4 weight-sparse linear layer, token-major: Y[tokens][out] = X[tokens][in] . W^T with
// W[out][in] pruned and compressed ONCE (spmma_plan_t::compress) and multiplied by fresh activations on every call
// (spmma_plan_t::linear, an extension of this build: sm_linear24_*).  Checks the result on the device data against the route a
// caller ran before -- sm_transpose(X) + the 2:4 matmul with W as A + sm_transpose(C) -- bit for bit where the tile form runs
// (tokens > 16 or out > 16384) and within the fp32-accumulation bound where the decode form runs, and prints the stage times.
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <string>
#include <type_traits>

#include <sparsify.me/containers/vector.hxx>
#include <sparsify.me/spmma.hxx>
#include <sparsify.me/util/timer.hxx>
#include <sparsify.me/util/util.hxx>

#ifndef SM_TYPE
#define SM_TYPE _Float16
#endif

int main(int argc, char** argv) {
  using namespace sparsifyme;
  using type_t = SM_TYPE;
  if (argc != 4 && argc != 5) {
    std::cout << "Invalid # of arguments. Usage: ./linear24 out in tokens [reps]" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t out = std::stoul(argv[1]), in = std::stoul(argv[2]), tokens = std::stoul(argv[3]);
  const int reps = argc == 5 ? std::stoi(argv[4]) : 10;

  host_vector<type_t> h_W(out * in), h_X(tokens * in);
  for (auto& w : h_W) w = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& x : h_X) x = static_cast<type_t>(util::get_random<float>() - 0.5f);
  device_vector<type_t> W = h_W, X = h_X, Y(tokens * out), Xt(in * tokens), C(out * tokens), Yr(tokens * out);
  type_t *pW = W.data().get(), *pX = X.data().get(), *pY = Y.data().get(), *pXt = Xt.data().get(), *pC = C.data().get(), *pYr = Yr.data().get();

  int rc = SM_STATUS_SUCCESS;
  auto keep_first = [&rc](int status) {
    if (rc == SM_STATUS_SUCCESS) rc = status;
  };
  util::timer_t timer;
  spmma_plan_t<type_t> plan(out, in);
  timer.begin();
  keep_first(plan.compress(pW, true));  // TILE prune in place + blob, once
  (void)hipDeviceSynchronize();
  const float t_compress = timer.end();

  auto linear = [&] { keep_first(plan.linear(pX, pY, tokens)); };
  auto route = [&] {
    keep_first(sm_transpose(pX, pXt, tokens, in, in, tokens, sizeof(type_t), 1, 0, 0, nullptr));
    keep_first(plan.multiply(pXt, pC, tokens));
    keep_first(sm_transpose(pC, pYr, out, tokens, tokens, out, sizeof(type_t), 1, 0, 0, nullptr));
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
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "linear24: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  const host_vector<type_t> h_Y = Y.to_host(), h_Yr = Yr.to_host();
  const bool exact = tokens > 16 || out > 16384;  // the tile form; the decode form adds its K slices in another order
  const double round = sizeof(type_t) == 2 && std::is_same<type_t, __bf16>::value ? 1.0 / 256 : 1.0 / 2048;
  std::size_t bad = 0;
  for (std::size_t i = 0; i < h_Y.size(); ++i) {
    const double y = static_cast<float>(h_Y[i]), r = static_cast<float>(h_Yr[i]);
    if (exact) bad += !(y == r || (y != y && r != r));
    // |w|, |x| <= 0.5, half of W kept: sum |w x| <= in / 8; both sides are within ROUND |ref| + 2 in 2^-24 sum |w x| of the exact product
    else bad += !(std::fabs(y - r) <= 2 * (round * std::fabs(r) + 2.0 * in * std::ldexp(1.0, -24) * (in / 8.0)));
  }
  std::cout << "Compress Time (ms): " << t_compress << std::endl;
  std::cout << "Linear 2:4 Time (ms): " << t_linear << std::endl;
  std::cout << "Transpose + SpMMA + Transpose Time (ms): " << t_route << std::endl;
  std::cout << "linear == the three-call route (" << (exact ? "bit for bit" : "within the accumulation bound") << "): " << (bad ? "NO" : "yes") << std::endl;
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
