// linear24_glu hidden in tokens -- the gated (SwiGLU) form of the 2:4 weight-sparse linear layer: the fused gate/up weight
// W[2 hidden][in] is pruned and compressed ONCE (spmma_plan_t::compress), then Y[tokens][hidden] = silu(gate) * up comes out of one
// launch (spmma_plan_t::linear_glu, an extension of this build: sm_linear24_glu_*).  Checks it against what a caller ran before --
// spmma_plan_t::linear on the same blob, which writes [tokens][2 hidden], plus a SwiGLU pass of its own (here on the host, in double)
// -- and exits non-zero on a miss.
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
  if (argc != 4) {
    std::cout << "Invalid # of arguments. Usage: ./linear24_glu hidden in tokens" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t hidden = std::stoul(argv[1]), in = std::stoul(argv[2]), tokens = std::stoul(argv[3]);
  const std::size_t out = 2 * hidden;

  host_vector<type_t> h_W(out * in), h_X(tokens * in);
  for (auto& w : h_W) w = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& x : h_X) x = static_cast<type_t>(util::get_random<float>() - 0.5f);
  device_vector<type_t> W = h_W, X = h_X, Y(tokens * hidden), Yw(tokens * out);
  type_t *pW = W.data().get(), *pX = X.data().get(), *pY = Y.data().get(), *pYw = Yw.data().get();

  int rc = SM_STATUS_SUCCESS;
  auto keep_first = [&rc](int status) {
    if (rc == SM_STATUS_SUCCESS) rc = status;
  };
  util::timer_t timer;
  spmma_plan_t<type_t> plan(out, in);
  keep_first(plan.compress(pW, true));  // TILE prune in place + blob, once
  auto timed = [&](auto&& call) {
    call();  // warm-up
    (void)hipDeviceSynchronize();
    timer.begin();
    for (int r = 0; r < 10; ++r) call();
    (void)hipDeviceSynchronize();
    return timer.end() / 10;
  };
  const float t_glu = timed([&] { keep_first(plan.linear_glu(pX, pY, tokens, SM_GLU_ACT_SILU)); });
  const float t_wide = timed([&] { keep_first(plan.linear(pX, pYw, tokens)); });
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "linear24_glu: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  // The reference reads g and u AFTER their rounding to the 16-bit type (relative error ROUND each); y is rounded once.  With
  // |silu'| <= 1.1:  |y - silu(g16) u16| <= ROUND |y| + 1.1 ROUND |g| |u| + |silu(g)| ROUND |u| + 6 * 2^-24 |y|, the last term the
  // fp32 gate and multiply; the 16-bit values stand for the exact ones at a cost below (1 + ROUND)^2 < 1.01.
  const host_vector<type_t> h_Y = Y.to_host(), h_Yw = Yw.to_host();
  const double round = std::is_same<type_t, __bf16>::value ? 1.0 / 256 : 1.0 / 2048;
  std::size_t bad = 0;
  double worst = 0.0;
  for (std::size_t t = 0; t < tokens; ++t)
    for (std::size_t h = 0; h < hidden; ++h) {
      const double g = static_cast<float>(h_Yw[t * out + h]), u = static_cast<float>(h_Yw[t * out + hidden + h]);
      const double a = g / (1.0 + std::exp(-g)), ref = a * u, y = static_cast<float>(h_Y[t * hidden + h]);
      const double tol = 1.01 * (round * std::fabs(ref) + 1.1 * round * std::fabs(g * u) + round * std::fabs(a * u) + 6 * std::ldexp(1.0, -24) * std::fabs(ref)) +
                         std::ldexp(1.0, -24);
      const double ratio = std::fabs(y - ref) / tol;
      worst = ratio > worst ? ratio : worst;
      bad += !(ratio <= 1.0);
    }
  std::cout << "Gated linear 2:4 Time (ms): " << t_glu << std::endl;
  std::cout << "Linear 2:4 [tokens][2 hidden] Time (ms): " << t_wide << std::endl;
  std::cout << "linear_glu == linear + host SwiGLU within the rounding bound (worst err / bound " << worst << "): " << (bad ? "NO" : "yes") << std::endl;
  return bad ? EXIT_FAILURE : EXIT_SUCCESS;
}
