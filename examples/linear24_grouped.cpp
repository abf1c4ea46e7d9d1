// linear24_grouped groups hidden in tokens -- the feed-forward block of a mixture-of-experts layer on 2:4 weights: `groups` experts,
// each a fused gate/up weight W1[2 hidden][in] and a down weight W2[in][hidden], the routed tokens sorted by expert.  The stacked
// weights are pruned and compressed ONCE (spmma_plan_t::compress); then H = silu(gate) * up (spmma_plan_t::linear_glu_grouped) and
// Y = H . W2^T (spmma_plan_t::linear_grouped) are one launch each, whatever the routing: the per-expert offsets stay in device memory
// (an extension of this build: sm_linear24_grouped_*).  A seeded random routing; both results are checked against the C ABI called
// directly and against what a caller ran before -- one spmma_plan_t::linear_glu / linear per non-empty expert on that expert's own
// blob, with the counts known to the host -- bit for bit.  Exits non-zero on a miss.
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

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
  if (argc != 5) {
    std::cout << "Invalid # of arguments. Usage: ./linear24_grouped groups hidden in tokens" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t groups = std::stoul(argv[1]), hidden = std::stoul(argv[2]), in = std::stoul(argv[3]), tokens = std::stoul(argv[4]);
  if (groups == 0 || hidden % 64 != 0 || in % 64 != 0) {
    std::cout << "groups >= 1, in % 64 == 0 and hidden % 64 == 0 (hidden is the down projection's in_features)" << std::endl;
    return EXIT_FAILURE;
  }

  // a seeded random routing: every token picks an expert; sorted by expert, that is groups + 1 offsets.  One expert is left empty.
  std::mt19937 gen(0x5EED);
  std::vector<int> h_off(groups + 1, 0);
  for (std::size_t t = 0; t < tokens; ++t) {
    std::size_t g = gen() % groups;
    if (groups > 1 && g == groups / 2) g = 0;
    ++h_off[g + 1];
  }
  for (std::size_t g = 0; g < groups; ++g) h_off[g + 1] += h_off[g];

  host_vector<type_t> h_W1(groups * 2 * hidden * in), h_W2(groups * in * hidden), h_X(tokens * in);
  for (auto& w : h_W1) w = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& w : h_W2) w = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& x : h_X) x = static_cast<type_t>(util::get_random<float>() - 0.5f);
  device_vector<type_t> W1 = h_W1, W2 = h_W2, X = h_X, H(tokens * hidden), Y(tokens * in), Hc(tokens * hidden), Yc(tokens * in), Hl(tokens * hidden),
                        Yl(tokens * in);
  device_vector<int> off = h_off;
  type_t *pW1 = W1.data().get(), *pW2 = W2.data().get(), *pX = X.data().get(), *pH = H.data().get(), *pY = Y.data().get();
  type_t *pHc = Hc.data().get(), *pYc = Yc.data().get(), *pHl = Hl.data().get(), *pYl = Yl.data().get();
  const int* pOff = off.data().get();

  int rc = SM_STATUS_SUCCESS;
  auto keep_first = [&rc](int status) {
    if (rc == SM_STATUS_SUCCESS) rc = status;
  };
  // the stacked plans: m = groups * 2 hidden and m = groups * in
  spmma_plan_t<type_t> up(groups * 2 * hidden, in), down(groups * in, hidden);
  keep_first(up.compress(pW1, true));  // TILE prune in place + blob, once
  keep_first(down.compress(pW2, true));
  // every expert's own plans, from the pruned weights as they are now
  std::vector<std::unique_ptr<spmma_plan_t<type_t>>> up_g, down_g;
  for (std::size_t g = 0; g < groups; ++g) {
    up_g.emplace_back(new spmma_plan_t<type_t>(2 * hidden, in));
    down_g.emplace_back(new spmma_plan_t<type_t>(in, hidden));
    keep_first(up_g[g]->compress(pW1 + g * 2 * hidden * in));
    keep_first(down_g[g]->compress(pW2 + g * in * hidden));
  }

  util::timer_t timer;
  auto timed = [&](auto&& call) {
    call();  // warm-up
    (void)hipDeviceSynchronize();
    timer.begin();
    for (int r = 0; r < 10; ++r) call();
    (void)hipDeviceSynchronize();
    return timer.end() / 10;
  };
  const float t_grouped = timed([&] {
    keep_first(up.linear_glu_grouped(pX, pH, pOff, groups, tokens, SM_GLU_ACT_SILU));
    keep_first(down.linear_grouped(pH, pY, pOff, groups, tokens));
  });
  const float t_loop = timed([&] {
    for (std::size_t g = 0; g < groups; ++g) {
      const std::size_t lo = h_off[g], n = h_off[g + 1] - h_off[g];
      if (n == 0) continue;
      keep_first(up_g[g]->linear_glu(pX + lo * in, pHl + lo * hidden, n, SM_GLU_ACT_SILU));
      keep_first(down_g[g]->linear(pHl + lo * hidden, pYl + lo * in, n));
    }
  });
  // the C ABI called directly on the plans' blobs
  constexpr bool bf = std::is_same<type_t, __bf16>::value;
  keep_first((bf ? sm_linear24_grouped_glu_bf16 : sm_linear24_grouped_glu_f16)(up.compressed(), pX, pHc, pOff, groups, tokens, hidden, in, in, hidden,
                                                                               SM_GLU_ACT_SILU, nullptr, nullptr));
  keep_first((bf ? sm_linear24_grouped_bf16 : sm_linear24_grouped_f16)(down.compressed(), pHc, pYc, pOff, groups, tokens, in, hidden, hidden, in, 1.0f,
                                                                       0.0f, nullptr, nullptr));
  (void)hipDeviceSynchronize();
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "linear24_grouped: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  const host_vector<type_t> h_H = H.to_host(), h_Y = Y.to_host(), h_Hc = Hc.to_host(), h_Yc = Yc.to_host(), h_Hl = Hl.to_host(), h_Yl = Yl.to_host();
  auto same = [](const host_vector<type_t>& a, const host_vector<type_t>& b) { return std::memcmp(a.data(), b.data(), a.size() * sizeof(type_t)) == 0; };
  const bool abi = same(h_H, h_Hc) && same(h_Y, h_Yc);
  // the loop ran the decode form (another K order) wherever an expert had at most 16 tokens: compare only where it ran a tile form
  bool per_expert = true, any_decode = false;
  for (std::size_t g = 0; g < groups; ++g) {
    const std::size_t lo = h_off[g], n = h_off[g + 1] - h_off[g];
    if (n == 0) continue;
    if (n <= 16) {
      any_decode = true;
      continue;
    }
    per_expert = per_expert && std::memcmp(&h_H[lo * hidden], &h_Hl[lo * hidden], n * hidden * sizeof(type_t)) == 0 &&
                 std::memcmp(&h_Y[lo * in], &h_Yl[lo * in], n * in * sizeof(type_t)) == 0;
  }
  std::cout << "Grouped gate/up + down, 2 launches, Time (ms): " << t_grouped << std::endl;
  std::cout << "Per-expert loop, 2 launches per non-empty expert, Time (ms): " << t_loop << std::endl;
  std::cout << "plan.linear_glu_grouped + plan.linear_grouped equal to the C ABI bit for bit: " << (abi ? "yes" : "NO") << std::endl;
  std::cout << "... and equal to the per-expert calls bit for bit: " << (per_expert ? "yes" : "NO")
            << (any_decode ? " (experts with <= 16 tokens ran the decode form there: not compared)" : "") << std::endl;
  return abi && per_expert ? EXIT_SUCCESS : EXIT_FAILURE;
}
