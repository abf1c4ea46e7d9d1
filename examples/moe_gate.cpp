// moe_gate experts tokens top_k [softmax|sigmoid] -- the head of a mixture-of-experts block through the headers, without a framework op:
//     moe_gate    logits[tokens][experts] -> topk_ids, topk_weights (renormalised over the top_k)   (sm_moe_gate_*, one launch)
//     moe_route   topk_ids -> offsets, sorted_token, sorted_pair, pair_pos                            (sm_moe_route)
// Seeded logits in the 16-bit type (so equal logits do occur).  Checked on the host: the ids against a stable partial sort (descending
// logit, equal logits in ascending expert index), the weights against an fp64 evaluation of the definition within
// (top_k + D + 11) * 2^-24 relative, D the row's largest |x - m| (include/sparsifyme.h), the route's offsets against a
// count of the ids.  Exits non-zero on a miss.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <numeric>
#include <string>
#include <vector>

#include <sparsify.me/containers/vector.hxx>
#include <sparsify.me/spmma.hxx>
#include <sparsify.me/util/util.hxx>

#ifndef SM_TYPE
#define SM_TYPE _Float16
#endif

int main(int argc, char** argv) {
  using namespace sparsifyme;
  using type_t = SM_TYPE;
  if (argc != 4 && argc != 5) {
    std::cout << "Invalid # of arguments. Usage: ./moe_gate experts tokens top_k [softmax|sigmoid]" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t experts = std::stoul(argv[1]), tokens = std::stoul(argv[2]), top_k = std::stoul(argv[3]);
  const std::string how = argc == 5 ? argv[4] : "softmax";
  if (top_k == 0 || top_k > experts || top_k > SM_MOE_GATE_MAX_TOP_K || experts > SM_LINEAR24_MAX_GROUPS || tokens == 0 ||
      (how != "softmax" && how != "sigmoid")) {
    std::cout << "1 <= top_k <= min(experts, " << SM_MOE_GATE_MAX_TOP_K << "), experts <= " << SM_LINEAR24_MAX_GROUPS
              << ", tokens >= 1, scoring softmax or sigmoid" << std::endl;
    return EXIT_FAILURE;
  }
  const int scoring = how == "softmax" ? SM_MOE_SCORE_SOFTMAX : SM_MOE_SCORE_SIGMOID;
  const std::size_t P = tokens * top_k;

  host_vector<type_t> h_logits(tokens * experts);
  for (auto& x : h_logits) x = static_cast<type_t>(8.0f * (util::get_random<float>() - 0.5f));
  device_vector<type_t> logits = h_logits;
  device_vector<int> ids(P), off(experts + 1), s_token(P), s_pair(P), pos(P);
  device_vector<float> w(P);
  device_vector<unsigned char> ws(std::max<std::size_t>(moe_route_workspace(tokens, top_k, experts), 16));

  int rc = moe_gate<type_t>(logits.data().get(), ids.data().get(), w.data().get(), tokens, experts, top_k, scoring);
  if (rc == SM_STATUS_SUCCESS)
    rc = moe_route(ids.data().get(), tokens, top_k, experts, off.data().get(), s_token.data().get(), s_pair.data().get(), pos.data().get(), ws.data().get(),
                   ws.size());
  (void)hipDeviceSynchronize();
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "moe_gate: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  const host_vector<int> d_ids = ids.to_host(), d_off = off.to_host();
  const host_vector<float> d_w = w.to_host();
  bool ids_ok = true, w_ok = true;
  double worst = 0.0;  // the largest error as a share of its bound
  std::vector<int> order(experts);
  for (std::size_t t = 0; t < tokens; ++t) {
    const type_t* row = &h_logits[t * experts];
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return static_cast<float>(row[a]) > static_cast<float>(row[b]); });
    for (std::size_t j = 0; j < top_k; ++j) ids_ok = ids_ok && d_ids[t * top_k + j] == order[j];
    // the definition in fp64 at the host's ids; D over the whole row
    const double m = static_cast<double>(row[order[0]]);
    double D = 0.0, S = 0.0;
    for (std::size_t e = 0; e < experts; ++e) D = std::max(D, std::fabs(static_cast<double>(row[e]) - m));
    std::vector<double> v(top_k);
    for (std::size_t j = 0; j < top_k; ++j) {
      const double x = static_cast<double>(row[order[j]]);
      v[j] = scoring == SM_MOE_SCORE_SOFTMAX ? std::exp(x - m) : 1.0 / (1.0 + std::exp(-x));
      S += v[j];
    }
    const double bound = (double)(top_k + 11) + D;
    for (std::size_t j = 0; j < top_k; ++j) {
      const double want = v[j] / S, rel = std::fabs((double)d_w[t * top_k + j] - want) / want * 16777216.0 / bound;
      worst = std::max(worst, rel);
      w_ok = w_ok && rel <= 1.0;
    }
  }
  std::vector<int> count(experts + 1, 0);
  for (std::size_t p = 0; p < P; ++p)
    if (d_ids[p] >= 0 && (std::size_t)d_ids[p] < experts) ++count[d_ids[p] + 1];
  for (std::size_t e = 0; e < experts; ++e) count[e + 1] += count[e];
  const bool off_ok = std::equal(count.begin(), count.end(), d_off.begin()) && (std::size_t)d_off[experts] == P;

  std::cout << "MoE gate: " << experts << " experts, top-" << top_k << ", " << tokens << " tokens, " << how << std::endl;
  std::cout << "ids equal to the host-side stable partial sort: " << (ids_ok ? "yes" : "NO") << std::endl;
  std::cout << "weights within the bound of the fp64 evaluation: " << (w_ok ? "yes" : "NO") << " (worst " << worst << " of the bound)" << std::endl;
  std::cout << "moe_route offsets equal to the host-side count: " << (off_ok ? "yes" : "NO") << std::endl;
  return ids_ok && w_ok && off_ok ? EXIT_SUCCESS : EXIT_FAILURE;
}
