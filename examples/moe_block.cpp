// moe_block groups hidden in tokens top_k -- a whole mixture-of-experts feed-forward block on 2:4 weights, from the router's output to
// the combined hidden states, without a framework op in between: `groups` experts, each a fused gate/up weight W1[2 hidden][in] and a
// down weight W2[in][hidden]; X[tokens][in] in token order; a seeded router gives every token top_k distinct experts (one id in
// groups + 1 stands for an expert of another rank: dropped) and fp32 weights.
//     moe_route              ids -> offsets, sorted_token, pair_pos                              (sm_moe_route, on the device)
//     plan.linear_glu_grouped(.., sorted_token, tokens, ..)   H[P][hidden] = silu(gate) * up, X gathered   (sm_linear24_grouped_glu_gather_*)
//     plan.linear_grouped    Yp[P][in] = H . W2^T                                                (sm_linear24_grouped_*)
//     moe_combine            out[tokens][in] = X + sum_j w_j * Yp[pair_pos]                      (sm_moe_combine_*)
// The result is checked bit for bit against the same block as a caller ran it before: a host-side stable sort, a materialised copy
// X[x_index], the existing linear_glu_grouped / linear_grouped, and a combine on the host (fp32 multiply, fp32 add, one rounding).
// Exits non-zero on a miss.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <numeric>
#include <random>
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
  if (argc != 6) {
    std::cout << "Invalid # of arguments. Usage: ./moe_block groups hidden in tokens top_k" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t groups = std::stoul(argv[1]), hidden = std::stoul(argv[2]), in = std::stoul(argv[3]), tokens = std::stoul(argv[4]),
                    top_k = std::stoul(argv[5]);
  if (groups == 0 || top_k == 0 || top_k > groups || tokens == 0 || hidden % 64 != 0 || in % 64 != 0) {
    std::cout << "1 <= top_k <= groups, tokens >= 1, in % 64 == 0 and hidden % 64 == 0 (hidden is the down projection's in_features)" << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t P = tokens * top_k;

  // the router: top_k distinct choices per token out of groups + 1, the last of which lives on another rank
  std::mt19937 gen(0x5EED);
  std::vector<int> h_ids(P), pick(groups + 1);
  host_vector<float> h_w(P);
  for (std::size_t t = 0; t < tokens; ++t) {
    std::iota(pick.begin(), pick.end(), 0);
    for (std::size_t j = 0; j < top_k; ++j) {
      std::swap(pick[j], pick[j + gen() % (groups + 1 - j)]);
      h_ids[t * top_k + j] = pick[j];
      h_w[t * top_k + j] = 0.125f + 0.75f * util::get_random<float>();
    }
  }
  // the host-side route: a stable sort of the kept pairs by expert
  std::vector<int> order;
  for (std::size_t p = 0; p < P; ++p)
    if (h_ids[p] >= 0 && (std::size_t)h_ids[p] < groups) order.push_back((int)p);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return h_ids[a] < h_ids[b]; });
  const std::size_t V = order.size();
  std::vector<int> r_off(groups + 1, 0), r_token(P, -1), r_pair(P, -1), r_pos(P, -1);
  for (std::size_t s = 0; s < V; ++s) {
    ++r_off[h_ids[order[s]] + 1];
    r_pair[s] = order[s];
    r_token[s] = order[s] / (int)top_k;
    r_pos[order[s]] = (int)s;
  }
  for (std::size_t g = 0; g < groups; ++g) r_off[g + 1] += r_off[g];

  host_vector<type_t> h_W1(groups * 2 * hidden * in), h_W2(groups * in * hidden), h_X(tokens * in), h_Xs(P * in);
  for (auto& w : h_W1) w = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& w : h_W2) w = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& x : h_X) x = static_cast<type_t>(util::get_random<float>() - 0.5f);
  for (auto& x : h_Xs) x = static_cast<type_t>(0.0f);
  for (std::size_t s = 0; s < V; ++s) std::memcpy(&h_Xs[s * in], &h_X[(std::size_t)r_token[s] * in], in * sizeof(type_t));   // X[x_index]

  device_vector<type_t> W1 = h_W1, W2 = h_W2, X = h_X, Xs = h_Xs, H(P * hidden), Yp(P * in), out(tokens * in), Hr(P * hidden), Yr(P * in);
  device_vector<int> ids = h_ids, off(groups + 1), s_token(P), s_pair(P), pos(P), off_r = r_off;
  device_vector<float> w = h_w;
  device_vector<unsigned char> ws(std::max<std::size_t>(moe_route_workspace(tokens, top_k, groups), 16));

  int rc = SM_STATUS_SUCCESS;
  auto keep_first = [&rc](int status) {
    if (rc == SM_STATUS_SUCCESS) rc = status;
  };
  spmma_plan_t<type_t> up(groups * 2 * hidden, in), down(groups * in, hidden);
  keep_first(up.compress(W1.data().get(), true));  // TILE prune in place + blob, once
  keep_first(down.compress(W2.data().get(), true));

  // the block: four launches (the route's multi form: six), nothing allocated, nothing copied to the host
  keep_first(moe_route(ids.data().get(), tokens, top_k, groups, off.data().get(), s_token.data().get(), s_pair.data().get(), pos.data().get(),
                       ws.data().get(), ws.size()));
  keep_first(up.linear_glu_grouped(X.data().get(), H.data().get(), off.data().get(), s_token.data().get(), tokens, groups, P, SM_GLU_ACT_SILU));
  keep_first(down.linear_grouped(H.data().get(), Yp.data().get(), off.data().get(), groups, P));
  keep_first(moe_combine<type_t>(Yp.data().get(), pos.data().get(), w.data().get(), X.data().get(), out.data().get(), tokens, top_k, in, P));
  // the host-routed block: the materialised X[x_index] through the existing grouped calls
  keep_first(up.linear_glu_grouped(Xs.data().get(), Hr.data().get(), off_r.data().get(), groups, P, SM_GLU_ACT_SILU));
  keep_first(down.linear_grouped(Hr.data().get(), Yr.data().get(), off_r.data().get(), groups, P));
  (void)hipDeviceSynchronize();
  if (rc != SM_STATUS_SUCCESS) {
    std::cerr << "moe_block: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }

  const host_vector<int> d_off = off.to_host(), d_token = s_token.to_host(), d_pair = s_pair.to_host(), d_pos = pos.to_host();
  const bool route_ok = std::memcmp(d_off.data(), r_off.data(), (groups + 1) * sizeof(int)) == 0 &&
                        std::memcmp(d_token.data(), r_token.data(), P * sizeof(int)) == 0 &&
                        std::memcmp(d_pair.data(), r_pair.data(), P * sizeof(int)) == 0 && std::memcmp(d_pos.data(), r_pos.data(), P * sizeof(int)) == 0;
  // ... and the combine on the host: s = X[t]; per kept pair q = w * y, s = s + q (two roundings: the volatile keeps them apart); one rounding
  const host_vector<type_t> h_Yr = Yr.to_host(), h_out = out.to_host();
  bool block_ok = true;
  for (std::size_t t = 0; t < tokens; ++t)
    for (std::size_t c = 0; c < in; ++c) {
      float s = static_cast<float>(h_X[t * in + c]);
      for (std::size_t j = 0; j < top_k; ++j) {
        const int sp = r_pos[t * top_k + j];
        if (sp < 0) continue;
        volatile float q = h_w[t * top_k + j] * static_cast<float>(h_Yr[(std::size_t)sp * in + c]);
        s = s + q;
      }
      const type_t want = static_cast<type_t>(s);
      block_ok = block_ok && std::memcmp(&want, &h_out[t * in + c], sizeof(type_t)) == 0;
    }
  std::cout << "MoE block: " << groups << " experts, top-" << top_k << ", " << tokens << " tokens, " << V << " of " << P << " pairs kept" << std::endl;
  std::cout << "moe_route equal to the host-side stable sort: " << (route_ok ? "yes" : "NO") << std::endl;
  std::cout << "route + gathered gate/up + down + combine equal to the host-routed block bit for bit: " << (block_ok ? "yes" : "NO") << std::endl;
  return route_ok && block_ok ? EXIT_SUCCESS : EXIT_FAILURE;
}
