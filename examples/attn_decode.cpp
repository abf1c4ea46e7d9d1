// attn_decode seqs q_heads kv_heads head_dim context -- single-query attention over a paged KV cache through the headers, without a framework op:
//     attn_decode  O[s][h] = softmax(scale q . K^T) V over the pages block_table[s] names, lengths from seq_lens      (sm_attn_decode_bf16)
// bfloat16 operands, pages of 16 tokens, a permuted page table, sequence s holds max(1, context - 7 s) tokens.  Checked on the host:
//   one-hot   scale 1, q = 8 entries of 4, K zero except K[target] = q: the target scores 128, every other token 0, p is exactly one-hot, so
//             O is V's target row bit for bit (V's bits encode page, slot, head and dim) and lse = 128
//   uniform   Q = 0: every p = 1; V integers |v| <= 7, every partial sum an exact integer: O = round(sum v / L) bit for bit
//   general   Q, K uniform in [-1, 1), V in [-2, 2): O against a host fp64 softmax within half an ulp of bfloat16 plus
//             (2 u + 2 delta + (L + head_dim + 16) 2^-24) sum p |v| / sum p  (u = 2^-8, delta = (head_dim + 2) 2^-24 scale max_t sum |q k|)
// Exits non-zero on a miss.
#include <hip/hip_runtime.h>

#include <algorithm>
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
  if (argc != 6) {
    std::cout << "Invalid # of arguments. Usage: ./attn_decode seqs q_heads kv_heads head_dim context" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t seqs = std::stoul(argv[1]), qh = std::stoul(argv[2]), kvh = std::stoul(argv[3]), hd = std::stoul(argv[4]), context = std::stoul(argv[5]);
  const std::size_t ps = 16;
  int form = SM_ATTN_DECODE_FORM_INVALID;
  const std::size_t max_pages = (context + ps - 1) / ps + 1, num_pages = seqs * max_pages + 2;
  if (seqs == 0 || qh == 0 || context == 0 || sm_attn_decode_form(seqs, qh, kvh, hd, ps, max_pages, &form) != SM_STATUS_SUCCESS ||
      form == SM_ATTN_DECODE_FORM_INVALID || (qh / kvh) * 8 > hd || 7 * context >= (1u << 24)) {
    std::cout << "seqs, q_heads, context >= 1; head_dim 64 or 128; q_heads a multiple of kv_heads with a group of at most head_dim / 8 (the one-hot class) "
                 "and " << SM_ATTN_DECODE_MAX_GROUP << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t group = qh / kvh;
  const float scale = 1.0f / std::sqrt((float)hd);

  // a permuted page table: sequence s owns max_pages pages scattered over the cache
  std::vector<int> perm(num_pages), table(seqs * max_pages), lens(seqs);
  for (std::size_t i = 0; i < num_pages; ++i) perm[i] = (int)i;
  for (std::size_t i = num_pages - 1; i > 0; --i) std::swap(perm[i], perm[std::min(i, (std::size_t)(util::get_random<float>() * (i + 1)))]);
  for (std::size_t i = 0; i < seqs * max_pages; ++i) table[i] = perm[i];
  for (std::size_t s = 0; s < seqs; ++s) lens[s] = (int)std::max<std::size_t>(1, context > 7 * s ? context - 7 * s : 1);
  auto at = [&](std::size_t s, std::size_t t) { return (((std::size_t)table[s * max_pages + t / ps] * ps + t % ps) * kvh) * hd; };  // + kv * hd + d

  const std::size_t nq = seqs * qh * hd, nkv = num_pages * ps * kvh * hd, ws_bytes = attn_decode_workspace_size(seqs, qh, hd, ps, max_pages);
  __bf16 *Q = nullptr, *K = nullptr, *V = nullptr, *O = nullptr;
  int *bt = nullptr, *sl = nullptr;
  float* lse = nullptr;
  void* ws = nullptr;
  const bool alloc = hipMalloc((void**)&Q, nq * 2) == hipSuccess && hipMalloc((void**)&K, nkv * 2) == hipSuccess && hipMalloc((void**)&V, nkv * 2) == hipSuccess &&
                     hipMalloc((void**)&O, nq * 2) == hipSuccess && hipMalloc((void**)&bt, table.size() * 4) == hipSuccess &&
                     hipMalloc((void**)&sl, seqs * 4) == hipSuccess && hipMalloc((void**)&lse, seqs * qh * 4) == hipSuccess &&
                     (ws_bytes == 0 || hipMalloc(&ws, ws_bytes) == hipSuccess);
  if (!alloc) {
    std::cerr << "attn_decode: out of device memory" << std::endl;
    return EXIT_FAILURE;
  }
  (void)hipMemcpy(bt, table.data(), table.size() * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(sl, lens.data(), seqs * 4, hipMemcpyHostToDevice);

  std::vector<uint16_t> h_Q(nq), h_K(nkv), h_V(nkv), d_O(nq);
  std::vector<float> d_lse(seqs * qh);
  auto run = [&](float sc) {
    (void)hipMemcpy(Q, h_Q.data(), nq * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(K, h_K.data(), nkv * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(V, h_V.data(), nkv * 2, hipMemcpyHostToDevice);
    int rc = attn_decode<__bf16>(Q, K, V, bt, sl, O, seqs, qh, kvh, hd, num_pages, ps, max_pages, ws, ws_bytes, lse, sc);
    if (rc == SM_STATUS_SUCCESS && hipDeviceSynchronize() != hipSuccess) rc = SM_STATUS_LAUNCH_FAILED;
    if (rc != SM_STATUS_SUCCESS) {
      std::cerr << "attn_decode: " << sm_last_error() << std::endl;
      std::exit(EXIT_FAILURE);
    }
    (void)hipMemcpy(d_O.data(), O, nq * 2, hipMemcpyDeviceToHost);
    (void)hipMemcpy(d_lse.data(), lse, seqs * qh * 4, hipMemcpyDeviceToHost);
  };

  // one-hot: the target of (s, h) is one of the first, the last, a page's last slot, the next page's first
  std::size_t bad_hot = 0;
  std::fill(h_Q.begin(), h_Q.end(), 0);
  std::fill(h_K.begin(), h_K.end(), 0);
  for (std::size_t i = 0; i < nkv; ++i) h_V[i] = (uint16_t)(0x0400u + (i * 2654435761u >> 7) % 0x3000u + ((i & 1u) << 15));
  std::vector<std::size_t> target(seqs * qh);
  for (std::size_t s = 0; s < seqs; ++s)
    for (std::size_t h = 0; h < qh; ++h) {
      const std::size_t L = (std::size_t)lens[s], pick[4] = {0, L - 1, std::min(ps - 1, L - 1), std::min(ps, L - 1)};
      const std::size_t t = target[s * qh + h] = pick[(s + h) % 4], g = h % group;
      for (std::size_t j = 0; j < 8; ++j) {
        h_Q[(s * qh + h) * hd + 8 * g + j] = float_to_bf16(4.0f);
        h_K[at(s, t) + (h / group) * hd + 8 * g + j] = float_to_bf16(4.0f);
      }
    }
  run(1.0f);
  for (std::size_t s = 0; s < seqs; ++s)
    for (std::size_t h = 0; h < qh; ++h) {
      for (std::size_t d = 0; d < hd; ++d) bad_hot += d_O[(s * qh + h) * hd + d] != h_V[at(s, target[s * qh + h]) + (h / group) * hd + d];
      bad_hot += d_lse[s * qh + h] != 128.0f;
    }

  // uniform
  std::size_t bad_uni = 0;
  std::fill(h_Q.begin(), h_Q.end(), 0);
  for (auto& x : h_K) x = float_to_bf16(2.0f * util::get_random<float>() - 1.0f);
  for (auto& x : h_V) x = float_to_bf16(std::floor(util::get_random<float>() * 15.0f) - 7.0f);
  run(scale);
  for (std::size_t s = 0; s < seqs; ++s)
    for (std::size_t h = 0; h < qh; ++h)
      for (std::size_t d = 0; d < hd; ++d) {
        float sum = 0.0f;  // exact: integers, 7 L < 2^24
        for (std::size_t t = 0; t < (std::size_t)lens[s]; ++t) sum += bf16_to_float(h_V[at(s, t) + (h / group) * hd + d]);
        bad_uni += d_O[(s * qh + h) * hd + d] != float_to_bf16(sum / (float)lens[s]);
      }

  // general data against fp64
  std::size_t bad_gen = 0;
  double worst = 0.0;
  for (auto& x : h_Q) x = float_to_bf16(2.0f * util::get_random<float>() - 1.0f);
  for (auto& x : h_V) x = float_to_bf16(4.0f * util::get_random<float>() - 2.0f);
  run(scale);
  for (std::size_t s = 0; s < seqs; ++s)
    for (std::size_t h = 0; h < qh; ++h) {
      const std::size_t L = (std::size_t)lens[s], kv = h / group;
      std::vector<double> sc(L);
      double m = -INFINITY, sabs = 0.0, l = 0.0;
      for (std::size_t t = 0; t < L; ++t) {
        double dot = 0.0, ab = 0.0;
        for (std::size_t d = 0; d < hd; ++d) {
          const double p = (double)bf16_to_float(h_Q[(s * qh + h) * hd + d]) * (double)bf16_to_float(h_K[at(s, t) + kv * hd + d]);
          dot += p;
          ab += std::fabs(p);
        }
        sc[t] = (double)scale * dot;
        m = std::max(m, sc[t]);
        sabs = std::max(sabs, (double)scale * ab);
      }
      for (std::size_t t = 0; t < L; ++t) l += (sc[t] = std::exp(sc[t] - m));
      const double delta = (double)(hd + 2) * std::ldexp(1.0, -24) * sabs;
      for (std::size_t d = 0; d < hd; ++d) {
        double acc = 0.0, aabs = 0.0;
        for (std::size_t t = 0; t < L; ++t) {
          const double v = (double)bf16_to_float(h_V[at(s, t) + kv * hd + d]);
          acc += sc[t] * v;
          aabs += sc[t] * std::fabs(v);
        }
        const double ref = acc / l, got = (double)bf16_to_float(d_O[(s * qh + h) * hd + d]), big = std::max(std::fabs(ref), std::fabs(got));
        const double ulp = std::ldexp(1.0, std::max(big > 0.0 ? (int)std::floor(std::log2(big)) : -126, -126) - 7);
        const double bound = 0.5 * ulp + (2.0 * std::ldexp(1.0, -8) + 2.0 * delta + (double)(L + hd + 16) * std::ldexp(1.0, -24)) * aabs / l;
        const double ratio = std::fabs(got - ref) / bound;
        worst = std::max(worst, ratio);
        bad_gen += !(ratio <= 1.0);
      }
    }

  std::cout << "paged decode attention: " << seqs << " sequences, " << qh << " query heads on " << kvh << " KV heads, head_dim " << hd << ", context "
            << context << " in pages of " << ps << ", form " << (form == SM_ATTN_DECODE_FORM_DIRECT ? "direct" : "split") << std::endl;
  std::cout << "one-hot scores: O equal to V's target row, lse = 128: " << (bad_hot ? "NO" : "yes") << std::endl;
  std::cout << "uniform scores: O equal to the rounded mean of V: " << (bad_uni ? "NO" : "yes") << std::endl;
  std::cout << "general data within the bound of the fp64 softmax (worst " << worst << " of it): " << (bad_gen ? "NO" : "yes") << std::endl;
  for (void* p : {(void*)Q, (void*)K, (void*)V, (void*)O, (void*)bt, (void*)sl, (void*)lse, ws}) (void)hipFree(p);
  return !bad_hot && !bad_uni && !bad_gen ? EXIT_SUCCESS : EXIT_FAILURE;
}
