// rope_append seqs q_heads kv_heads head_dim context -- the attention half of a decode step through the headers, without a framework op:
//     rope_append  rotate Q and K by the cos/sin table, write K and V into their pages                               (sm_rope_append_bf16)
//     attn_decode  O[s][h] = softmax(scale q . K^T) V over the pages block_table[s] names                            (sm_attn_decode_bf16)
// bfloat16 operands, NEOX pairs over the whole head, pages of 16 tokens, a permuted page table, sequence s holds max(2, context - 7 s) tokens.
//   1. prefill: the first L_s - 1 tokens of every sequence, in shuffled order, as column slices of one fused QKV buffer, Q rotated in place
//   2. decode:  one token per sequence with positions = nullptr and token_seq = nullptr (seq_lens already counts it)
//   3. attn_decode on the decode step's rotated Q, read in place from the fused buffer
// Checked on the host: Qo of both calls and every row of the cache bit for bit against a loop of the definition (two rounded fp32 products,
// one rounded sum, one rounding to bfloat16), and the attention output bit for bit against attn_decode on a cache filled on the host.
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
// the definition on one head, NEOX pairs over rot = head_dim: never an fma
static void rotate_head(const uint16_t* x, uint16_t* y, const float* row, std::size_t hd) {
#pragma clang fp contract(off)
  const std::size_t half = hd / 2;
  for (std::size_t j = 0; j < half; ++j) {
    const float xa = bf16_to_float(x[j]), xb = bf16_to_float(x[j + half]), c = row[j], s = row[half + j];
    const volatile float ac = xa * c, bs = xb * s, bc = xb * c, as = xa * s;
    const float ya = ac - bs, yb = bc + as;
    y[j] = float_to_bf16(ya);
    y[j + half] = float_to_bf16(yb);
  }
}

int main(int argc, char** argv) {
  using namespace sparsifyme;
  if (argc != 6) {
    std::cout << "Invalid # of arguments. Usage: ./rope_append seqs q_heads kv_heads head_dim context" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t seqs = std::stoul(argv[1]), qh = std::stoul(argv[2]), kvh = std::stoul(argv[3]), hd = std::stoul(argv[4]), context = std::stoul(argv[5]);
  const std::size_t ps = 16, max_pages = (context + ps - 1) / ps + 1, num_pages = seqs * max_pages + 2, max_pos = max_pages * ps;
  int aform = SM_ATTN_DECODE_FORM_INVALID, rform = SM_ROPE_APPEND_FORM_INVALID;
  if (seqs == 0 || qh == 0 || context < 2 || sm_attn_decode_form(seqs, qh, kvh, hd, ps, max_pages, &aform) != SM_STATUS_SUCCESS ||
      aform == SM_ATTN_DECODE_FORM_INVALID || hd % 16 != 0) {
    std::cout << "seqs, q_heads >= 1, context >= 2; head_dim 64 or 128; q_heads a multiple of kv_heads with a group of at most " << SM_ATTN_DECODE_MAX_GROUP
              << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t W = (qh + 2 * kvh) * hd, kw = kvh * hd;   // the fused QKV row; Q at column 0, K at qh * hd, V behind it

  // a permuted page table and the lengths AFTER the decode step
  std::vector<int> perm(num_pages), table(seqs * max_pages), lens(seqs);
  for (std::size_t i = 0; i < num_pages; ++i) perm[i] = (int)i;
  for (std::size_t i = num_pages - 1; i > 0; --i) std::swap(perm[i], perm[std::min(i, (std::size_t)(util::get_random<float>() * (i + 1)))]);
  for (std::size_t i = 0; i < seqs * max_pages; ++i) table[i] = perm[i];
  for (std::size_t s = 0; s < seqs; ++s) lens[s] = (int)std::max<std::size_t>(2, context > 7 * s ? context - 7 * s : 2);
  auto at = [&](std::size_t s, std::size_t t) { return ((std::size_t)table[s * max_pages + t / ps] * ps + t % ps) * kw; };

  // the prefill's tokens, shuffled
  std::vector<int> tseq, tpos;
  for (std::size_t s = 0; s < seqs; ++s)
    for (int t = 0; t + 1 < lens[s]; ++t) {
      tseq.push_back((int)s);
      tpos.push_back(t);
    }
  const std::size_t T = tseq.size();
  for (std::size_t i = T - 1; i > 0; --i) {
    const std::size_t j = std::min(i, (std::size_t)(util::get_random<float>() * (i + 1)));
    std::swap(tseq[i], tseq[j]);
    std::swap(tpos[i], tpos[j]);
  }
  (void)sm_rope_append_form(T, qh, kvh, hd, hd, &rform);

  std::vector<float> h_cs(max_pos * hd);
  rope_table(h_cs.data(), max_pos, hd);
  std::vector<uint16_t> h_pre(T * W), h_dec(seqs * W), d_pre(T * W), d_dec(seqs * W);
  for (auto& x : h_pre) x = float_to_bf16(2.0f * util::get_random<float>() - 1.0f);
  for (auto& x : h_dec) x = float_to_bf16(2.0f * util::get_random<float>() - 1.0f);

  const std::size_t nkv = num_pages * ps * kw, nq = seqs * qh * hd, ws_bytes = attn_decode_workspace_size(seqs, qh, hd, ps, max_pages);
  __bf16 *pre = nullptr, *dec = nullptr, *Kc = nullptr, *Vc = nullptr, *Kh = nullptr, *Vh = nullptr, *Qh = nullptr, *O = nullptr, *Oh = nullptr;
  float* cs = nullptr;
  int *bt = nullptr, *sl = nullptr, *dseq = nullptr, *dpos = nullptr;
  void* ws = nullptr;
  const bool alloc = hipMalloc((void**)&pre, T * W * 2) == hipSuccess && hipMalloc((void**)&dec, seqs * W * 2) == hipSuccess && hipMalloc((void**)&Kc, nkv * 2) == hipSuccess &&
                     hipMalloc((void**)&Vc, nkv * 2) == hipSuccess && hipMalloc((void**)&Kh, nkv * 2) == hipSuccess && hipMalloc((void**)&Vh, nkv * 2) == hipSuccess &&
                     hipMalloc((void**)&Qh, nq * 2) == hipSuccess && hipMalloc((void**)&O, nq * 2) == hipSuccess && hipMalloc((void**)&Oh, nq * 2) == hipSuccess &&
                     hipMalloc((void**)&cs, h_cs.size() * 4) == hipSuccess && hipMalloc((void**)&bt, table.size() * 4) == hipSuccess &&
                     hipMalloc((void**)&sl, seqs * 4) == hipSuccess && hipMalloc((void**)&dseq, T * 4) == hipSuccess && hipMalloc((void**)&dpos, T * 4) == hipSuccess &&
                     (ws_bytes == 0 || hipMalloc(&ws, ws_bytes) == hipSuccess);
  if (!alloc) {
    std::cerr << "rope_append: out of device memory" << std::endl;
    return EXIT_FAILURE;
  }
  (void)hipMemcpy(pre, h_pre.data(), T * W * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(dec, h_dec.data(), seqs * W * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(cs, h_cs.data(), h_cs.size() * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(bt, table.data(), table.size() * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(sl, lens.data(), seqs * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(dseq, tseq.data(), T * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(dpos, tpos.data(), T * 4, hipMemcpyHostToDevice);
  (void)hipMemset(Kc, 0, nkv * 2);
  (void)hipMemset(Vc, 0, nkv * 2);

  auto must = [&](int rc, const char* what) {
    if (rc == SM_STATUS_SUCCESS && hipDeviceSynchronize() != hipSuccess) rc = SM_STATUS_LAUNCH_FAILED;
    if (rc != SM_STATUS_SUCCESS) {
      std::cerr << what << ": " << sm_last_error() << std::endl;
      std::exit(EXIT_FAILURE);
    }
  };
  // 1. the prefill: Q rotated in place, Ko not written, K and V into their pages
  must(rope_append<__bf16>(pre, pre + qh * hd, pre + qh * hd + kw, pre, nullptr, Kc, Vc, cs, dpos, dseq, nullptr, bt, T, seqs, qh, kvh, hd, hd, max_pos, num_pages, ps,
                           max_pages, SM_ROPE_NEOX, nullptr, W, W, W, W),
       "rope_append (prefill)");
  // 2. the decode step: token i is sequence i at seq_lens[i] - 1
  must(rope_append<__bf16>(dec, dec + qh * hd, dec + qh * hd + kw, dec, nullptr, Kc, Vc, cs, nullptr, nullptr, sl, bt, seqs, seqs, qh, kvh, hd, hd, max_pos, num_pages,
                           ps, max_pages, SM_ROPE_NEOX, nullptr, W, W, W, W),
       "rope_append (decode)");
  // 3. attention, Q read in place from the fused buffer
  must(attn_decode<__bf16>(dec, Kc, Vc, bt, sl, O, seqs, qh, kvh, hd, num_pages, ps, max_pages, ws, ws_bytes, nullptr, 0.0f, nullptr, W), "attn_decode");
  (void)hipMemcpy(d_pre.data(), pre, T * W * 2, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_dec.data(), dec, seqs * W * 2, hipMemcpyDeviceToHost);
  std::vector<uint16_t> d_K(nkv), d_V(nkv), d_O(nq), d_Oh(nq);
  (void)hipMemcpy(d_K.data(), Kc, nkv * 2, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_V.data(), Vc, nkv * 2, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_O.data(), O, nq * 2, hipMemcpyDeviceToHost);

  // 4. the definition on the host: the fused buffers as the calls leave them (Q rotated, K and V untouched) and the cache
  std::vector<uint16_t> w_pre(h_pre), w_dec(h_dec), w_K(nkv, 0), w_V(nkv, 0), w_Q(nq), rk(hd);
  auto token = [&](const uint16_t* in, uint16_t* out, std::size_t s, std::size_t pos) {
    const float* row = h_cs.data() + pos * hd;
    for (std::size_t h = 0; h < qh; ++h) rotate_head(in + h * hd, out + h * hd, row, hd);
    for (std::size_t g = 0; g < kvh; ++g) {
      rotate_head(in + (qh + g) * hd, rk.data(), row, hd);
      std::copy(rk.begin(), rk.end(), w_K.begin() + at(s, pos) + g * hd);
      std::copy(in + (qh + kvh + g) * hd, in + (qh + kvh + g + 1) * hd, w_V.begin() + at(s, pos) + g * hd);
    }
  };
  for (std::size_t i = 0; i < T; ++i) token(h_pre.data() + i * W, w_pre.data() + i * W, (std::size_t)tseq[i], (std::size_t)tpos[i]);
  for (std::size_t s = 0; s < seqs; ++s) {
    token(h_dec.data() + s * W, w_dec.data() + s * W, s, (std::size_t)lens[s] - 1);
    std::copy(w_dec.begin() + s * W, w_dec.begin() + s * W + qh * hd, w_Q.begin() + s * qh * hd);
  }
  std::size_t bad_q = 0, bad_kv = 0, bad_o = 0;
  for (std::size_t i = 0; i < T * W; ++i) bad_q += d_pre[i] != w_pre[i];
  for (std::size_t i = 0; i < seqs * W; ++i) bad_q += d_dec[i] != w_dec[i];
  for (std::size_t i = 0; i < nkv; ++i) bad_kv += (d_K[i] != w_K[i]) + (d_V[i] != w_V[i]);

  // 5. attn_decode on the host-filled cache and the host-rotated Q
  (void)hipMemcpy(Kh, w_K.data(), nkv * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(Vh, w_V.data(), nkv * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(Qh, w_Q.data(), nq * 2, hipMemcpyHostToDevice);
  must(attn_decode<__bf16>(Qh, Kh, Vh, bt, sl, Oh, seqs, qh, kvh, hd, num_pages, ps, max_pages, ws, ws_bytes), "attn_decode (host-filled cache)");
  (void)hipMemcpy(d_Oh.data(), Oh, nq * 2, hipMemcpyDeviceToHost);
  std::size_t nonzero = 0;
  for (std::size_t i = 0; i < nq; ++i) {
    bad_o += d_O[i] != d_Oh[i];
    nonzero += (d_O[i] & 0x7fffu) != 0;
  }
  bad_o += nonzero == 0;

  std::cout << "rope + cache append + paged decode attention: " << seqs << " sequences, " << qh << " query heads on " << kvh << " KV heads, head_dim " << hd
            << ", context " << context << " in pages of " << ps << "; prefill of " << T << " tokens in the "
            << (rform == SM_ROPE_APPEND_FORM_BLOCK ? "block" : "wave") << " form, attention in the " << (aform == SM_ATTN_DECODE_FORM_DIRECT ? "direct" : "split")
            << " form" << std::endl;
  std::cout << "rotated Q of the prefill and the decode step equal to the host loop of the definition, K and V slices untouched: " << (bad_q ? "NO" : "yes") << std::endl;
  std::cout << "every row of the K and V cache equal to the host loop: " << (bad_kv ? "NO" : "yes") << std::endl;
  std::cout << "attention output equal to attn_decode on the host-filled cache: " << (bad_o ? "NO" : "yes") << std::endl;
  for (void* p : {(void*)pre, (void*)dec, (void*)Kc, (void*)Vc, (void*)Kh, (void*)Vh, (void*)Qh, (void*)O, (void*)Oh, (void*)cs, (void*)bt, (void*)sl, (void*)dseq,
                  (void*)dpos, ws})
    (void)hipFree(p);
  return !bad_q && !bad_kv && !bad_o ? EXIT_SUCCESS : EXIT_FAILURE;
}
