// kv8_decode seqs q_heads kv_heads head_dim context [e4m3|e5m2] -- the attention half of a decode step over the fp8 paged KV cache, through
// the headers:
//     rope_append_kv8  rotate Q and K, quantise every K and V head by the per-row fp8 rule, write bytes and scales    (sm_rope_append_kv8_bf16)
//     attn_decode_kv8  O[s][h] = softmax(scale q . (ks k8)^T) (vs v8) over the pages block_table[s] names            (sm_attn_decode_kv8_bf16)
// bfloat16 Q / K / V, NEOX pairs over the whole head, pages of 16 tokens, a permuted page table, sequence s holds max(2, context - 7 s) tokens.
//   1. prefill: the first L_s - 1 tokens of every sequence, in shuffled order, as column slices of one fused QKV buffer, Q rotated in place
//   2. decode:  one token per sequence with positions = nullptr and token_seq = nullptr (seq_lens already counts it)
//   3. attn_decode_kv8 on the decode step's rotated Q, read in place from the fused buffer
// Checked on the host: every byte and every scale of the cache bit for bit against a loop of the definition (the rotation, then amax,
// two fp32 divisions, one multiply, round to nearest even to the format), and O against an fp64 softmax over the DEQUANTISED cache within
// half an ulp of bfloat16 plus (2 u + 2 delta + (L + head_dim + 17) 2^-24) sum p |vs v8| / sum p, u = 2^-8, delta = (head_dim + 3) 2^-24
// scale max_t |ks_t| sum |q k8|.  Exits non-zero on a miss.
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

// OCP fp8: e4m3 (3 mantissa bits, bias 7) or e5m2 (2 mantissa bits, bias 15)
struct Fp8 {
  int mant, bias;
  float fmax;
};
static double fp8_to_double(uint8_t b, const Fp8& f) {
  const int e = (b & 0x7f) >> f.mant, m = b & ((1 << f.mant) - 1);
  const double v = e ? std::ldexp(1.0 + m / (double)(1 << f.mant), e - f.bias) : std::ldexp(m / (double)(1 << f.mant), 1 - f.bias);
  return b & 0x80 ? -v : v;
}
// a finite y with |y| <= FMAX (1 + 2^-23), rounded to nearest even, subnormals of the format included
static uint8_t float_to_fp8(float y, const Fp8& f) {
  const uint8_t sign = std::signbit(y) ? 0x80 : 0x00;
  const double a = std::fabs((double)y);
  if (a == 0.0) return sign;
  int e;
  (void)std::frexp(a, &e);                                    // a = 1.x * 2^(e - 1)
  int E = std::max(e - 1, 1 - f.bias);
  int q = (int)std::nearbyint(std::ldexp(a, f.mant - E));     // exact scaling, one rounding (the default mode: to nearest even)
  if (q == (2 << f.mant)) {
    q >>= 1;
    ++E;
  }
  if (q < (1 << f.mant)) return sign | (uint8_t)q;            // a subnormal of the format, or zero
  return sign | (uint8_t)(((E + f.bias) << f.mant) | (q - (1 << f.mant)));
}
// the per-row rule on one head of bfloat16 bits: bytes and the scale
static float quantise_head(const uint16_t* y, uint8_t* q, std::size_t hd, const Fp8& f) {
#pragma clang fp contract(off)
  float amax = 0.0f;
  for (std::size_t d = 0; d < hd; ++d) amax = std::max(amax, std::fabs(bf16_to_float(y[d])));
  amax = std::max(amax, std::ldexp(1.0f, -100));
  const volatile float scale = amax / f.fmax, inv = f.fmax / amax;
  for (std::size_t d = 0; d < hd; ++d) {
    const volatile float v = bf16_to_float(y[d]) * inv;
    q[d] = float_to_fp8(v, f);
  }
  return scale;
}

int main(int argc, char** argv) {
  using namespace sparsifyme;
  if (argc != 6 && argc != 7) {
    std::cout << "Invalid # of arguments. Usage: ./kv8_decode seqs q_heads kv_heads head_dim context [e4m3|e5m2]" << std::endl;
    return EXIT_FAILURE;
  }
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "\nlibsparsifyme is supported only on gfx950 (MI355X) devices: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t seqs = std::stoul(argv[1]), qh = std::stoul(argv[2]), kvh = std::stoul(argv[3]), hd = std::stoul(argv[4]), context = std::stoul(argv[5]);
  const std::string fname = argc == 7 ? argv[6] : "e4m3";
  if (fname != "e4m3" && fname != "e5m2") {
    std::cout << "the format is e4m3 or e5m2" << std::endl;
    return EXIT_FAILURE;
  }
  const int fmt = fname == "e4m3" ? SM_FP8_E4M3 : SM_FP8_E5M2;
  const Fp8 f8 = fname == "e4m3" ? Fp8{3, 7, 448.0f} : Fp8{2, 15, 57344.0f};
  const std::size_t ps = 16, max_pages = (context + ps - 1) / ps + 1, num_pages = seqs * max_pages + 2, max_pos = max_pages * ps;
  int aform = SM_ATTN_DECODE_FORM_INVALID, rform = SM_ROPE_APPEND_FORM_INVALID;
  if (seqs == 0 || qh == 0 || context < 2 || sm_attn_decode_form(seqs, qh, kvh, hd, ps, max_pages, &aform) != SM_STATUS_SUCCESS ||
      aform == SM_ATTN_DECODE_FORM_INVALID) {
    std::cout << "seqs, q_heads >= 1, context >= 2; head_dim 64 or 128; q_heads a multiple of kv_heads with a group of at most " << SM_ATTN_DECODE_MAX_GROUP
              << std::endl;
    return EXIT_FAILURE;
  }
  const std::size_t W = (qh + 2 * kvh) * hd, kw = kvh * hd, group = qh / kvh;   // the fused QKV row; Q at column 0, K at qh * hd, V behind it
  const float scale = 1.0f / std::sqrt((float)hd);

  // a permuted page table and the lengths AFTER the decode step
  std::vector<int> perm(num_pages), table(seqs * max_pages), lens(seqs);
  for (std::size_t i = 0; i < num_pages; ++i) perm[i] = (int)i;
  for (std::size_t i = num_pages - 1; i > 0; --i) std::swap(perm[i], perm[std::min(i, (std::size_t)(util::get_random<float>() * (i + 1)))]);
  for (std::size_t i = 0; i < seqs * max_pages; ++i) table[i] = perm[i];
  for (std::size_t s = 0; s < seqs; ++s) lens[s] = (int)std::max<std::size_t>(2, context > 7 * s ? context - 7 * s : 2);
  auto at = [&](std::size_t s, std::size_t t) { return ((std::size_t)table[s * max_pages + t / ps] * ps + t % ps) * kw; };          // a token's row of bytes
  auto sat = [&](std::size_t s, std::size_t t, std::size_t g) { return ((std::size_t)table[s * max_pages + t / ps] * kvh + g) * ps + t % ps; };   // a head's scale

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
  std::vector<uint16_t> h_pre(T * W), h_dec(seqs * W), d_dec(seqs * W);
  for (auto& x : h_pre) x = float_to_bf16(2.0f * util::get_random<float>() - 1.0f);
  for (auto& x : h_dec) x = float_to_bf16(2.0f * util::get_random<float>() - 1.0f);

  const std::size_t nkv = num_pages * ps * kw, nsc = num_pages * kvh * ps, nq = seqs * qh * hd, ws_bytes = attn_decode_workspace_size(seqs, qh, hd, ps, max_pages);
  __bf16 *pre = nullptr, *dec = nullptr, *O = nullptr;
  uint8_t *Kc = nullptr, *Vc = nullptr;
  float *Ksc = nullptr, *Vsc = nullptr, *cs = nullptr;
  int *bt = nullptr, *sl = nullptr, *dseq = nullptr, *dpos = nullptr;
  void* ws = nullptr;
  const bool alloc = hipMalloc((void**)&pre, T * W * 2) == hipSuccess && hipMalloc((void**)&dec, seqs * W * 2) == hipSuccess && hipMalloc((void**)&Kc, nkv) == hipSuccess &&
                     hipMalloc((void**)&Vc, nkv) == hipSuccess && hipMalloc((void**)&Ksc, nsc * 4) == hipSuccess && hipMalloc((void**)&Vsc, nsc * 4) == hipSuccess &&
                     hipMalloc((void**)&O, nq * 2) == hipSuccess && hipMalloc((void**)&cs, h_cs.size() * 4) == hipSuccess &&
                     hipMalloc((void**)&bt, table.size() * 4) == hipSuccess && hipMalloc((void**)&sl, seqs * 4) == hipSuccess &&
                     hipMalloc((void**)&dseq, T * 4) == hipSuccess && hipMalloc((void**)&dpos, T * 4) == hipSuccess && (ws_bytes == 0 || hipMalloc(&ws, ws_bytes) == hipSuccess);
  if (!alloc) {
    std::cerr << "kv8_decode: out of device memory" << std::endl;
    return EXIT_FAILURE;
  }
  (void)hipMemcpy(pre, h_pre.data(), T * W * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(dec, h_dec.data(), seqs * W * 2, hipMemcpyHostToDevice);
  (void)hipMemcpy(cs, h_cs.data(), h_cs.size() * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(bt, table.data(), table.size() * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(sl, lens.data(), seqs * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(dseq, tseq.data(), T * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(dpos, tpos.data(), T * 4, hipMemcpyHostToDevice);
  (void)hipMemset(Kc, 0, nkv);
  (void)hipMemset(Vc, 0, nkv);
  (void)hipMemset(Ksc, 0, nsc * 4);
  (void)hipMemset(Vsc, 0, nsc * 4);

  auto must = [&](int rc, const char* what) {
    if (rc == SM_STATUS_SUCCESS && hipDeviceSynchronize() != hipSuccess) rc = SM_STATUS_LAUNCH_FAILED;
    if (rc != SM_STATUS_SUCCESS) {
      std::cerr << what << ": " << sm_last_error() << std::endl;
      std::exit(EXIT_FAILURE);
    }
  };
  // 1. the prefill: Q rotated in place, Ko not written, K and V quantised into their pages
  must(rope_append_kv8<__bf16>(pre, pre + qh * hd, pre + qh * hd + kw, pre, nullptr, Kc, Vc, Ksc, Vsc, cs, dpos, dseq, nullptr, bt, T, seqs, qh, kvh, hd, hd, max_pos,
                               num_pages, ps, max_pages, fmt, SM_ROPE_NEOX, nullptr, W, W, W, W),
       "rope_append_kv8 (prefill)");
  // 2. the decode step: token i is sequence i at seq_lens[i] - 1
  must(rope_append_kv8<__bf16>(dec, dec + qh * hd, dec + qh * hd + kw, dec, nullptr, Kc, Vc, Ksc, Vsc, cs, nullptr, nullptr, sl, bt, seqs, seqs, qh, kvh, hd, hd, max_pos,
                               num_pages, ps, max_pages, fmt, SM_ROPE_NEOX, nullptr, W, W, W, W),
       "rope_append_kv8 (decode)");
  // 3. attention, Q read in place from the fused buffer
  must(attn_decode_kv8<__bf16>(dec, Kc, Vc, Ksc, Vsc, bt, sl, O, seqs, qh, kvh, hd, num_pages, ps, max_pages, fmt, ws, ws_bytes, nullptr, 0.0f, nullptr, W),
       "attn_decode_kv8");
  std::vector<uint8_t> d_K(nkv), d_V(nkv);
  std::vector<float> d_Ks(nsc), d_Vs(nsc);
  std::vector<uint16_t> d_O(nq);
  (void)hipMemcpy(d_dec.data(), dec, seqs * W * 2, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_K.data(), Kc, nkv, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_V.data(), Vc, nkv, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_Ks.data(), Ksc, nsc * 4, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_Vs.data(), Vsc, nsc * 4, hipMemcpyDeviceToHost);
  (void)hipMemcpy(d_O.data(), O, nq * 2, hipMemcpyDeviceToHost);

  // 4. the definition on the host: the cache as the two appends leave it, and the decode step's rotated Q
  std::vector<uint8_t> w_K(nkv, 0), w_V(nkv, 0);
  std::vector<float> w_Ks(nsc, 0.0f), w_Vs(nsc, 0.0f);
  std::vector<uint16_t> w_Q(nq), rk(hd);
  auto token = [&](const uint16_t* in, std::size_t s, std::size_t pos) {
    const float* row = h_cs.data() + pos * hd;
    for (std::size_t g = 0; g < kvh; ++g) {
      rotate_head(in + (qh + g) * hd, rk.data(), row, hd);
      w_Ks[sat(s, pos, g)] = quantise_head(rk.data(), w_K.data() + at(s, pos) + g * hd, hd, f8);
      w_Vs[sat(s, pos, g)] = quantise_head(in + (qh + kvh + g) * hd, w_V.data() + at(s, pos) + g * hd, hd, f8);
    }
  };
  for (std::size_t i = 0; i < T; ++i) token(h_pre.data() + i * W, (std::size_t)tseq[i], (std::size_t)tpos[i]);
  for (std::size_t s = 0; s < seqs; ++s) {
    token(h_dec.data() + s * W, s, (std::size_t)lens[s] - 1);
    for (std::size_t h = 0; h < qh; ++h) rotate_head(h_dec.data() + s * W + h * hd, w_Q.data() + (s * qh + h) * hd, h_cs.data() + ((std::size_t)lens[s] - 1) * hd, hd);
  }
  std::size_t bad_q = 0, bad_bytes = 0, bad_scales = 0, bad_o = 0;
  for (std::size_t s = 0; s < seqs; ++s)
    for (std::size_t i = 0; i < qh * hd; ++i) bad_q += d_dec[s * W + i] != w_Q[s * qh * hd + i];
  for (std::size_t i = 0; i < nkv; ++i) bad_bytes += (d_K[i] != w_K[i]) + (d_V[i] != w_V[i]);
  for (std::size_t i = 0; i < nsc; ++i) bad_scales += (std::memcmp(&d_Ks[i], &w_Ks[i], 4) != 0) + (std::memcmp(&d_Vs[i], &w_Vs[i], 4) != 0);

  // 5. O against fp64 over the dequantised cache (the device's own bytes and scales, just checked)
  double worst = 0.0;
  for (std::size_t s = 0; s < seqs; ++s)
    for (std::size_t h = 0; h < qh; ++h) {
      const std::size_t L = (std::size_t)lens[s], kv = h / group;
      std::vector<double> sc(L);
      double m = -INFINITY, sabs = 0.0, l = 0.0;
      for (std::size_t t = 0; t < L; ++t) {
        double dot = 0.0, ab = 0.0;
        const double ks = (double)d_Ks[sat(s, t, kv)];
        for (std::size_t d = 0; d < hd; ++d) {
          const double p = (double)bf16_to_float(w_Q[(s * qh + h) * hd + d]) * fp8_to_double(d_K[at(s, t) + kv * hd + d], f8);
          dot += p;
          ab += std::fabs(p);
        }
        sc[t] = (double)scale * (dot * ks);
        m = std::max(m, sc[t]);
        sabs = std::max(sabs, (double)scale * ks * ab);
      }
      for (std::size_t t = 0; t < L; ++t) l += (sc[t] = std::exp(sc[t] - m));
      const double delta = (double)(hd + 3) * std::ldexp(1.0, -24) * sabs;
      for (std::size_t d = 0; d < hd; ++d) {
        double acc = 0.0, aabs = 0.0;
        for (std::size_t t = 0; t < L; ++t) {
          const double v = (double)d_Vs[sat(s, t, kv)] * fp8_to_double(d_V[at(s, t) + kv * hd + d], f8);
          acc += sc[t] * v;
          aabs += sc[t] * std::fabs(v);
        }
        const double ref = acc / l, got = (double)bf16_to_float(d_O[(s * qh + h) * hd + d]), big = std::max(std::fabs(ref), std::fabs(got));
        const double ulp = std::ldexp(1.0, std::max(big > 0.0 ? (int)std::floor(std::log2(big)) : -126, -126) - 7);
        const double bound = 0.5 * ulp + (2.0 * std::ldexp(1.0, -8) + 2.0 * delta + (double)(L + hd + 17) * std::ldexp(1.0, -24)) * aabs / l;
        const double ratio = std::fabs(got - ref) / bound;
        worst = std::max(worst, ratio);
        bad_o += !(ratio <= 1.0);
      }
    }

  std::cout << "rope + quantising append + decode attention over the " << fname << " paged cache: " << seqs << " sequences, " << qh << " query heads on " << kvh
            << " KV heads, head_dim " << hd << ", context " << context << " in pages of " << ps << "; prefill of " << T << " tokens in the "
            << (rform == SM_ROPE_APPEND_FORM_BLOCK ? "block" : "wave") << " form, attention in the " << (aform == SM_ATTN_DECODE_FORM_DIRECT ? "direct" : "split")
            << " form; the cache holds " << 2 * (nkv + nsc * 4) << " bytes where the 16-bit cache holds " << 4 * nkv << std::endl;
  std::cout << "rotated Q of the decode step equal to the host loop of the definition: " << (bad_q ? "NO" : "yes") << std::endl;
  std::cout << "every byte of the K and V cache equal to the host loop: " << (bad_bytes ? "NO" : "yes") << std::endl;
  std::cout << "every scale of the K and V cache equal to the host loop: " << (bad_scales ? "NO" : "yes") << std::endl;
  std::cout << "attention output within the bound of the fp64 softmax over the dequantised cache (worst " << worst << " of it): " << (bad_o ? "NO" : "yes") << std::endl;
  for (void* p : {(void*)pre, (void*)dec, (void*)Kc, (void*)Vc, (void*)Ksc, (void*)Vsc, (void*)O, (void*)cs, (void*)bt, (void*)sl, (void*)dseq, (void*)dpos, ws})
    (void)hipFree(p);
  return !bad_q && !bad_bytes && !bad_scales && !bad_o ? EXIT_SUCCESS : EXIT_FAILURE;
}
