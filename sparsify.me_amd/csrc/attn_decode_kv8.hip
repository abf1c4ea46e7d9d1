// attn_decode_kv8.hip -- sm_attn_decode_kv8_{f16,bf16} (extension): sm_attn_decode_* over the fp8 cache of paged_kv.h -- K and V bytes
// with one fp32 scale per (token, kv head) -- at half the cache bytes.  Q, O and lse are the 16-bit call's, and so are the chunk, the forms,
// the workspace and the SPLIT form's combine kernel (attn_decode_common.h).  The definition (include/sparsifyme.h) changes two lines:
// s_t = (dot_t * ks_t) * scale, and acc_c,d = sum_t (fp32(p_t) * vs_t) * fp32(v8_t,d).
//
// The kernel keeps the shape of attn_decode_kernel: four waves per (sequence, kv head, chunk), wave w owns tokens w CHUNK/4 .. of the chunk.
//   scores  S^T = K Q^T on v_mfma_f32_16x16x32 in Q's 16-bit type.  A lane's K bytes go straight from the cache to registers, 16 contiguous
//           bytes of one token row per load, and are widened there (v_cvt_scalef32_pk_{f16,bf16}_{fp8,bf8} at scale 1: every e4m3 and e5m2
//           value is a value of fp16 and of bf16, so the widening is exact).  The 16 bytes feed TWO matrix instructions -- columns
//           64 u + 16 (l>>4) + 0..7 and + 8..15 -- and the lane's Q fragments take the same columns: the order of the sum is the kernel's.
//           ks multiplies the instruction's result, then scale.  The four ks (and vs) of a lane's tokens 4 (l>>4) + r of a tile are one
//           16-byte load where all four are live, selected single loads at the edge: a masked token's scale is never loaded.
//   mask, max, p, l   as in attn_decode_kernel; the lane that rounds p_t also forms fp32(p_t) * vs_t, and THAT goes to LDS.
//   P V     on the vector ALUs from bytes widened to fp32 (v_cvt_pk_f32_{fp8,bf8}), in attn_decode_kernel's own tiling: head_dim / 8 lanes own a
//           token row, 8 BYTES each (one 8-byte load).  16 bytes per lane were built and timed: they halve the lanes of a row, so the
//           cross-lane additions behind the loop grow from 2 - 3 levels over 8 GM values to 3 - 4 levels over 16 GM, and every cell of the
//           table was slower for it (head_dim 64 fell behind the 16-bit call); in the 16-row class they would also be 256 accumulators.
//   out     as in attn_decode_kernel; the partial sums have LDS of their own here (one barrier fewer).
#include "attn_decode_common.h"

namespace sm {

struct Ad8Args {
  const uint16_t* Q;
  const uint8_t *K, *V;
  const float *Ksc, *Vsc;
  const int *bt, *sl;
  uint16_t* O;
  float *lse, *ws_acc, *ws_ml;  // lse: or null; ws_*: null in the DIRECT form
  size_t ldq, ldkv, page_stride, scale_page_stride, ldbt, ldo;
  unsigned q_heads, kv_heads, group, num_pages, page_size, page_shift, cap, nchunks;  // bt .. cap: the PagedKv fields (paged_kv.h)
  float scale;
};

// two fp8 bytes (the low or the high half of w) -> two elements of Q's type, exactly
template <bool BF, int FMT, bool HI>
__device__ __forceinline__ uint32_t widen2(uint32_t w) {
  if constexpr (BF) {
    if constexpr (FMT == SM_FP8_E4M3) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI));
    else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_bf8(w, 1.0f, HI));
  } else {
    if constexpr (FMT == SM_FP8_E4M3) return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, 1.0f, HI));
    else return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_bf8(w, 1.0f, HI));
  }
}
// eight fp8 bytes -> one matrix-instruction fragment
template <bool BF, int FMT>
__device__ __forceinline__ h8 widen8(uint32_t w0, uint32_t w1) {
  const u4 v = {widen2<BF, FMT, false>(w0), widen2<BF, FMT, true>(w0), widen2<BF, FMT, false>(w1), widen2<BF, FMT, true>(w1)};
  return __builtin_bit_cast(h8, v);
}
// four fp8 bytes -> fp32
template <int FMT>
__device__ __forceinline__ void widen4_f32(uint32_t w, float* x) {
  f2 lo, hi;
  if constexpr (FMT == SM_FP8_E4M3) {
    lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  } else {
    lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false);
    hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
  }
  x[0] = lo[0]; x[1] = lo[1]; x[2] = hi[0]; x[3] = hi[1];
}
// the scales of tokens t0 + 4 kg + r of a tile: `n` of the four are live (from r = 0 on); one 16-byte load where all are
__device__ __forceinline__ f4 ad8_scales(const float* sc, unsigned n) {
  if (n >= 4u) return *reinterpret_cast<const f4*>(sc);
  f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
  if (n > 0u) v[0] = sc[0];
  if (n > 1u) v[1] = sc[1];
  if (n > 2u) v[2] = sc[2];
  return v;
}

template <bool BF, int FMT, int HD, int GM>
__global__ __launch_bounds__(256) void attn_decode_kv8_kernel(const Ad8Args p) {
  constexpr unsigned KP = HD / 64;            // 16-byte K loads per lane and tile; each feeds two matrix instructions
  constexpr unsigned VB = 8;                  // bytes (= columns) of a V row per lane (see above)
  constexpr unsigned LPT = HD / VB;           // lanes that own a token row of V
  constexpr unsigned TPS = 64 / LPT;          // tokens a wave takes per V step
  constexpr unsigned NVS = AD_TPW / TPS;      // V steps per wave
  static_assert(TPS <= 16 && 16 % TPS == 0, "a V step lies inside one tile");
  __shared__ __attribute__((aligned(16))) float lds_p[AD_CHUNK * 16];  // fp32(p) * vs, [wave][token][16]
  __shared__ __attribute__((aligned(16))) float lds_a[4 * GM * HD];    // acc [wave][GM][HD]
  __shared__ float lds_m[4][16], lds_l[4][16];

  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  unsigned b = blockIdx.x;
  const unsigned c = b % p.nchunks;
  b /= p.nchunks;
  const unsigned kvh = b % p.kv_heads, s = b / p.kv_heads;
  const unsigned L = ad_len(p, s), c0 = c * AD_CHUNK;
  const bool split = p.ws_acc != nullptr;
  const unsigned h0 = kvh * p.group;  // the group's first query head
  if (c0 >= L) {                      // (workgroup-uniform)
    if (!split) {                     // DIRECT, L == 0: +0 and -inf
      for (unsigned idx = tid; idx < p.group * HD; idx += 256u) p.O[(size_t)s * p.ldo + (size_t)h0 * HD + idx] = 0;
      if (p.lse && tid < p.group) p.lse[(size_t)s * p.q_heads + h0 + tid] = -INFINITY;
    }
    return;
  }
  const unsigned row = lane & 15u, kg = lane >> 4, w0 = c0 + wave * AD_TPW;

  // the page of every tile: read only for a tile that starts below L
  size_t pbase[AD_NT], sbase[AD_NT];
  bool present[AD_NT];
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i) {
    const unsigned t0 = w0 + i * 16u;
    int id = -1;
    if (t0 < L) id = kv_page_id(p, s, t0);
    present[i] = kv_present(p, id);
    pbase[i] = present[i] ? KV_OFFSET(p, id, t0) + (size_t)kvh * HD : 0;
    sbase[i] = present[i] ? KV8_SCALE_OFFSET(p, id, kvh, t0) : 0;
  }

  // Q: the B operand, rows beyond the group are zeros; fragment 2 u + v holds columns 64 u + 16 kg + 8 v + 0..7, the columns of K's bytes
  h8 qf[2 * KP];
  {
    const uint16_t* qp = p.Q + (size_t)s * p.ldq + (size_t)(h0 + row) * HD + kg * 16u;
#pragma unroll
    for (unsigned f = 0; f < 2 * KP; ++f)
      qf[f] = row < p.group ? *reinterpret_cast<const h8*>(qp + (f >> 1) * 64u + (f & 1u) * 8u) : h8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  // K: token w0 + 16 i + row, 16 bytes per lane and pair of matrix instructions
  u4 kb[AD_NT][KP];
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i) {
    const bool live = present[i] && w0 + i * 16u + row < L;
    const uint8_t* kp = p.K + pbase[i] + (size_t)row * p.ldkv + kg * 16u;
#pragma unroll
    for (unsigned u = 0; u < KP; ++u) kb[i][u] = live ? *reinterpret_cast<const u4*>(kp + u * 64u) : u4{0u, 0u, 0u, 0u};
  }
  // the scales of this lane's tokens w0 + 16 i + 4 kg + r
  f4 ksc[AD_NT], vsc[AD_NT];
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i) {
    const unsigned t = w0 + i * 16u + kg * 4u;
    const unsigned n = present[i] && t < L ? L - t : 0u;
    ksc[i] = ad8_scales(p.Ksc + sbase[i] + kg * 4u, n);
    vsc[i] = ad8_scales(p.Vsc + sbase[i] + kg * 4u, n);
  }
  // V: step j takes tokens w0 + TPS j + lane / LPT, VB bytes from column VB (lane % LPT); in flight across the softmax
  const unsigned vt = lane / LPT, vd = (lane % LPT) * VB;
  uint32_t vf[NVS][VB / 4];
#pragma unroll
  for (unsigned j = 0; j < NVS; ++j) {
    const unsigned i = j * TPS / 16u, tl = j * TPS + vt;  // tile, token inside the wave's range
    const bool live = present[i] && w0 + tl < L;
    const uint8_t* vp = p.V + pbase[i] + (size_t)(tl - i * 16u) * p.ldkv + vd;
    const u2 v = live ? *reinterpret_cast<const u2*>(vp) : u2{0u, 0u};
    vf[j][0] = v[0];
    vf[j][1] = v[1];
  }

  f4 sc[AD_NT];
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i) {
    sc[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (unsigned u = 0; u < KP; ++u) {
      sc[i] = mfma16<BF>(widen8<BF, FMT>(kb[i][u][0], kb[i][u][1]), qf[2 * u], sc[i]);
      sc[i] = mfma16<BF>(widen8<BF, FMT>(kb[i][u][2], kb[i][u][3]), qf[2 * u + 1], sc[i]);
    }
  }

  // scores, masked by selection, and their maximum per q row (this lane's q row is `row`)
  float m = -INFINITY;
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i)
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      const bool live = present[i] && w0 + i * 16u + kg * 4u + r < L;
      sc[i][r] = live ? (sc[i][r] * ksc[i][r]) * p.scale : -INFINITY;
      m = __builtin_fmaxf(m, sc[i][r]);
    }
  m = __builtin_fmaxf(m, __shfl_xor(m, 16));
  m = __builtin_fmaxf(m, __shfl_xor(m, 32));
  if (kg == 0) lds_m[wave][row] = m;
  __syncthreads();
  m = __builtin_fmaxf(__builtin_fmaxf(lds_m[0][row], lds_m[1][row]), __builtin_fmaxf(lds_m[2][row], lds_m[3][row]));

  // p rounded to the type, l from the rounded values; fp32(p) * vs, one rounded multiply, is what the product takes
  float* P = lds_p + wave * (AD_TPW * 16u);
  float l = 0.0f;
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i)
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      const bool live = present[i] && w0 + i * 16u + kg * 4u + r < L;
      const float pr = live ? to_f32<BF>(to_elt<BF>(ad_exp(sc[i][r] - m))) : 0.0f;
      l += pr;
      P[(i * 16u + kg * 4u + r) * 16u + row] = live ? pr * vsc[i][r] : 0.0f;
    }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (kg == 0) lds_l[wave][row] = l;
  __syncthreads();

  // P V: acc[g][e] for q row g, column vd + e, over this lane's tokens
  float acc[GM][VB];
#pragma unroll
  for (int g = 0; g < GM; ++g)
#pragma unroll
    for (unsigned e = 0; e < VB; ++e) acc[g][e] = 0.0f;
#pragma unroll
  for (unsigned j = 0; j < NVS; ++j) {
    float v[VB];
#pragma unroll
    for (unsigned e = 0; e < VB / 4; ++e) widen4_f32<FMT>(vf[j][e], v + 4 * e);
    const float* pj = P + (j * TPS + vt) * 16u;
#pragma unroll
    for (int g4 = 0; g4 < GM / 4; ++g4) {
      const f4 pq = *reinterpret_cast<const f4*>(pj + 4 * g4);
#pragma unroll
      for (int gi = 0; gi < 4; ++gi)
#pragma unroll
        for (unsigned e = 0; e < VB; ++e) acc[4 * g4 + gi][e] = __builtin_fmaf(pq[gi], v[e], acc[4 * g4 + gi][e]);
    }
  }
  // the lanes of a column, then the waves
#pragma unroll
  for (unsigned off = LPT; off < 64u; off <<= 1)
#pragma unroll
    for (int g = 0; g < GM; ++g)
#pragma unroll
      for (unsigned e = 0; e < VB; ++e) acc[g][e] += __shfl_xor(acc[g][e], (int)off);
  if (lane < LPT) {
#pragma unroll
    for (int g = 0; g < GM; ++g) {
      float* a = lds_a + (wave * GM + g) * HD + vd;
#pragma unroll
      for (unsigned e = 0; e < VB; e += 4) *reinterpret_cast<f4*>(a + e) = f4{acc[g][e], acc[g][e + 1], acc[g][e + 2], acc[g][e + 3]};
    }
  }
  __syncthreads();

  for (unsigned idx = tid; idx < p.group * HD; idx += 256u) {
    const unsigned g = idx / HD, d = idx % HD, h = h0 + g;
    const float a = ((lds_a[(0 * GM + g) * HD + d] + lds_a[(1 * GM + g) * HD + d]) + lds_a[(2 * GM + g) * HD + d]) + lds_a[(3 * GM + g) * HD + d];
    const float lg = ((lds_l[0][g] + lds_l[1][g]) + lds_l[2][g]) + lds_l[3][g];
    const float mg = __builtin_fmaxf(__builtin_fmaxf(lds_m[0][g], lds_m[1][g]), __builtin_fmaxf(lds_m[2][g], lds_m[3][g]));
    if (split) {
      const size_t rec = ((size_t)s * p.q_heads + h) * p.nchunks + c;
      p.ws_acc[rec * HD + d] = a;
      if (d == 0) {
        p.ws_ml[rec * 2] = mg;
        p.ws_ml[rec * 2 + 1] = lg;
      }
    } else {
      const bool none = mg == -INFINITY;  // every page absent
      p.O[(size_t)s * p.ldo + (size_t)h * HD + d] = __builtin_bit_cast(uint16_t, to_elt<BF>(none ? 0.0f : a / lg));
      if (d == 0 && p.lse) p.lse[(size_t)s * p.q_heads + h] = none ? -INFINITY : mg + logf(lg);
    }
  }
}

template <bool BF, int FMT, int HD>
static int attn_decode_kv8_launch(const Ad8Args& a, size_t seqs, bool split, hipStream_t st) {
  static const char* const who = "sm_attn_decode_kv8_{f16,bf16}";
  const size_t nwg = seqs * a.kv_heads * a.nchunks;  // (each factor < 2^31 and seqs * kv_heads < 2^31: no overflow)
  int rc;
  if (a.group <= 4) rc = launch_grid<attn_decode_kv8_kernel<BF, FMT, HD, 4>>(nwg, 256, LDS_NO_OPTIN, 0, st, who, "attn_decode_kv8_kernel", a);
  else rc = launch_grid<attn_decode_kv8_kernel<BF, FMT, HD, 16>>(nwg, 256, LDS_NO_OPTIN, 0, st, who, "attn_decode_kv8_kernel", a);
  if (rc != SM_STATUS_SUCCESS || !split) return rc;
  AdArgs cmb = {};  // the 16-bit call's combine, unchanged: it reads the lengths, the workspace and where O and lse go
  cmb.sl = a.sl; cmb.O = a.O; cmb.lse = a.lse; cmb.ws_acc = a.ws_acc; cmb.ws_ml = a.ws_ml; cmb.ldo = a.ldo;
  cmb.q_heads = a.q_heads; cmb.cap = a.cap; cmb.nchunks = a.nchunks;
  return launch_grid<attn_combine_kernel<BF, HD>>(seqs * a.q_heads, HD, LDS_NO_OPTIN, 0, st, who, "attn_combine_kernel", cmb);
}

template <bool BF>
static int attn_decode_kv8(const void* Q, const void* Kc8, const void* Vc8, const float* Ksc, const float* Vsc, const int* block_table, const int* seq_lens, void* O,
                           float* lse, void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t num_pages,
                           size_t page_size, size_t max_pages, size_t ldq, size_t ldkv, size_t page_stride, size_t scale_page_stride, size_t ldbt, size_t ldo,
                           float scale, int fmt, sm_stream_t stream) {
  static const char* const who = "sm_attn_decode_kv8_{f16,bf16}";
  if (!Q || !Kc8 || !Vc8 || !Ksc || !Vsc || !block_table || !seq_lens || !O) {
    set_error("%s: invalid argument (null Q, Kc8, Vc8, Ksc, Vsc, block_table, seq_lens or O)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (ldq < mul_sat(q_heads, head_dim) || ldo < mul_sat(q_heads, head_dim) ||
      !kv_pitches_ok(mul_sat(kv_heads, head_dim), page_size, max_pages, ldkv, page_stride, ldbt)) {
    set_error("%s: invalid argument (a pitch below its extent: ldq, ldo >= q_heads * head_dim, ldkv >= kv_heads * head_dim, page_stride >= page_size * ldkv, "
              "ldbt >= max_pages)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!fmt_ok(fmt)) {
    set_error("%s: invalid argument (fmt is SM_FP8_E4M3 or SM_FP8_E5M2)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!kv8_scale_pitch_ok(kv_heads, page_size, scale_page_stride)) {
    set_error("%s: invalid argument (scale_page_stride below kv_heads * page_size)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (q_heads > 0 && kv_heads == 0) {
    set_error("%s: invalid argument (kv_heads is 0)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (q_heads > 0 && q_heads % kv_heads != 0) {
    set_error("%s: invalid argument (q_heads is not a multiple of kv_heads)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  const bool split = mul_sat(page_size, max_pages) > AD_CHUNK;
  if (split && (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3u) != 0 ||
                workspace_bytes < attn_decode_ws_bytes(seqs, q_heads, head_dim, page_size, max_pages))) {
    set_error("%s: invalid argument (max_pages * page_size exceeds SM_ATTN_DECODE_CHUNK (%d): the SPLIT form needs a 4-byte aligned workspace of "
              "sm_attn_decode_workspace_size bytes; it is null, misaligned or short)", who, (int)AD_CHUNK);
    return SM_STATUS_INVALID_VALUE;
  }
  if (scale != scale) {
    set_error("%s: invalid argument (scale is NaN)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  const size_t lim = KV_I32_MAX;
  if (seqs > lim || q_heads > lim || kv_heads > lim || head_dim > lim || ldq > lim || ldo > lim || mul_sat(q_heads, head_dim) > lim ||
      mul_sat(kv_heads, head_dim) > lim || mul_sat(seqs, q_heads) > lim || scale_page_stride > lim ||
      !kv_fields_fit(num_pages, page_size, max_pages, ldkv, page_stride, ldbt)) {
    set_error("%s: a dimension, a pitch, q_heads * head_dim, kv_heads * head_dim or seqs * q_heads exceeds 2^31-1", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!ad_head_dim_ok(head_dim)) {
    set_error("%s: head_dim is SM_ATTN_DECODE_MIN_HEAD_DIM (%d) or SM_ATTN_DECODE_MAX_HEAD_DIM (%d)", who, SM_ATTN_DECODE_MIN_HEAD_DIM, SM_ATTN_DECODE_MAX_HEAD_DIM);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!kv_page_size_ok(page_size)) {
    set_error("%s: page_size is a power of two from SM_ATTN_DECODE_MIN_PAGE_SIZE (%d) to SM_ATTN_DECODE_MAX_PAGE_SIZE (%d)", who, SM_ATTN_DECODE_MIN_PAGE_SIZE,
              SM_ATTN_DECODE_MAX_PAGE_SIZE);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (q_heads > 0 && q_heads / kv_heads > SM_ATTN_DECODE_MAX_GROUP) {
    set_error("%s: the group q_heads / kv_heads exceeds SM_ATTN_DECODE_MAX_GROUP (%d)", who, SM_ATTN_DECODE_MAX_GROUP);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!kv_context_fits(page_size, max_pages)) {
    set_error("%s: max_pages * page_size exceeds 2^31-1 (SM_ATTN_DECODE_MAX_CONTEXT)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!aligned16(Q) || !aligned16(O) || ldq % 8 != 0 || ldo % 8 != 0) {
    set_error("%s: needs 16-byte aligned rows of Q and O (pointer, ldq, ldo %% 8 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!aligned16(Kc8) || !aligned16(Vc8) || !kv8_rows_aligned16(ldkv, page_stride) || !aligned16(Ksc) || !aligned16(Vsc) ||
      !kv8_scale_rows_aligned16(scale_page_stride)) {
    set_error("%s: needs 16-byte aligned rows of Kc8 and Vc8 (pointer, ldkv, page_stride %% 16 == 0) and of Ksc and Vsc (pointer, scale_page_stride %% 4 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (seqs == 0 || q_heads == 0) return SM_STATUS_SUCCESS;
  Ad8Args a = {};
  a.Q = (const uint16_t*)Q; a.K = (const uint8_t*)Kc8; a.V = (const uint8_t*)Vc8; a.Ksc = Ksc; a.Vsc = Vsc; a.sl = seq_lens; a.O = (uint16_t*)O; a.lse = lse;
  a.ldq = ldq; a.ldo = ldo; a.scale_page_stride = scale_page_stride;
  paged_kv_fill(a, block_table, num_pages, page_size, max_pages, ldkv, page_stride, ldbt);
  a.q_heads = (unsigned)q_heads; a.kv_heads = (unsigned)kv_heads; a.group = (unsigned)(q_heads / kv_heads);
  a.nchunks = (unsigned)(split ? ad_chunks(page_size, max_pages) : 1);
  a.scale = scale;
  if (split) {
    a.ws_acc = (float*)workspace;
    a.ws_ml = a.ws_acc + seqs * q_heads * a.nchunks * head_dim;
  }
  // (max_pages == 0: DIRECT with one workgroup per (sequence, kv head), whose L == 0 path writes +0 and -inf)
  hipStream_t st = (hipStream_t)stream;
  if (fmt == SM_FP8_E4M3)
    return head_dim == 64 ? attn_decode_kv8_launch<BF, SM_FP8_E4M3, 64>(a, seqs, split, st) : attn_decode_kv8_launch<BF, SM_FP8_E4M3, 128>(a, seqs, split, st);
  return head_dim == 64 ? attn_decode_kv8_launch<BF, SM_FP8_E5M2, 64>(a, seqs, split, st) : attn_decode_kv8_launch<BF, SM_FP8_E5M2, 128>(a, seqs, split, st);
}

}  // namespace sm

using namespace sm;

extern "C" int sm_attn_decode_kv8_f16(const void* Q, const void* Kc8, const void* Vc8, const float* Ksc, const float* Vsc, const int* block_table, const int* seq_lens,
                                      void* O, float* lse, void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim,
                                      size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldkv, size_t page_stride, size_t scale_page_stride,
                                      size_t ldbt, size_t ldo, float scale, int fmt, sm_stream_t stream) {
  return attn_decode_kv8<false>(Q, Kc8, Vc8, Ksc, Vsc, block_table, seq_lens, O, lse, workspace, workspace_bytes, seqs, q_heads, kv_heads, head_dim, num_pages,
                                page_size, max_pages, ldq, ldkv, page_stride, scale_page_stride, ldbt, ldo, scale, fmt, stream);
}
extern "C" int sm_attn_decode_kv8_bf16(const void* Q, const void* Kc8, const void* Vc8, const float* Ksc, const float* Vsc, const int* block_table, const int* seq_lens,
                                       void* O, float* lse, void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim,
                                       size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldkv, size_t page_stride, size_t scale_page_stride,
                                       size_t ldbt, size_t ldo, float scale, int fmt, sm_stream_t stream) {
  return attn_decode_kv8<true>(Q, Kc8, Vc8, Ksc, Vsc, block_table, seq_lens, O, lse, workspace, workspace_bytes, seqs, q_heads, kv_heads, head_dim, num_pages,
                               page_size, max_pages, ldq, ldkv, page_stride, scale_page_stride, ldbt, ldo, scale, fmt, stream);
}
