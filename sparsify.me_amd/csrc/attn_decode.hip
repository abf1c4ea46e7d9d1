// attn_decode.hip -- sm_attn_decode_{f16,bf16} (extension): single-query attention over a paged KV cache, grouped query heads, the
// context split into chunks of SM_ATTN_DECODE_CHUNK tokens.  The definition (include/sparsifyme.h) is fp32 to the operation; the kernel
// owns only the order of the sums inside a chunk, and that order is a function of the chunk alone.
//
// One workgroup of four waves handles one (sequence, kv head, chunk); wave w owns tokens w CHUNK/4 .. + CHUNK/4 - 1 of the chunk.
//   scores  S^T = K Q^T on v_mfma_f32_16x16x32: the TOKEN is the instruction's row, so a lane's K fragment is 16 contiguous bytes of
//           one token row (A: row l&15, k = 8 (l>>4) + j), loaded straight from the cache to registers; the group's query rows, zero
//           padded to 16, are the B operand (col l&15).  All K loads of a wave are issued before the first matrix instruction.
//           D: lane l holds q row l&15 at tokens 4 (l>>4) + r of each 16-token tile.  A tile lies inside one page (tiles start on
//           multiples of 16, pages hold at least 16 tokens): one block-table read per tile, and only for tiles that start below L.
//   mask    by selection: a token at or beyond L, or of an absent page (paged_kv.h), is never loaded (its K and V fragments are zeros made in
//           registers), its score is -inf and its p is +0.
//   max     over the lane's registers, the four lane groups (xor 16, 32), the four waves (LDS).
//   p       exp2f((s - m) log2e) by v_exp_f32, rounded to the 16-bit type; l sums the rounded values; p goes to LDS as [token][q row].
//   P V     on the vector ALUs: 8 (head_dim 64) or 16 (128) lanes own a token row of V, 16 bytes each, loaded straight to registers
//           (issued before the softmax, consumed after it); a lane reads its token's p for the group's rows from LDS (a broadcast
//           read) and keeps acc[row][8] in registers; the lanes of a column are then added (xor 8 / 16 / 32) and the four waves through
//           LDS, (((w0 + w1) + w2) + w3).
//   out     DIRECT: O = rne16(acc / l), lse = m + logf(l) from this kernel.  SPLIT: (acc, m, l) to the workspace; attn_combine_kernel
//           merges a sequence's ceil(L / CHUNK) chunks in ascending order.
// Two group classes: rows held per lane GM = 4 (group <= 4) and GM = 16.
#include "attn_decode_common.h"  // the chunk, the form, the workspace, AdArgs, ad_len, ad_exp, attn_combine_kernel

namespace sm {

template <bool BF, int HD, int GM>
__global__ __launch_bounds__(256) void attn_decode_kernel(const AdArgs p) {
  constexpr unsigned KS = HD / 32;       // matrix instructions per tile
  constexpr unsigned LPT = HD / 8;       // lanes that own a token row of V
  constexpr unsigned TPS = 64 / LPT;     // tokens a wave takes per V step
  constexpr unsigned NVS = AD_TPW / TPS;  // V steps per wave
  constexpr unsigned P_FLOATS = AD_CHUNK * 16, A_FLOATS = 4 * GM * HD;
  __shared__ __attribute__((aligned(16))) float lds_pa[P_FLOATS > A_FLOATS ? P_FLOATS : A_FLOATS];  // p [wave][token][16], then acc [wave][GM][HD]
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
  size_t pbase[AD_NT];
  bool present[AD_NT];
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i) {
    const unsigned t0 = w0 + i * 16u;
    int id = -1;
    if (t0 < L) id = kv_page_id(p, s, t0);
    present[i] = kv_present(p, id);
    pbase[i] = present[i] ? KV_OFFSET(p, id, t0) + (size_t)kvh * HD : 0;
  }

  // Q: the B operand, rows beyond the group are zeros
  h8 qf[KS];
  {
    const uint16_t* qp = p.Q + (size_t)s * p.ldq + (size_t)(h0 + row) * HD + kg * 8u;
#pragma unroll
    for (unsigned ks = 0; ks < KS; ++ks) qf[ks] = row < p.group ? *reinterpret_cast<const h8*>(qp + ks * 32u) : h8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  // K: token w0 + 16 i + row, 16 bytes per lane and matrix instruction
  h8 kf[AD_NT][KS];
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i) {
    const bool live = present[i] && w0 + i * 16u + row < L;
    const uint16_t* kp = p.K + pbase[i] + (size_t)row * p.ldkv + kg * 8u;
#pragma unroll
    for (unsigned ks = 0; ks < KS; ++ks) kf[i][ks] = live ? *reinterpret_cast<const h8*>(kp + ks * 32u) : h8{0, 0, 0, 0, 0, 0, 0, 0};
  }
  f4 sc[AD_NT];
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i) {
    sc[i] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (unsigned ks = 0; ks < KS; ++ks) sc[i] = mfma16<BF>(kf[i][ks], qf[ks], sc[i]);
  }
  // V: step j takes tokens w0 + TPS j + lane / LPT, 8 elements from column 8 (lane % LPT); in flight across the softmax
  const unsigned vt = lane / LPT, vd = (lane % LPT) * 8u;
  u4 vf[NVS];
#pragma unroll
  for (unsigned j = 0; j < NVS; ++j) {
    const unsigned i = j * TPS / 16u, tl = j * TPS + vt;  // tile, token inside the wave's range
    const bool live = present[i] && w0 + tl < L;
    vf[j] = live ? *reinterpret_cast<const u4*>(p.V + pbase[i] + (size_t)(tl - i * 16u) * p.ldkv + vd) : u4{0u, 0u, 0u, 0u};
  }

  // scores, masked by selection, and their maximum per q row (this lane's q row is `row`)
  float m = -INFINITY;
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i)
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      const bool live = present[i] && w0 + i * 16u + kg * 4u + r < L;
      sc[i][r] = live ? sc[i][r] * p.scale : -INFINITY;
      m = __builtin_fmaxf(m, sc[i][r]);
    }
  m = __builtin_fmaxf(m, __shfl_xor(m, 16));
  m = __builtin_fmaxf(m, __shfl_xor(m, 32));
  if (kg == 0) lds_m[wave][row] = m;
  __syncthreads();
  m = __builtin_fmaxf(__builtin_fmaxf(lds_m[0][row], lds_m[1][row]), __builtin_fmaxf(lds_m[2][row], lds_m[3][row]));

  // p rounded to the type, l from the rounded values
  float* P = lds_pa + wave * (AD_TPW * 16u);
  float l = 0.0f;
#pragma unroll
  for (unsigned i = 0; i < AD_NT; ++i)
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      const bool live = present[i] && w0 + i * 16u + kg * 4u + r < L;
      const float pr = live ? to_f32<BF>(to_elt<BF>(ad_exp(sc[i][r] - m))) : 0.0f;
      l += pr;
      P[(i * 16u + kg * 4u + r) * 16u + row] = pr;
    }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (kg == 0) lds_l[wave][row] = l;
  __syncthreads();

  // P V: acc[g][e] for q row g, column vd + e, over this lane's tokens
  float acc[GM][8];
#pragma unroll
  for (int g = 0; g < GM; ++g)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[g][e] = 0.0f;
#pragma unroll
  for (unsigned j = 0; j < NVS; ++j) {
    float v[8];  // (unpack8 of quant_fp8.h, written out: through the call the CHUNK 512 build pairs the bf16 conversions differently, 118 -> 120 AGPRs)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[2 * e] = Src16<BF>::f32(vf[j][e] & 0xffffu);
      v[2 * e + 1] = Src16<BF>::f32(vf[j][e] >> 16);
    }
    const float* pj = P + (j * TPS + vt) * 16u;
#pragma unroll
    for (int g4 = 0; g4 < GM / 4; ++g4) {
      const f4 pq = *reinterpret_cast<const f4*>(pj + 4 * g4);
#pragma unroll
      for (int gi = 0; gi < 4; ++gi)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[4 * g4 + gi][e] = __builtin_fmaf(pq[gi], v[e], acc[4 * g4 + gi][e]);
    }
  }
  // the lanes of a column, then the waves
#pragma unroll
  for (unsigned off = LPT; off < 64u; off <<= 1)
#pragma unroll
    for (int g = 0; g < GM; ++g)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] += __shfl_xor(acc[g][e], (int)off);
  __syncthreads();  // every wave has read its p: the region becomes acc [wave][GM][HD]
  if (lane < LPT) {
#pragma unroll
    for (int g = 0; g < GM; ++g) {
      float* a = lds_pa + (wave * GM + g) * HD + vd;
      *reinterpret_cast<f4*>(a) = f4{acc[g][0], acc[g][1], acc[g][2], acc[g][3]};
      *reinterpret_cast<f4*>(a + 4) = f4{acc[g][4], acc[g][5], acc[g][6], acc[g][7]};
    }
  }
  __syncthreads();

  for (unsigned idx = tid; idx < p.group * HD; idx += 256u) {
    const unsigned g = idx / HD, d = idx % HD, h = h0 + g;
    const float a = ((lds_pa[(0 * GM + g) * HD + d] + lds_pa[(1 * GM + g) * HD + d]) + lds_pa[(2 * GM + g) * HD + d]) + lds_pa[(3 * GM + g) * HD + d];
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

template <bool BF, int HD>
static int attn_decode_launch(const AdArgs& a, size_t seqs, bool split, hipStream_t st) {
  static const char* const who = "sm_attn_decode_{f16,bf16}";
  const size_t nwg = seqs * a.kv_heads * a.nchunks;  // (each factor < 2^31 and seqs * kv_heads < 2^31: no overflow)
  int rc;
  if (a.group <= 4) rc = launch_grid<attn_decode_kernel<BF, HD, 4>>(nwg, 256, LDS_NO_OPTIN, 0, st, who, "attn_decode_kernel", a);
  else rc = launch_grid<attn_decode_kernel<BF, HD, 16>>(nwg, 256, LDS_NO_OPTIN, 0, st, who, "attn_decode_kernel", a);
  if (rc != SM_STATUS_SUCCESS || !split) return rc;
  return launch_grid<attn_combine_kernel<BF, HD>>(seqs * a.q_heads, HD, LDS_NO_OPTIN, 0, st, who, "attn_combine_kernel", a);
}

template <bool BF>
static int attn_decode(const void* Q, const void* Kc, const void* Vc, const int* block_table, const int* seq_lens, void* O, float* lse, void* workspace,
                       size_t workspace_bytes, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t num_pages, size_t page_size,
                       size_t max_pages, size_t ldq, size_t ldkv, size_t page_stride, size_t ldbt, size_t ldo, float scale, sm_stream_t stream) {
  static const char* const who = "sm_attn_decode_{f16,bf16}";
  if (!Q || !Kc || !Vc || !block_table || !seq_lens || !O) {
    set_error("%s: invalid argument (null Q, Kc, Vc, block_table, seq_lens or O)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (ldq < mul_sat(q_heads, head_dim) || ldo < mul_sat(q_heads, head_dim) ||
      !kv_pitches_ok(mul_sat(kv_heads, head_dim), page_size, max_pages, ldkv, page_stride, ldbt)) {
    set_error("%s: invalid argument (a pitch below its extent: ldq, ldo >= q_heads * head_dim, ldkv >= kv_heads * head_dim, page_stride >= page_size * ldkv, "
              "ldbt >= max_pages)", who);
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
      mul_sat(kv_heads, head_dim) > lim || mul_sat(seqs, q_heads) > lim || !kv_fields_fit(num_pages, page_size, max_pages, ldkv, page_stride, ldbt)) {
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
  if (!aligned16(Q) || !aligned16(Kc) || !aligned16(Vc) || !aligned16(O) || ldq % 8 != 0 || ldo % 8 != 0 || !kv_rows_aligned16(ldkv, page_stride)) {
    set_error("%s: needs 16-byte aligned rows of Q, Kc, Vc and O (pointer, ldq, ldkv, page_stride, ldo %% 8 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (seqs == 0 || q_heads == 0) return SM_STATUS_SUCCESS;
  AdArgs a = {};
  a.Q = (const uint16_t*)Q; a.K = (const uint16_t*)Kc; a.V = (const uint16_t*)Vc; a.sl = seq_lens; a.O = (uint16_t*)O; a.lse = lse;
  a.ldq = ldq; a.ldo = ldo;
  paged_kv_fill(a, block_table, num_pages, page_size, max_pages, ldkv, page_stride, ldbt);
  a.q_heads = (unsigned)q_heads; a.kv_heads = (unsigned)kv_heads; a.group = (unsigned)(q_heads / kv_heads);
  a.nchunks = (unsigned)(split ? ad_chunks(page_size, max_pages) : 1);
  a.scale = scale;
  if (split) {
    a.ws_acc = (float*)workspace;
    a.ws_ml = a.ws_acc + seqs * q_heads * a.nchunks * head_dim;
  }
  // (max_pages == 0: DIRECT with one workgroup per (sequence, kv head), whose L == 0 path writes +0 and -inf)
  return head_dim == 64 ? attn_decode_launch<BF, 64>(a, seqs, split, (hipStream_t)stream) : attn_decode_launch<BF, 128>(a, seqs, split, (hipStream_t)stream);
}

}  // namespace sm

using namespace sm;

extern "C" int sm_attn_decode_form(size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t page_size, size_t max_pages, int* form) {
  if (!form) {
    set_error("sm_attn_decode_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = attn_decode_form(seqs, q_heads, kv_heads, head_dim, page_size, max_pages);
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_attn_decode_workspace_size(size_t seqs, size_t q_heads, size_t head_dim, size_t page_size, size_t max_pages, size_t* bytes) {
  if (!bytes) {
    set_error("sm_attn_decode_workspace_size: invalid argument (bytes is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  const size_t n = attn_decode_ws_bytes(seqs, q_heads, head_dim, page_size, max_pages);
  if (n == SIZE_MAX) {
    set_error("sm_attn_decode_workspace_size: the size overflows size_t");
    return SM_STATUS_NOT_SUPPORTED;
  }
  *bytes = n;
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_attn_decode_f16(const void* Q, const void* Kc, const void* Vc, const int* block_table, const int* seq_lens, void* O, float* lse,
                                  void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t num_pages,
                                  size_t page_size, size_t max_pages, size_t ldq, size_t ldkv, size_t page_stride, size_t ldbt, size_t ldo, float scale,
                                  sm_stream_t stream) {
  return attn_decode<false>(Q, Kc, Vc, block_table, seq_lens, O, lse, workspace, workspace_bytes, seqs, q_heads, kv_heads, head_dim, num_pages, page_size,
                            max_pages, ldq, ldkv, page_stride, ldbt, ldo, scale, stream);
}
extern "C" int sm_attn_decode_bf16(const void* Q, const void* Kc, const void* Vc, const int* block_table, const int* seq_lens, void* O, float* lse,
                                   void* workspace, size_t workspace_bytes, size_t seqs, size_t q_heads, size_t kv_heads, size_t head_dim, size_t num_pages,
                                   size_t page_size, size_t max_pages, size_t ldq, size_t ldkv, size_t page_stride, size_t ldbt, size_t ldo, float scale,
                                   sm_stream_t stream) {
  return attn_decode<true>(Q, Kc, Vc, block_table, seq_lens, O, lse, workspace, workspace_bytes, seqs, q_heads, kv_heads, head_dim, num_pages, page_size,
                           max_pages, ldq, ldkv, page_stride, ldbt, ldo, scale, stream);
}
