// rope_append.hip -- sm_rope_append_{f16,bf16} (extension): rotate every Q and K head of a token by its row of the caller's cos/sin table
// and write K and V into the token's slot of the paged cache sm_attn_decode_* reads, in one launch.  The definition (include/sparsifyme.h)
// fixes every operation -- two rounded fp32 products, one rounded sum, one rounding to the 16-bit type, never contracted -- so the op is a
// byte stream with fixed bits: Q, K, V and one table row are read once, Qo, Ko and two cache rows written once.
//
// A lane owns one ITEM of a head and keeps it for the whole token: under SM_ROPE_NEOX the 16-byte piece at column 8 j and its partner
// `half` columns on (eight pairs, c and s eight floats each), under SM_ROPE_INTERLEAVED one 16-byte piece (four pairs, c and s four floats
// each); the pieces at or beyond rot_dim are items that are copied.  A head has L items (at most 32), a wave step takes 64 / L heads, and
// the lanes walk the token's q_heads Q heads, kv_heads K heads and -- when the cache is written -- kv_heads V heads (V is copied through
// the same pieces).  The lane's c / s values are loaded once per token.  Every load of a head step is issued before its first store, and a
// lane stores exactly the elements it loaded: Qo == Q and Ko == K are safe by construction.
//   BLOCK  one four-wave workgroup per token, head step h = wave * (64 / L) + lane / L, stride 4 * (64 / L): the decode regime
//   WAVE   one wave per token, four tokens per workgroup, stride 64 / L: the prefill regime
// The token's sequence, position, table entry and page offset are wave-uniform: read once per wave and kept in SGPRs.  A padding token's
// wave leaves before any load.  No LDS, no barrier, no atomics.  The cache, its page lookup and the geometry the entry point checks: paged_kv.h.
#include "mma_tile.h"
#include "paged_kv.h"
#include "quant_fp8.h"
#include "rope_common.h"  // ra_style_ok, ra_rot

namespace sm {

// tools/rope_append_table.py builds this file alone with the threshold forced to 0 (every count runs WAVE) and to 2^31 - 1 (BLOCK)
#ifndef ROPE_APPEND_BLOCK_MAX
#define ROPE_APPEND_BLOCK_MAX SM_ROPE_APPEND_BLOCK_MAX_TOKENS
#endif

inline int rope_append_form(size_t tokens, size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim) {
  const size_t lim = 0x7fffffffull;
  if (tokens > lim || q_heads > lim || kv_heads > lim || mul_sat(q_heads, head_dim) > lim || mul_sat(kv_heads, head_dim) > lim) return SM_ROPE_APPEND_FORM_INVALID;
  if (head_dim % 8 != 0 || head_dim > SM_ROPE_APPEND_MAX_HEAD_DIM || rot_dim > head_dim || rot_dim % 16 != 0) return SM_ROPE_APPEND_FORM_INVALID;
  if (tokens == 0 || q_heads + kv_heads == 0 || head_dim == 0) return SM_ROPE_APPEND_FORM_EMPTY;
  return tokens <= (size_t)ROPE_APPEND_BLOCK_MAX ? SM_ROPE_APPEND_FORM_BLOCK : SM_ROPE_APPEND_FORM_WAVE;
}

struct RaArgs {
  const uint16_t *Q, *K, *V;
  uint16_t *Qo, *Ko, *Kc, *Vc;  // Ko: or null; Kc, Vc: both or neither
  const float* cs;              // or null (rot == 0)
  const int *pos, *tseq, *sl, *bt;
  size_t ldq, ldk, ldv, ldqo, ldko, ldkv, page_stride, ldcs, ldbt;
  unsigned tokens, seqs, q_heads, kv_heads, hd, rot, half, pos_end, num_pages, page_size, page_shift, cap;  // the PagedKv fields (paged_kv.h): zeros without a cache
  unsigned items, rot_items, hps;  // items per head, how many of them rotate, heads per wave step (64 / items)
};

template <bool BF, bool NEOX, bool BLOCK>
__global__ __launch_bounds__(256) void rope_append_kernel(const RaArgs p) {
  constexpr unsigned NC = NEOX ? 8 : 4;  // c / s values a rotating lane holds
  const unsigned lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned i = BLOCK ? blockIdx.x : blockIdx.x * 4u + wave;  // the token (wave-uniform)
  if (i >= p.tokens) return;
  // the token's sequence and position: no address is formed from an id out of range
  int s = p.tseq ? p.tseq[i] : (int)i;
  s = __builtin_amdgcn_readfirstlane(s);
  const bool s_ok = s >= 0 && (unsigned)s < p.seqs;
  int pos = p.pos ? p.pos[i] : (s_ok ? p.sl[s] - 1 : -1);
  pos = __builtin_amdgcn_readfirstlane(pos);
  if (pos < 0 || (unsigned)pos >= p.pos_end) return;  // a padding token: nothing read, nothing written
  // the cache slot
  size_t slot = 0;
  bool append = false;
  if (p.Kc && s_ok && (unsigned)pos < p.cap) {
    int pg = kv_page_id(p, (size_t)s, (unsigned)pos);
    pg = __builtin_amdgcn_readfirstlane(pg);
    append = kv_present(p, pg);
    if (append) slot = KV_OFFSET(p, pg, (unsigned)pos);
  }

  // this lane's item: its piece(s) and its c / s values
  const unsigned item = lane % p.items, hslot = lane / p.items;
  if (hslot >= p.hps) return;
  const bool rot = item < p.rot_items;
  unsigned colA, colB = 0;
  float c[NC], sn[NC];
  if constexpr (NEOX) {
    colA = rot ? item * 8u : p.rot + (item - p.rot_items) * 8u;
    colB = colA + p.half;  // (read only when rot)
  } else {
    colA = item * 8u;
  }
  if (rot) {
    const float* row = p.cs + (size_t)(unsigned)pos * p.ldcs + item * NC;
#pragma unroll
    for (unsigned q = 0; q < NC / 4; ++q) {
      const f4 cv = *reinterpret_cast<const f4*>(row + 4 * q), sv = *reinterpret_cast<const f4*>(row + p.half + 4 * q);
#pragma unroll
      for (unsigned e = 0; e < 4; ++e) {
        c[4 * q + e] = cv[e];
        sn[4 * q + e] = sv[e];
      }
    }
  } else {
#pragma unroll
    for (unsigned e = 0; e < NC; ++e) c[e] = sn[e] = 0.0f;
  }

  const unsigned nheads = p.q_heads + p.kv_heads + (append ? p.kv_heads : 0u);
  const unsigned h0 = BLOCK ? wave * p.hps + hslot : hslot, step = BLOCK ? 4u * p.hps : p.hps;
  // (two and four head steps in flight per lane were timed and are no faster in either form: DESIGN.md 4.21)
  for (unsigned h = h0; h < nheads; h += step) {
    const uint16_t* src;
    uint16_t *d1, *d2 = nullptr;
    bool rotate = rot;
    if (h < p.q_heads) {
      src = p.Q + (size_t)i * p.ldq + (size_t)h * p.hd;
      d1 = p.Qo + (size_t)i * p.ldqo + (size_t)h * p.hd;
    } else if (h < p.q_heads + p.kv_heads) {
      const unsigned g = h - p.q_heads;
      src = p.K + (size_t)i * p.ldk + (size_t)g * p.hd;
      d1 = p.Ko ? p.Ko + (size_t)i * p.ldko + (size_t)g * p.hd : nullptr;
      d2 = append ? p.Kc + slot + (size_t)g * p.hd : nullptr;
    } else {  // V: copied through the same pieces
      const unsigned g = h - p.q_heads - p.kv_heads;
      src = p.V + (size_t)i * p.ldv + (size_t)g * p.hd;
      d1 = p.Vc + slot + (size_t)g * p.hd;
      rotate = false;
    }
    // every load of the step, then the arithmetic, then the stores
    u4 a = *reinterpret_cast<const u4*>(src + colA), b = u4{0u, 0u, 0u, 0u};
    if constexpr (NEOX) {
      if (rot) b = *reinterpret_cast<const u4*>(src + colB);
    }
    if (rotate) {
      float xa[8], ya[8];
      unpack8<BF>(a, xa);
      if constexpr (NEOX) {
        float xb[8], yb[8];
        unpack8<BF>(b, xb);
#pragma unroll
        for (int e = 0; e < 8; ++e) ra_rot(xa[e], xb[e], c[e], sn[e], ya[e], yb[e]);
        b = pack8<BF>(yb);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) ra_rot(xa[2 * e], xa[2 * e + 1], c[e], sn[e], ya[2 * e], ya[2 * e + 1]);
      }
      a = pack8<BF>(ya);
    }
    if (d1) *reinterpret_cast<u4*>(d1 + colA) = a;
    if (d2) *reinterpret_cast<u4*>(d2 + colA) = a;
    if constexpr (NEOX) {
      if (rot) {
        if (d1) *reinterpret_cast<u4*>(d1 + colB) = b;
        if (d2) *reinterpret_cast<u4*>(d2 + colB) = b;
      }
    }
  }
}

template <bool BF, bool NEOX>
static int rope_append_launch(const RaArgs& a, int form, hipStream_t st) {
  static const char* const who = "sm_rope_append_{f16,bf16}";
  if (form == SM_ROPE_APPEND_FORM_BLOCK) return launch_grid<rope_append_kernel<BF, NEOX, true>>(a.tokens, 256, LDS_NO_OPTIN, 0, st, who, "rope_append_kernel", a);
  return launch_grid<rope_append_kernel<BF, NEOX, false>>(ceil_div(a.tokens, 4), 256, LDS_NO_OPTIN, 0, st, who, "rope_append_kernel", a);
}

template <bool BF>
static int rope_append(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc, void* Vc, const float* cs, const int* positions,
                       const int* token_seq, const int* seq_lens, const int* block_table, size_t tokens, size_t seqs, size_t q_heads, size_t kv_heads,
                       size_t head_dim, size_t rot_dim, size_t max_pos, size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldk, size_t ldv,
                       size_t ldqo, size_t ldko, size_t ldkv, size_t page_stride, size_t ldcs, size_t ldbt, int style, sm_stream_t stream) {
  static const char* const who = "sm_rope_append_{f16,bf16}";
  const bool cache = Kc != nullptr, table = rot_dim > 0;
  if (!Q || !K || !V || !Qo) {
    set_error("%s: invalid argument (null Q, K, V or Qo)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if ((Kc == nullptr) != (Vc == nullptr)) {
    set_error("%s: invalid argument (exactly one of Kc / Vc is null: the cache is both or neither)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!cache && !Ko) {
    set_error("%s: invalid argument (Kc and Ko are both null: the rotated K goes nowhere)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (cache && !block_table) {
    set_error("%s: invalid argument (null block_table with a cache)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!positions && !seq_lens) {
    set_error("%s: invalid argument (positions and seq_lens are both null)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (table && !cs) {
    set_error("%s: invalid argument (null cs with rot_dim > 0)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!ra_style_ok(style)) {
    set_error("%s: invalid argument (style is SM_ROPE_NEOX or SM_ROPE_INTERLEAVED)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  const size_t qw = mul_sat(q_heads, head_dim), kw = mul_sat(kv_heads, head_dim);
  if (ldq < qw || ldqo < qw || ldk < kw || ldv < kw || (Ko && ldko < kw) || (cache && !kv_pitches_ok(kw, page_size, max_pages, ldkv, page_stride, ldbt)) ||
      (table && ldcs < rot_dim)) {
    set_error("%s: invalid argument (a pitch below its extent: ldq, ldqo >= q_heads * head_dim; ldk, ldv, ldko, ldkv >= kv_heads * head_dim; page_stride >= "
              "page_size * ldkv; ldcs >= rot_dim; ldbt >= max_pages)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (rot_dim > head_dim) {
    set_error("%s: invalid argument (rot_dim exceeds head_dim)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!token_seq && tokens > seqs) {
    set_error("%s: invalid argument (null token_seq with tokens > seqs: token i is sequence i)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  {
    const void* ops[7] = {Q, K, V, Qo, Ko, Kc, Vc};  // (Q, Qo) and (K, Ko) may be one buffer at one pitch; no other two operands are
    bool bad = (Qo == Q && ldqo != ldq) || (Ko && Ko == K && ldko != ldk);
    for (int x = 0; x < 7; ++x)
      for (int y = x + 1; y < 7; ++y) bad = bad || (ops[x] && ops[x] == ops[y] && !(x == 0 && y == 3) && !(x == 1 && y == 4));
    if (bad) {
      set_error("%s: invalid argument (aliased operands: only Qo == Q and Ko == K, at equal pitches, are allowed)", who);
      return SM_STATUS_INVALID_VALUE;
    }
  }
  const size_t lim = KV_I32_MAX;
  if (tokens > lim || seqs > lim || q_heads > lim || kv_heads > lim || head_dim > lim || rot_dim > lim || (table && max_pos > lim) || ldq > lim || ldk > lim ||
      ldv > lim || ldqo > lim || (Ko && ldko > lim) || (table && ldcs > lim) || qw > lim || kw > lim ||
      (cache && !(kv_fields_fit(num_pages, page_size, max_pages, ldkv, page_stride, ldbt) && kv_context_fits(page_size, max_pages)))) {
    set_error("%s: a dimension, a pitch, q_heads * head_dim, kv_heads * head_dim or max_pages * page_size exceeds 2^31-1", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (head_dim % 8 != 0 || head_dim > SM_ROPE_APPEND_MAX_HEAD_DIM) {
    set_error("%s: head_dim is a multiple of 8, at most SM_ROPE_APPEND_MAX_HEAD_DIM (%d)", who, SM_ROPE_APPEND_MAX_HEAD_DIM);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (rot_dim % SM_ROPE_APPEND_ROT_DIM_MULTIPLE != 0) {
    set_error("%s: rot_dim is a multiple of SM_ROPE_APPEND_ROT_DIM_MULTIPLE (%d)", who, SM_ROPE_APPEND_ROT_DIM_MULTIPLE);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (cache && !kv_page_size_ok(page_size)) {
    set_error("%s: page_size is a power of two from SM_ATTN_DECODE_MIN_PAGE_SIZE (%d) to SM_ATTN_DECODE_MAX_PAGE_SIZE (%d)", who, SM_ATTN_DECODE_MIN_PAGE_SIZE,
              SM_ATTN_DECODE_MAX_PAGE_SIZE);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(Qo) || !aligned16(Ko) || !aligned16(Kc) || !aligned16(Vc) || ldq % 8 != 0 || ldk % 8 != 0 ||
      ldv % 8 != 0 || ldqo % 8 != 0 || (Ko && ldko % 8 != 0) || (cache && !kv_rows_aligned16(ldkv, page_stride))) {
    set_error("%s: needs 16-byte aligned rows of Q, K, V, Qo, Ko, Kc and Vc (pointer, ldq, ldk, ldv, ldqo, ldko, ldkv, page_stride %% 8 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (table && (!aligned16(cs) || ldcs % 4 != 0)) {
    set_error("%s: needs 16-byte aligned rows of cs (pointer, ldcs %% 4 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  const int form = rope_append_form(tokens, q_heads, kv_heads, head_dim, rot_dim);
  if (form == SM_ROPE_APPEND_FORM_EMPTY) return SM_STATUS_SUCCESS;
  RaArgs a = {};
  a.Q = (const uint16_t*)Q; a.K = (const uint16_t*)K; a.V = (const uint16_t*)V; a.Qo = (uint16_t*)Qo; a.Ko = (uint16_t*)Ko; a.Kc = (uint16_t*)Kc; a.Vc = (uint16_t*)Vc;
  a.cs = table ? cs : nullptr; a.pos = positions; a.tseq = token_seq; a.sl = seq_lens;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldqo = ldqo; a.ldko = ldko; a.ldcs = ldcs;
  a.tokens = (unsigned)tokens; a.seqs = (unsigned)seqs; a.q_heads = (unsigned)q_heads; a.kv_heads = (unsigned)kv_heads; a.hd = (unsigned)head_dim;
  a.rot = (unsigned)rot_dim; a.half = (unsigned)(rot_dim / 2);
  a.pos_end = table ? (unsigned)max_pos : 0x80000000u;  // without a table a token is padding only when pos < 0
  if (cache) paged_kv_fill(a, block_table, num_pages, page_size, max_pages, ldkv, page_stride, ldbt);
  const bool neox = style == SM_ROPE_NEOX;
  a.rot_items = (unsigned)(neox ? rot_dim / 16 : rot_dim / 8);
  a.items = (unsigned)(neox ? rot_dim / 16 + (head_dim - rot_dim) / 8 : head_dim / 8);  // 1 .. 32
  a.hps = 64u / a.items;
  hipStream_t st = (hipStream_t)stream;
  return neox ? rope_append_launch<BF, true>(a, form, st) : rope_append_launch<BF, false>(a, form, st);
}

}  // namespace sm

using namespace sm;

extern "C" int sm_rope_append_form(size_t tokens, size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim, int* form) {
  if (!form) {
    set_error("sm_rope_append_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = rope_append_form(tokens, q_heads, kv_heads, head_dim, rot_dim);
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_rope_append_f16(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc, void* Vc, const float* cs, const int* positions,
                                  const int* token_seq, const int* seq_lens, const int* block_table, size_t tokens, size_t seqs, size_t q_heads, size_t kv_heads,
                                  size_t head_dim, size_t rot_dim, size_t max_pos, size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldk,
                                  size_t ldv, size_t ldqo, size_t ldko, size_t ldkv, size_t page_stride, size_t ldcs, size_t ldbt, int style, sm_stream_t stream) {
  return rope_append<false>(Q, K, V, Qo, Ko, Kc, Vc, cs, positions, token_seq, seq_lens, block_table, tokens, seqs, q_heads, kv_heads, head_dim, rot_dim, max_pos,
                            num_pages, page_size, max_pages, ldq, ldk, ldv, ldqo, ldko, ldkv, page_stride, ldcs, ldbt, style, stream);
}
extern "C" int sm_rope_append_bf16(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc, void* Vc, const float* cs, const int* positions,
                                   const int* token_seq, const int* seq_lens, const int* block_table, size_t tokens, size_t seqs, size_t q_heads, size_t kv_heads,
                                   size_t head_dim, size_t rot_dim, size_t max_pos, size_t num_pages, size_t page_size, size_t max_pages, size_t ldq, size_t ldk,
                                   size_t ldv, size_t ldqo, size_t ldko, size_t ldkv, size_t page_stride, size_t ldcs, size_t ldbt, int style, sm_stream_t stream) {
  return rope_append<true>(Q, K, V, Qo, Ko, Kc, Vc, cs, positions, token_seq, seq_lens, block_table, tokens, seqs, q_heads, kv_heads, head_dim, rot_dim, max_pos,
                           num_pages, page_size, max_pages, ldq, ldk, ldv, ldqo, ldko, ldkv, page_stride, ldcs, ldbt, style, stream);
}
