// rope_append_kv8.hip -- sm_rope_append_kv8_{f16,bf16} (extension): sm_rope_append_* with the append going to the fp8 cache of paged_kv.h.
// Qo and Ko are bit for bit what rope_append.hip writes (the rotation is rope_common.h's); every K head, rotated and rounded to the 16-bit
// type, and every V head is then one row of the per-row fp8 rule of quant_fp8.h: its scale goes to Ksc / Vsc[page][head][slot], its bytes
// to the token's row of Kc8 / Vc8.
//
// The item ownership is rope_append_kernel's: a lane keeps its 16-byte piece or pieces of a head in registers, rotated.  The row's maximum
// is taken with mag_max8 over the lane's pieces and then over the head's L item lanes.  L is rot_dim / 16 + (head_dim - rot_dim) / 8 under
// SM_ROPE_NEOX, not a power of two when 0 < rot_dim < head_dim (6 at 64 / 32), so the xor ladder of row_reduce does not apply: head_max
// doubles a ROTATION instead -- after the steps 1, 2, 4, ... (each below L) lane i holds the maximum over items i .. i + 2^k - 1 (mod L) with
// 2^k >= L, every item of the head; a maximum does not mind the overlap.  The lanes of a head run every branch together (the head's kind,
// whether its row holds a non-finite element), so every exchange has its source lanes active.  Then quant4 and 8-byte stores; the lane of
// item 0 stores the scale.  Forms, threshold and the form query are sm_rope_append_*'s.  No LDS, no scratch, no barrier, no atomics.
#include "mma_tile.h"
#include "paged_kv.h"
#include "quant_fp8.h"
#include "rope_common.h"

namespace sm {

struct Ra8Args {
  const uint16_t *Q, *K, *V;
  uint16_t *Qo, *Ko;  // Ko: or null
  uint8_t *Kc, *Vc;
  float *Ksc, *Vsc;
  const float* cs;  // or null (rot == 0)
  const int *pos, *tseq, *sl, *bt;
  size_t ldq, ldk, ldv, ldqo, ldko, ldkv, page_stride, scale_page_stride, ldcs, ldbt;
  unsigned tokens, seqs, q_heads, kv_heads, hd, rot, half, pos_end, num_pages, page_size, page_shift, cap;  // bt .. cap: the PagedKv fields (paged_kv.h)
  unsigned items, rot_items, hps;  // items per head, how many of them rotate, heads per wave step (64 / items)
};

// maximum of both halves of m over the `items` lanes of a head, `first` the head's first lane, `item` this lane's place among them
__device__ __forceinline__ uint32_t head_max(uint32_t m, unsigned item, unsigned items, unsigned first) {
  m = (m & 0xffffu) > (m >> 16) ? (m & 0xffffu) : (m >> 16);
  for (unsigned off = 1; off < items; off <<= 1) {
    unsigned j = item + off;
    if (j >= items) j -= items;
    const uint32_t o = (uint32_t)__shfl((int)m, (int)(first + j));
    m = o > m ? o : m;
  }
  return m;
}

template <bool BF, int FMT, bool NEOX, bool BLOCK>
__global__ __launch_bounds__(256) void rope_append_kv8_kernel(const Ra8Args p) {
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
  // the cache slot: the token's row of bytes and its place in a head's scales
  size_t slot = 0, sslot = 0;
  bool append = false;
  if (s_ok && (unsigned)pos < p.cap) {
    int pg = kv_page_id(p, (size_t)s, (unsigned)pos);
    pg = __builtin_amdgcn_readfirstlane(pg);
    append = kv_present(p, pg);
    if (append) {
      slot = KV_OFFSET(p, pg, (unsigned)pos);
      sslot = KV8_SCALE_OFFSET(p, pg, 0u, (unsigned)pos);
    }
  }

  // this lane's item: its piece(s) and its c / s values
  const unsigned item = lane % p.items, hslot = lane / p.items;
  if (hslot >= p.hps) return;
  const unsigned first = lane - item;
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
  for (unsigned h = h0; h < nheads; h += step) {
    const uint16_t* src;
    uint16_t* d1 = nullptr;
    uint8_t* d8 = nullptr;  // the head's bytes in the cache; with it dsc, the head's scale
    float* dsc = nullptr;
    bool rotate = rot;
    if (h < p.q_heads) {
      src = p.Q + (size_t)i * p.ldq + (size_t)h * p.hd;
      d1 = p.Qo + (size_t)i * p.ldqo + (size_t)h * p.hd;
    } else if (h < p.q_heads + p.kv_heads) {
      const unsigned g = h - p.q_heads;
      src = p.K + (size_t)i * p.ldk + (size_t)g * p.hd;
      if (p.Ko) d1 = p.Ko + (size_t)i * p.ldko + (size_t)g * p.hd;
      if (append) {
        d8 = p.Kc + slot + (size_t)g * p.hd;
        dsc = p.Ksc + sslot + (size_t)g * p.page_size;
      }
    } else {  // V: quantised from its own bits (reached only when append)
      const unsigned g = h - p.q_heads - p.kv_heads;
      src = p.V + (size_t)i * p.ldv + (size_t)g * p.hd;
      d8 = p.Vc + slot + (size_t)g * p.hd;
      dsc = p.Vsc + sslot + (size_t)g * p.page_size;
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
    if (d1) {
      *reinterpret_cast<u4*>(d1 + colA) = a;
      if constexpr (NEOX) {
        if (rot) *reinterpret_cast<u4*>(d1 + colB) = b;
      }
    }
    if (d8) {  // (uniform over the head's lanes) the row a | b of every item lane is one row of the per-row rule
      uint32_t mx = mag_max8<BF, false>(0u, a);  // (b is zeros where the lane holds one piece)
      if constexpr (NEOX) mx = mag_max8<BF, false>(mx, b);
      mx = head_max(mx, item, p.items, first);
      const bool fix = mx >= Src16<BF>::inf;  // the row holds a NaN or an infinity: they do not enter amax
      if (fix) {
        uint32_t fin = mag_max8<BF, true>(0u, a);
        if constexpr (NEOX) fin = mag_max8<BF, true>(fin, b);
        mx = head_max(fin, item, p.items, first);
      }
      const float amax = __builtin_fmaxf(Src16<BF>::f32(mx), 0x1p-100f);
      const float scale = amax / F8Lim<FMT>::fmax, inv = F8Lim<FMT>::fmax / amax;
      if (item == 0) *dsc = scale;
      *reinterpret_cast<u2*>(d8 + colA) = u2{quant4<BF, FMT, false>(a[0], a[1], inv, fix), quant4<BF, FMT, false>(a[2], a[3], inv, fix)};
      if constexpr (NEOX) {
        if (rot) *reinterpret_cast<u2*>(d8 + colB) = u2{quant4<BF, FMT, false>(b[0], b[1], inv, fix), quant4<BF, FMT, false>(b[2], b[3], inv, fix)};
      }
    }
  }
}

template <bool BF, int FMT, bool NEOX>
static int rope_append_kv8_launch(const Ra8Args& a, int form, hipStream_t st) {
  static const char* const who = "sm_rope_append_kv8_{f16,bf16}";
  if (form == SM_ROPE_APPEND_FORM_BLOCK)
    return launch_grid<rope_append_kv8_kernel<BF, FMT, NEOX, true>>(a.tokens, 256, LDS_NO_OPTIN, 0, st, who, "rope_append_kv8_kernel", a);
  return launch_grid<rope_append_kv8_kernel<BF, FMT, NEOX, false>>(ceil_div(a.tokens, 4), 256, LDS_NO_OPTIN, 0, st, who, "rope_append_kv8_kernel", a);
}

template <bool BF>
static int rope_append_kv8(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc8, void* Vc8, float* Ksc, float* Vsc, const float* cs,
                           const int* positions, const int* token_seq, const int* seq_lens, const int* block_table, size_t tokens, size_t seqs, size_t q_heads,
                           size_t kv_heads, size_t head_dim, size_t rot_dim, size_t max_pos, size_t num_pages, size_t page_size, size_t max_pages, size_t ldq,
                           size_t ldk, size_t ldv, size_t ldqo, size_t ldko, size_t ldkv, size_t page_stride, size_t scale_page_stride, size_t ldcs, size_t ldbt,
                           int style, int fmt, sm_stream_t stream) {
  static const char* const who = "sm_rope_append_kv8_{f16,bf16}";
  const bool table = rot_dim > 0;
  if (!Q || !K || !V || !Qo || !Kc8 || !Vc8 || !Ksc || !Vsc) {
    set_error("%s: invalid argument (null Q, K, V, Qo, Kc8, Vc8, Ksc or Vsc: without an fp8 cache the call is sm_rope_append_*)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!block_table) {
    set_error("%s: invalid argument (null block_table)", who);
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
  if (ldq < qw || ldqo < qw || ldk < kw || ldv < kw || (Ko && ldko < kw) || !kv_pitches_ok(kw, page_size, max_pages, ldkv, page_stride, ldbt) ||
      (table && ldcs < rot_dim)) {
    set_error("%s: invalid argument (a pitch below its extent: ldq, ldqo >= q_heads * head_dim; ldk, ldv, ldko, ldkv >= kv_heads * head_dim; page_stride >= "
              "page_size * ldkv; ldcs >= rot_dim; ldbt >= max_pages)", who);
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
  if (rot_dim > head_dim) {
    set_error("%s: invalid argument (rot_dim exceeds head_dim)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  if (!token_seq && tokens > seqs) {
    set_error("%s: invalid argument (null token_seq with tokens > seqs: token i is sequence i)", who);
    return SM_STATUS_INVALID_VALUE;
  }
  {
    const void* ops[9] = {Q, K, V, Qo, Ko, Kc8, Vc8, Ksc, Vsc};  // (Q, Qo) and (K, Ko) may be one buffer at one pitch; no other two operands are
    bool bad = (Qo == Q && ldqo != ldq) || (Ko && Ko == K && ldko != ldk);
    for (int x = 0; x < 9; ++x)
      for (int y = x + 1; y < 9; ++y) bad = bad || (ops[x] && ops[x] == ops[y] && !(x == 0 && y == 3) && !(x == 1 && y == 4));
    if (bad) {
      set_error("%s: invalid argument (aliased operands: only Qo == Q and Ko == K, at equal pitches, are allowed)", who);
      return SM_STATUS_INVALID_VALUE;
    }
  }
  const size_t lim = KV_I32_MAX;
  if (tokens > lim || seqs > lim || q_heads > lim || kv_heads > lim || head_dim > lim || rot_dim > lim || (table && max_pos > lim) || ldq > lim || ldk > lim ||
      ldv > lim || ldqo > lim || (Ko && ldko > lim) || (table && ldcs > lim) || qw > lim || kw > lim || scale_page_stride > lim ||
      !(kv_fields_fit(num_pages, page_size, max_pages, ldkv, page_stride, ldbt) && kv_context_fits(page_size, max_pages))) {
    set_error("%s: a dimension, a pitch, q_heads * head_dim, kv_heads * head_dim or max_pages * page_size exceeds 2^31-1", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (head_dim != SM_ATTN_DECODE_MIN_HEAD_DIM && head_dim != SM_ATTN_DECODE_MAX_HEAD_DIM) {
    set_error("%s: head_dim is SM_ATTN_DECODE_MIN_HEAD_DIM (%d) or SM_ATTN_DECODE_MAX_HEAD_DIM (%d): what sm_attn_decode_kv8_* reads", who,
              SM_ATTN_DECODE_MIN_HEAD_DIM, SM_ATTN_DECODE_MAX_HEAD_DIM);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (rot_dim % SM_ROPE_APPEND_ROT_DIM_MULTIPLE != 0) {
    set_error("%s: rot_dim is a multiple of SM_ROPE_APPEND_ROT_DIM_MULTIPLE (%d)", who, SM_ROPE_APPEND_ROT_DIM_MULTIPLE);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!kv_page_size_ok(page_size)) {
    set_error("%s: page_size is a power of two from SM_ATTN_DECODE_MIN_PAGE_SIZE (%d) to SM_ATTN_DECODE_MAX_PAGE_SIZE (%d)", who, SM_ATTN_DECODE_MIN_PAGE_SIZE,
              SM_ATTN_DECODE_MAX_PAGE_SIZE);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(Qo) || !aligned16(Ko) || ldq % 8 != 0 || ldk % 8 != 0 || ldv % 8 != 0 || ldqo % 8 != 0 ||
      (Ko && ldko % 8 != 0)) {
    set_error("%s: needs 16-byte aligned rows of Q, K, V, Qo and Ko (pointer, ldq, ldk, ldv, ldqo, ldko %% 8 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (!aligned16(Kc8) || !aligned16(Vc8) || !kv8_rows_aligned16(ldkv, page_stride) || !aligned16(Ksc) || !aligned16(Vsc) ||
      !kv8_scale_rows_aligned16(scale_page_stride)) {
    set_error("%s: needs 16-byte aligned rows of Kc8 and Vc8 (pointer, ldkv, page_stride %% 16 == 0) and of Ksc and Vsc (pointer, scale_page_stride %% 4 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (table && (!aligned16(cs) || ldcs % 4 != 0)) {
    set_error("%s: needs 16-byte aligned rows of cs (pointer, ldcs %% 4 == 0)", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  int form = SM_ROPE_APPEND_FORM_INVALID;
  sm_rope_append_form(tokens, q_heads, kv_heads, head_dim, rot_dim, &form);  // the 16-bit call's rule and threshold
  if (form == SM_ROPE_APPEND_FORM_EMPTY) return SM_STATUS_SUCCESS;
  Ra8Args a = {};
  a.Q = (const uint16_t*)Q; a.K = (const uint16_t*)K; a.V = (const uint16_t*)V; a.Qo = (uint16_t*)Qo; a.Ko = (uint16_t*)Ko;
  a.Kc = (uint8_t*)Kc8; a.Vc = (uint8_t*)Vc8; a.Ksc = Ksc; a.Vsc = Vsc;
  a.cs = table ? cs : nullptr; a.pos = positions; a.tseq = token_seq; a.sl = seq_lens;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldqo = ldqo; a.ldko = ldko; a.ldcs = ldcs; a.scale_page_stride = scale_page_stride;
  a.tokens = (unsigned)tokens; a.seqs = (unsigned)seqs; a.q_heads = (unsigned)q_heads; a.kv_heads = (unsigned)kv_heads; a.hd = (unsigned)head_dim;
  a.rot = (unsigned)rot_dim; a.half = (unsigned)(rot_dim / 2);
  a.pos_end = table ? (unsigned)max_pos : 0x80000000u;  // without a table a token is padding only when pos < 0
  paged_kv_fill(a, block_table, num_pages, page_size, max_pages, ldkv, page_stride, ldbt);
  const bool neox = style == SM_ROPE_NEOX;
  a.rot_items = (unsigned)(neox ? rot_dim / 16 : rot_dim / 8);
  a.items = (unsigned)(neox ? rot_dim / 16 + (head_dim - rot_dim) / 8 : head_dim / 8);  // 4 .. 16
  a.hps = 64u / a.items;
  hipStream_t st = (hipStream_t)stream;
  if (fmt == SM_FP8_E4M3) return neox ? rope_append_kv8_launch<BF, SM_FP8_E4M3, true>(a, form, st) : rope_append_kv8_launch<BF, SM_FP8_E4M3, false>(a, form, st);
  return neox ? rope_append_kv8_launch<BF, SM_FP8_E5M2, true>(a, form, st) : rope_append_kv8_launch<BF, SM_FP8_E5M2, false>(a, form, st);
}

}  // namespace sm

using namespace sm;

extern "C" int sm_rope_append_kv8_f16(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc8, void* Vc8, float* Ksc, float* Vsc, const float* cs,
                                      const int* positions, const int* token_seq, const int* seq_lens, const int* block_table, size_t tokens, size_t seqs,
                                      size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim, size_t max_pos, size_t num_pages, size_t page_size,
                                      size_t max_pages, size_t ldq, size_t ldk, size_t ldv, size_t ldqo, size_t ldko, size_t ldkv, size_t page_stride,
                                      size_t scale_page_stride, size_t ldcs, size_t ldbt, int style, int fmt, sm_stream_t stream) {
  return rope_append_kv8<false>(Q, K, V, Qo, Ko, Kc8, Vc8, Ksc, Vsc, cs, positions, token_seq, seq_lens, block_table, tokens, seqs, q_heads, kv_heads, head_dim, rot_dim,
                                max_pos, num_pages, page_size, max_pages, ldq, ldk, ldv, ldqo, ldko, ldkv, page_stride, scale_page_stride, ldcs, ldbt, style, fmt, stream);
}
extern "C" int sm_rope_append_kv8_bf16(const void* Q, const void* K, const void* V, void* Qo, void* Ko, void* Kc8, void* Vc8, float* Ksc, float* Vsc, const float* cs,
                                       const int* positions, const int* token_seq, const int* seq_lens, const int* block_table, size_t tokens, size_t seqs,
                                       size_t q_heads, size_t kv_heads, size_t head_dim, size_t rot_dim, size_t max_pos, size_t num_pages, size_t page_size,
                                       size_t max_pages, size_t ldq, size_t ldk, size_t ldv, size_t ldqo, size_t ldko, size_t ldkv, size_t page_stride,
                                       size_t scale_page_stride, size_t ldcs, size_t ldbt, int style, int fmt, sm_stream_t stream) {
  return rope_append_kv8<true>(Q, K, V, Qo, Ko, Kc8, Vc8, Ksc, Vsc, cs, positions, token_seq, seq_lens, block_table, tokens, seqs, q_heads, kv_heads, head_dim, rot_dim,
                               max_pos, num_pages, page_size, max_pages, ldq, ldk, ldv, ldqo, ldko, ldkv, page_stride, scale_page_stride, ldcs, ldbt, style, fmt, stream);
}
