// linear24_fp8.hip -- the 2:4 WEIGHT-sparse linear layer in the token-major layout on fp8 operands (sm_linear24_fp8, extension):
//     Y[tokens][out] = act( s(o,t) * (X[tokens][in] . W_2:4[out][in]^T) + beta * R + bias ),  s(o,t) = (alpha * w_scale[o]) * x_scale[t]
// W is the blob sm_compress24_fp8 / sm_quantize_compress24_fp8_* write (srcA of v_smfmac_f32_16x16x128_{fp8,bf8}_{fp8,bf8}, as in
// spmma_b8.h); X is what sm_quantize_rows_fp8_* writes and Y what the next layer reads: both stay as the caller holds them.  That is
// the instruction's own layout (spmma_b8.h, operand maps): B lane l wants, of token l & 15, dense k 16 G .. 16 G + 15 and
// 64 + 16 G .. + 15 (G = l >> 4) -- two 16-byte pieces of one X row; and the lane ends with four consecutive out features of one
// token -- one contiguous piece of Y's row, no LDS transpose.
//
// Two forms behind the one entry point (linear8_form(), below: the rule sm_linear24_fp8_form exports and sm_linear24_fp8 switches on):
//   tile    BM out features x BN tokens per workgroup, 128 dense k (two blob planes) per stage, brought in by global_load_lds into
//           a ring of NS stage buffers (counted vmcnt, one barrier per stage: the pipeline of linear24_tile_kernel).  K ascends, ONE
//           matrix instruction per 128-k stage into one accumulator, the odd last plane meets zeros: the accumulator of
//           spmma_b8_kernel bit for bit.  The metadata moves in 4-byte pieces: no evenness or alignment is asked of `out`.
//   decode  tokens <= LINEAR24_FP8_DECODE_MAX and out <= LINEAR24_FP8_DECODE_MAX_OUT: a pure weight stream.  One workgroup per 16
//           out features; its waves split the 128-k stages among themselves, stream the blob straight to registers and add their
//           fp32 partial tiles through LDS in wave order: deterministic, no workspace, no atomics.  Other K order than the tile
//           form: held to the arithmetic's bound.
#include "spmma_b8.h"
#include "spmma_args.h"

namespace sm {

// the largest `tokens` the decode form takes, and the largest `out` (the rule and what it rests on)
constexpr size_t LINEAR24_FP8_DECODE_MAX = 16;
constexpr size_t LINEAR24_FP8_DECODE_MAX_OUT = 16384;

struct Linear8Args {
  const char* vals;  // plane-major [in/64][out][32 B]
  const char* meta;  // plane-major [in/64][out][8 B]
  size_t Mtot;       // rows of the blob (= out)
  const uint8_t* X;
  void* Y;
  size_t ldx, ldy;   // elements
  int out, tokens, nplanes;  // nplanes = in / 64
  int tiles_m, tiles_n;
  int out_type;      // SM_OUT_*: the type of Y and R
  int packed;        // Y (and R, when read) take four-element pieces: aligned to four elements, out % 4 == 0, ldy % 4 == 0
  float alpha, beta;
  const float* w_scale;  // per out feature, or null
  const float* x_scale;  // per token, or null
  EpiArgs e;         // bias_dim in Y's coordinates (SM_BIAS_COL: per out feature); R has Y's shape, type and ldy (R = Y when none was given)
};

// The X image of a stage: [tokens][128 B], 16-byte chunk c of token row t at slot c ^ ((t >> 1) & 7).  A ds_read_b128 access group is
// 16 lanes of which 8 read chunk c of rows {0-3, 12-15} (+16i) and 8 read chunk c ^ 1 of rows {4-11}: with the row's parity choosing the
// half of the 256-byte bank line and (t >> 1) the slot, the 16 lanes cover 16 different 16-byte slots -- all 64 banks once.
__device__ __forceinline__ unsigned x8_swz(unsigned t) { return (t >> 1) & 7u; }

// four consecutive elements of the output type as one vector piece
template <int N> struct RawPiece { typedef u2 type; };
template <> struct RawPiece<4> { typedef u4 type; };
template <int OT>
struct OutPiece {
  typedef typename OutElt<OT>::T T;
  typedef typename RawPiece<sizeof(T)>::type raw_t;  // 8 bytes (fp16 / bf16) or 16 (fp32): one load / store
  T v[4];
};

// One fragment's epilogue and store: the lane holds out features o0 .. o0+3 of token t.  s * acc + beta * R written as store_c_f8
// writes s * a + beta * C, the bias as an addition of its own, the activation, one rounding.  R == Y is in place: the lane reads
// its piece before it writes it, and no other lane touches it.  sw[q] = alpha * w_scale[o0 + q] (alpha when there is none).
template <int OT>
__device__ __forceinline__ void linear8_store_frag(const Linear8Args& p, const f4 acc, unsigned o0, unsigned t, f4 sw, bool has_xs, float xs, bool bias_tok,
                                                   float bt, bool bias_out, f4 bo) {
  typedef typename OutElt<OT>::T T;
  if (t >= (unsigned)p.tokens || o0 >= (unsigned)p.out) return;
  T* dst = reinterpret_cast<T*>(p.Y) + (size_t)t * p.ldy + o0;
  const T* rs = reinterpret_cast<const T*>(p.e.R) + (size_t)t * p.ldy + o0;
  f4 v4;
  if (p.packed) {
    typedef typename OutPiece<OT>::raw_t raw_t;
    raw_t rraw = {};
    if (p.beta != 0.0f) rraw = *reinterpret_cast<const raw_t*>(rs);
    const OutPiece<OT> rv = __builtin_bit_cast(OutPiece<OT>, rraw);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float s = sw[q];
      if (has_xs) s = s * xs;
      float v = s * acc[q];
      if (p.beta != 0.0f) v += p.beta * OutElt<OT>::load(&rv.v[q]);
      v4[q] = v;
    }
    v4 = epi_act4(epi_bias4(v4, bias_tok, bt, bias_out, bo), p.e.act, p.e.act_arg);
    OutPiece<OT> o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o.v[q] = OutElt<OT>::conv(v4[q]);
    *reinterpret_cast<raw_t*>(dst) = __builtin_bit_cast(raw_t, o);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float s = sw[q];
      if (has_xs) s = s * xs;
      float v = s * acc[q];
      if (p.beta != 0.0f && o0 + q < (unsigned)p.out) v += p.beta * OutElt<OT>::load(rs + q);
      v4[q] = v;
    }
    v4 = epi_act4(epi_bias4(v4, bias_tok, bt, bias_out, bo), p.e.act, p.e.act_arg);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (o0 + q < (unsigned)p.out) dst[q] = OutElt<OT>::conv(v4[q]);
  }
}

__device__ __forceinline__ void linear8_store_frag_any(const Linear8Args& p, const f4 acc, unsigned o0, unsigned t, f4 sw, bool has_xs, float xs, bool bias_tok,
                                                       float bt, bool bias_out, f4 bo) {
  if (p.out_type == SM_OUT_F32) linear8_store_frag<SM_OUT_F32>(p, acc, o0, t, sw, has_xs, xs, bias_tok, bt, bias_out, bo);
  else if (p.out_type == SM_OUT_F16) linear8_store_frag<SM_OUT_F16>(p, acc, o0, t, sw, has_xs, xs, bias_tok, bt, bias_out, bo);
  else linear8_store_frag<SM_OUT_BF16>(p, acc, o0, t, sw, has_xs, xs, bias_tok, bt, bias_out, bo);
}

// the lane's four per-out-feature values of a vector (bias, w_scale); indices past the edge are clamped, not branched round (their
// outputs are never stored), so that the loads stay in flight under the K loop
__device__ __forceinline__ f4 linear8_per_out(const float* v, unsigned o0, unsigned out) {
  f4 b;
#pragma unroll
  for (int q = 0; q < 4; ++q) b[q] = v[o0 + q < out ? o0 + q : out - 1];
  return b;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Tile form.  Stage = 128 dense k = two planes: blob values [BM][64 B] (plane 0 | plane 1 per row, 16 rows per DMA instruction,
// a64_swz on the source), metadata [2][BM][8 B] (4-byte pieces, 32 rows of one plane per instruction: any row count), X
// [BN][128 B] (8 token rows per instruction, whole 128-byte lines, x8_swz on the source).  Rows / tokens past the edge are clamped to
// the last valid one: their products land in outputs that are never stored.  An odd plane count: the last stage's second plane
// (values, metadata) and X's k 64 .. 127 come from the zero page, as in spmma_b8_kernel.
// ---------------------------------------------------------------------------------------------------------------------------
template <class MM, int BM, int BN, int WM, int WN, int NS>
__global__ __launch_bounds__(64 * WM * WN) void linear24_fp8_tile_kernel(const Linear8Args p) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  static_assert(FM >= 1 && FN >= 1 && BM % 32 == 0 && BN % 8 == 0, "tile");
  static_assert(NS >= 2 && NS <= 4, "ring depth");
  constexpr int SA = BM * 64, SM_ = 2 * BM * 8, SX = BN * 128, STAGE = SA + SM_ + SX;
  constexpr int MB = BM / 32;  // metadata instructions per plane
  constexpr int A_N = BM / 16, M_N = 2 * MB, X_N = BN / 8, W = A_N + M_N + X_N;
  constexpr int SL = (W + NW - 1) / NW;  // DMA slots per wave
  constexpr int LPS = W / NW;            // least any wave issues per stage: the vmcnt unit
  static_assert(LPS >= 1, "every wave must issue at least one DMA per stage");
  static_assert((SA + SM_) % 128 == 0 && STAGE % 128 == 0, "the X image of every stage buffer is 128-byte aligned");
  extern __shared__ __attribute__((aligned(128))) char smem[];

  const unsigned tid = threadIdx.x, lane = tid & 63u, g = lane >> 4, r = lane & 15u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned wm = wave / WN, wn = wave % WN;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tile_m = lid / (unsigned)p.tiles_n, tile_n = lid - tile_m * (unsigned)p.tiles_n;
  // row and token indices are unsigned: an edge tile's origin plus its extent may pass 2^31 - 1 (never 2^32)
  const unsigned m0 = tile_m * BM, n0 = tile_n * BN;
  const unsigned mlast = (unsigned)p.out - 1u, tlast = (unsigned)p.tokens - 1u;

  // the lane's scales and bias values, fetched ahead of the K loop (plain loads, older than every DMA piece: the counted waits cover them)
  const bool bias_out = p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_COL, bias_tok = p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_ROW;
  const bool has_xs = p.x_scale != nullptr;
  f4 bo[FM], sw[FM];
  float bt[FN], xs[FN];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const unsigned o0 = m0 + (wm * TM + i * 16 + 4u * g);
    bo[i] = f4{0.f, 0.f, 0.f, 0.f};
    sw[i] = f4{p.alpha, p.alpha, p.alpha, p.alpha};
    if (bias_out) bo[i] = linear8_per_out(p.e.bias, o0, (unsigned)p.out);
    if (p.w_scale) sw[i] = p.alpha * linear8_per_out(p.w_scale, o0, (unsigned)p.out);
  }
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const unsigned t = n0 + (wn * TN + j * 16 + r), tc = t < tlast ? t : tlast;
    bt[j] = bias_tok ? p.e.bias[tc] : 0.f;
    xs[j] = has_xs ? p.x_scale[tc] : 1.f;
  }

  // per slot: source of stage 0, LDS offset, and whether the lane's piece belongs to the stage's second plane / half.  Slot i of
  // wave w is DMA instruction w + NW i of the stage; every kind's count is a multiple of NW, so a slot's kind (values, metadata,
  // X) is the same in every wave and known at compile time.
  static_assert(A_N % NW == 0 && M_N % NW == 0 && X_N % NW == 0 && SL * NW == W, "a slot is of one kind in every wave");
  const char* src[SL];
  unsigned loff[SL];
  bool second[SL];
#pragma unroll
  for (int i = 0; i < SL; ++i) {
    const unsigned t = wave + (unsigned)NW * i;
    if (NW * i < A_N) {  // 16 rows x 64 B of kept values: lane -> row 16 t + lane / 4, LDS chunk lane % 4
      const unsigned row = 16u * t + (lane >> 2), cs = (lane & 3u) ^ a64_swz(row);  // source chunk: plane cs >> 1, half cs & 1
      unsigned gr = m0 + row;
      gr = gr < mlast ? gr : mlast;
      src[i] = p.vals + ((size_t)(cs >> 1) * p.Mtot + (size_t)gr) * 32 + 16u * (cs & 1u);
      loff[i] = t * 1024u;
      second[i] = (cs >> 1) != 0;  // per lane
    } else if (NW * i < A_N + M_N) {  // 32 rows x 8 B of one plane's metadata: lane -> row lane / 2, half lane % 2
      const unsigned u = t - A_N, pl = u / MB, blk = u % MB;
      unsigned gr = m0 + (32u * blk + (lane >> 1));
      gr = gr < mlast ? gr : mlast;
      src[i] = p.meta + ((size_t)pl * p.Mtot + (size_t)gr) * 8 + 4u * (lane & 1u);
      loff[i] = SA + pl * (BM * 8) + blk * 256u;
      second[i] = pl != 0;
    } else {  // X: 8 token rows x 128 B (k-contiguous)
      const unsigned j = t - (A_N + M_N), row = 8u * j + (lane >> 3), cs = (lane & 7u) ^ x8_swz(row);
      unsigned gt = n0 + row;
      gt = gt < tlast ? gt : tlast;
      src[i] = reinterpret_cast<const char*>(p.X + (size_t)gt * p.ldx) + 16u * cs;
      loff[i] = SA + SM_ + j * 1024u;
      second[i] = cs >= 4u;  // k 64 .. 127 of the stage
    }
  }
  const int nkt = (p.nplanes + 1) / 2;
  const bool odd = (p.nplanes & 1) != 0;  // the last stage then has one plane: its second half meets zeros
  const size_t vstep = 2 * p.Mtot * 32, mstep = 2 * p.Mtot * 8;  // two planes per stage
  auto stage = [&](int kt, int buf) {
    char* base = smem + buf * STAGE;
    const bool tail = odd && kt == nkt - 1;
#pragma unroll
    for (int i = 0; i < SL; ++i) {
      const bool is_a = NW * i < A_N, is_m = !is_a && NW * i < A_N + M_N;
      const char* gsrc = src[i] + (size_t)kt * (is_a ? vstep : (is_m ? mstep : (size_t)128));
      // one-plane tail: the absent plane's values and metadata, and X's k 64 .. 127 (past the end of the row), come from a zero page
      if (tail && second[i]) gsrc = reinterpret_cast<const char*>(sm_zero_page_b8) + 16u * (lane & 7u);
      lptr_t* lp = (lptr_t*)(base + loff[i]);
      if (is_m) __builtin_amdgcn_global_load_lds((gptr_t*)gsrc, lp, 4, 0, 0);
      else __builtin_amdgcn_global_load_lds((gptr_t*)gsrc, lp, 16, 0, 0);
    }
  };

  f4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  // the ring of linear24_tile_kernel: wait for this wave's DMA of stage kt, barrier, refill the buffer read in iteration kt-1
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nkt) stage(s, s);
  int cur = 0, fill = NS - 1;
  for (int kt = 0; kt < nkt; ++kt) {
    const int ahead = (nkt - 1 - kt) < (NS - 2) ? (nkt - 1 - kt) : (NS - 2);
    if (NS >= 4 && ahead == 2) wait_dma_and_barrier<2 * LPS>();
    else if (NS >= 3 && ahead == 1) wait_dma_and_barrier<LPS>();
    else wait_dma_and_barrier<0>();
    if (kt + NS - 1 < nkt) stage(kt + NS - 1, fill);
    const char* As = smem + cur * STAGE;
    const char* Ms = As + SA;
    const char* Xs = Ms + SM_;
    i4v af[FM];
    int idx[FM];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const unsigned row = wm * TM + i * 16 + r;
      af[i] = *reinterpret_cast<const i4v*>(As + row * 64u + 16u * (g ^ a64_swz(row)));
      idx[i] = *reinterpret_cast<const int*>(Ms + (g >> 1) * (BM * 8) + row * 8u + 4u * (g & 1u));
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const unsigned t = wn * TN + j * 16 + r;
      const u4 lo = *reinterpret_cast<const u4*>(Xs + t * 128u + 16u * (g ^ x8_swz(t)));
      const u4 hi = *reinterpret_cast<const u4*>(Xs + t * 128u + 16u * ((4u + g) ^ x8_swz(t)));
      const i8v xf = i8v{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
#pragma unroll
      for (int i = 0; i < FM; ++i) acc[i][j] = MM::mma(af[i], xf, acc[i][j], idx[i]);
    }
    cur = cur + 1 == NS ? 0 : cur + 1;
    fill = fill + 1 == NS ? 0 : fill + 1;
  }

  // ---- store: no LDS, no barrier -- each lane's four out features are one piece of Y's row
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
      linear8_store_frag_any(p, acc[i][j], m0 + (wm * TM + i * 16 + 4u * g), n0 + (wn * TN + j * 16 + r), sw[i], has_xs, xs[j], bias_tok,
                             bt[j], bias_out, bo[i]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Decode form: tokens <= 16 FN.  Workgroup = 16 out features x NWV waves; wave w takes the 128-k stages w, w + NWV, ... (ascending),
// U of them requested before the first is multiplied.  Per stage a wave reads 2 x 512 B of values and 2 x 128 B of metadata, each
// contiguous (16 consecutive rows of one plane), non-temporal; X (<= 16 FN rows, shared by every workgroup) comes from L2.  Token
// columns at or beyond `tokens` are fed zeros; so are the second plane and X's k 64 .. 127 of an odd last stage.  The partial tiles
// meet in LDS and are added in wave order 0, 1, ..: the same bits on every run.
// ---------------------------------------------------------------------------------------------------------------------------
template <class MM, int FN, int NWV, int U>
__global__ __launch_bounds__(64 * NWV) void linear24_fp8_decode_kernel(const Linear8Args p) {
  static_assert(FN * 64 <= 64 * NWV, "one thread per output piece in the combine");
  __shared__ f4 part[NWV][FN][64];
  const unsigned tid = threadIdx.x, lane = tid & 63u, g = lane >> 4, r = lane & 15u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned m0 = blockIdx.x * 16u;
  unsigned row = m0 + r;
  row = row < (unsigned)p.out - 1u ? row : (unsigned)p.out - 1u;  // (clamped rows: computed, never stored)
  // the lane's 16 kept bytes and 4 metadata bytes of a stage: plane g >> 1, half g & 1 of its row
  const char* va = p.vals + ((size_t)(g >> 1) * p.Mtot + (size_t)row) * 32 + 16u * (g & 1u);
  const char* me = p.meta + ((size_t)(g >> 1) * p.Mtot + (size_t)row) * 8 + 4u * (g & 1u);
  const size_t vstep = 2 * p.Mtot * 32, mstep = 2 * p.Mtot * 8;
  const int nkt = (p.nplanes + 1) / 2;
  const bool odd = (p.nplanes & 1) != 0;
  const uint8_t* xr[FN];
  bool xv[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int t = 16 * j + (int)r;
    xv[j] = t < p.tokens;
    xr[j] = p.X + (size_t)(xv[j] ? t : 0) * p.ldx + 16u * g;
  }
  f4 acc[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};

  for (int s = (int)wave; s < nkt; s += NWV * U) {
    u4 a[U], x0[U][FN], x1[U][FN];
    int ix[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ss = s + u * NWV;  // wave-uniform
      const bool live = ss < nkt, tail = odd && ss == nkt - 1;
      a[u] = u4{0u, 0u, 0u, 0u};
      ix[u] = 0;
      if (live && !(tail && g >= 2u)) {
        a[u] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(va + (size_t)ss * vstep));
        ix[u] = __builtin_nontemporal_load(reinterpret_cast<const int*>(me + (size_t)ss * mstep));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        x0[u][j] = u4{0u, 0u, 0u, 0u};
        x1[u][j] = u4{0u, 0u, 0u, 0u};
        if (live && xv[j]) {
          x0[u][j] = *reinterpret_cast<const u4*>(xr[j] + (size_t)ss * 128);
          if (!tail) x1[u][j] = *reinterpret_cast<const u4*>(xr[j] + (size_t)ss * 128 + 64);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s + u * NWV < nkt) {
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const i8v xf = i8v{(int)x0[u][j][0], (int)x0[u][j][1], (int)x0[u][j][2], (int)x0[u][j][3],
                             (int)x1[u][j][0], (int)x1[u][j][1], (int)x1[u][j][2], (int)x1[u][j][3]};
          acc[j] = MM::mma(__builtin_bit_cast(i4v, a[u]), xf, acc[j], ix[u]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < FN; ++j) part[wave][j][lane] = acc[j];
  __syncthreads();
  if (tid < (unsigned)(FN * 64)) {  // wave j finishes fragment j: lane for lane the accumulator map
    const unsigned j = wave;
    f4 s = part[0][j][lane];
#pragma unroll
    for (int w = 1; w < NWV; ++w) s += part[w][j][lane];
    const unsigned o0 = m0 + 4u * g, t = 16u * j + r;
    const bool bias_out = p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_COL, bias_tok = p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_ROW;
    const bool has_xs = p.x_scale != nullptr, tv = t < (unsigned)p.tokens;
    f4 bo = {0.f, 0.f, 0.f, 0.f}, sw = {p.alpha, p.alpha, p.alpha, p.alpha};
    float bt = 0.f, xs = 1.f;
    if (bias_out) bo = linear8_per_out(p.e.bias, o0, (unsigned)p.out);
    if (p.w_scale) sw = p.alpha * linear8_per_out(p.w_scale, o0, (unsigned)p.out);
    if (bias_tok && tv) bt = p.e.bias[t];
    if (has_xs && tv) xs = p.x_scale[t];
    linear8_store_frag_any(p, s, o0, t, sw, has_xs, xs, bias_tok, bt, bias_out, bo);
  }
}

template <class MM, int BM, int BN, int WM, int WN, int NS>
static int launch_linear8_tile(const Linear8Args& a0, hipStream_t st) {
  Linear8Args a = a0;
  a.tiles_m = (a.out + BM - 1) / BM;
  a.tiles_n = (a.tokens + BN - 1) / BN;
  const size_t nwg = (size_t)a.tiles_m * a.tiles_n;
  if (nwg > 0x7fffffffu) {
    set_error("sm_linear24_fp8: grid too large");
    return SM_STATUS_NOT_SUPPORTED;
  }
  constexpr size_t lds = (size_t)NS * (BM * 80 + BN * 128);
  static LdsOptIn lds_optin;
  if (lds > 64 * 1024) {
    if (const int rc = ensure_dyn_lds(lds_optin, reinterpret_cast<const void*>(&linear24_fp8_tile_kernel<MM, BM, BN, WM, WN, NS>), lds, "linear24_fp8_tile_kernel")) return rc;
  }
  linear24_fp8_tile_kernel<MM, BM, BN, WM, WN, NS><<<dim3((unsigned)nwg), dim3(64 * WM * WN), lds, st>>>(a);
  return check_launch("linear24_fp8_tile_kernel");
}

template <class MM, int FN, int NWV, int U>
static int launch_linear8_decode(const Linear8Args& a, hipStream_t st) {
  linear24_fp8_decode_kernel<MM, FN, NWV, U><<<dim3((unsigned)ceil_div((size_t)a.out, 16)), dim3(64 * NWV), 0, st>>>(a);
  return check_launch("linear24_fp8_decode_kernel");
}

// The dispatch rule, stated once: sm_linear24_fp8 switches on it, sm_linear24_fp8_form exports it.  Tiles: the largest of
// 128 x 128, 128 x 64 and 64 x 64 that still gives every compute unit a workgroup (fewer, larger tiles re-read X and the blob less).
static int linear8_form(size_t tokens, size_t out, size_t in, size_t cus) {
  if (in % 64 != 0 || tokens > 0x7fffffffull || out > 0x7fffffffull || in > 0x7fffffffull) return SM_LINEAR24_FORM_NOT_TAKEN;
  if (tokens == 0 || out == 0) return SM_LINEAR24_FORM_EMPTY;
  if (tokens <= LINEAR24_FP8_DECODE_MAX && out <= LINEAR24_FP8_DECODE_MAX_OUT) return SM_LINEAR24_FORM_DECODE;
  const size_t t128 = ceil_div(out, 128) * ceil_div(tokens, 128), t64 = ceil_div(out, 128) * ceil_div(tokens, 64);
  if (tokens > 64 && t128 >= cus) return t128 > 0x7fffffffull ? SM_LINEAR24_FORM_NOT_TAKEN : SM_LINEAR24_FORM_TILE128;  // (the grid limit)
  if (t64 >= cus) return t64 > 0x7fffffffull ? SM_LINEAR24_FORM_NOT_TAKEN : SM_LINEAR24_FORM_TILE128x64;
  return ceil_div(out, 64) * ceil_div(tokens, 64) > 0x7fffffffull ? SM_LINEAR24_FORM_NOT_TAKEN : SM_LINEAR24_FORM_TILE64;
}

template <int FW, int FX>
static int linear8_launch(const Linear8Args& a, int form, hipStream_t st) {
  typedef MmaF8<FW, FX> MM;
  switch (form) {
    case SM_LINEAR24_FORM_DECODE: return launch_linear8_decode<MM, 1, 16, 4>(a, st);
    case SM_LINEAR24_FORM_TILE128: return launch_linear8_tile<MM, 128, 128, 2, 2, 3>(a, st);
    case SM_LINEAR24_FORM_TILE128x64: return launch_linear8_tile<MM, 128, 64, 4, 1, 3>(a, st);
    default: return launch_linear8_tile<MM, 64, 64, 2, 2, 3>(a, st);
  }
}

}  // namespace sm

using namespace sm;

extern "C" int sm_linear24_fp8_form(size_t tokens, size_t out_features, size_t in_features, size_t cus, int* form) {
  if (!form) {
    set_error("sm_linear24_fp8_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = linear8_form(tokens, out_features, in_features, cus ? cus : (size_t)device_cu_count());
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_linear24_fp8(const void* blob, const void* X, void* Y, size_t tokens, size_t out_features, size_t in_features, size_t ldx,
                               size_t ldy, int fmt_w, int fmt_x, int out_type, float alpha, float beta, const float* w_scale, const float* x_scale,
                               const sm_epilogue_t* epilogue, sm_stream_t stream) {
  const size_t out = out_features, in = in_features;
  Linear8Args a = {};
  bool plain;  // (not used: a plain epilogue takes the same kernels, whose bias / activation steps are skipped at run time)
  if (const int rc = epilogue_args(epilogue, Y, 0, out, beta, a.e, &plain, "sm_linear24_fp8")) return rc;
  (void)plain;
  const bool fmt_ok = (fmt_w == SM_FP8_E4M3 || fmt_w == SM_FP8_E5M2) && (fmt_x == SM_FP8_E4M3 || fmt_x == SM_FP8_E5M2);
  const bool out_ok = out_type == SM_OUT_F32 || out_type == SM_OUT_F16 || out_type == SM_OUT_BF16;
  if (!blob || !X || !Y || !aligned16(blob) || !fmt_ok || !out_ok || ldx < in || ldy < out) {
    set_error("sm_linear24_fp8: invalid argument (null operand, blob not 16-byte aligned, fmt not SM_FP8_*, out_type not SM_OUT_*, ldx < in_features or ldy < out_features)");
    return SM_STATUS_INVALID_VALUE;
  }
  if (tokens > 0x7fffffffull || out > 0x7fffffffull || in > 0x7fffffffull) {
    set_error("sm_linear24_fp8: dimension exceeds 2^31-1");
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (in % 64 != 0 || !aligned16(X) || ldx % 16 != 0) {
    set_error("sm_linear24_fp8: in_features %% 64 == 0 and 16-byte aligned rows of X (pointer, ldx %% 16) are required");
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (tokens == 0 || out == 0) return SM_STATUS_SUCCESS;
  const BlobLayout L = blob_layout(out, in, 1, 1);
  a.vals = (const char*)blob;
  a.meta = (const char*)blob + L.meta_off;
  a.Mtot = L.M;
  a.X = (const uint8_t*)X;
  a.Y = Y;
  a.ldx = ldx; a.ldy = ldy;
  a.out = (int)out; a.tokens = (int)tokens; a.nplanes = (int)(in / 64);
  a.out_type = out_type;
  a.alpha = alpha; a.beta = beta;
  a.w_scale = w_scale; a.x_scale = x_scale;
  const uintptr_t piece = out_type == SM_OUT_F32 ? 15u : 7u;  // four elements
  const bool r_ok = beta == 0.0f || (reinterpret_cast<uintptr_t>(a.e.R) & piece) == 0;
  a.packed = (out % 4 == 0 && ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(Y) & piece) == 0 && r_ok) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  const int form = linear8_form(tokens, out, in, (size_t)device_cu_count());
  if (form == SM_LINEAR24_FORM_NOT_TAKEN) {
    set_error("sm_linear24_fp8: grid too large");
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (fmt_w == SM_FP8_E4M3) return fmt_x == SM_FP8_E4M3 ? linear8_launch<SM_FP8_E4M3, SM_FP8_E4M3>(a, form, st) : linear8_launch<SM_FP8_E4M3, SM_FP8_E5M2>(a, form, st);
  return fmt_x == SM_FP8_E4M3 ? linear8_launch<SM_FP8_E5M2, SM_FP8_E4M3>(a, form, st) : linear8_launch<SM_FP8_E5M2, SM_FP8_E5M2>(a, form, st);
}
