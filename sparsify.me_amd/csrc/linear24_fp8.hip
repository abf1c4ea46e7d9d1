// linear24_fp8.hip -- the 2:4 WEIGHT-sparse linear layer in the token-major layout on fp8 operands (sm_linear24_fp8, extension):
//     Y[tokens][out] = act( s(o,t) * (X[tokens][in] . W_2:4[out][in]^T) + beta * R + bias ),  s(o,t) = (alpha * w_scale[o]) * x_scale[t]
// W is the blob sm_compress24_fp8 / sm_quantize_compress24_fp8_* write (srcA of v_smfmac_f32_16x16x128_{fp8,bf8}_{fp8,bf8}, as in
// spmma_b8.h); X is what sm_quantize_rows_fp8_* writes and Y what the next layer reads: both stay as the caller holds them.  That is
// the instruction's own layout (spmma_b8.h, operand maps): B lane l wants, of token l & 15, dense k 16 G .. 16 G + 15 and
// 64 + 16 G .. + 15 (G = l >> 4) -- two 16-byte pieces of one X row; and the lane ends with four consecutive out features of one
// token -- one contiguous piece of Y's row, no LDS transpose.
//
// The operand-independent core (rule, argument checks, epilogue and store, decode combine, tile launcher) is linear24_common.h,
// shared with linear24_f16.hip.  Two forms behind the one entry point (linear24_form(): the rule sm_linear24_fp8_form exports and
// sm_linear24_fp8 switches on, asked with the device's compute-unit count):
//   tile    BM out features x BN tokens per workgroup, 128 dense k (two blob planes) per stage, brought in by global_load_lds into
//           a ring of NS stage buffers (counted vmcnt, one barrier per stage: the pipeline of linear24_tile_kernel).  K ascends, ONE
//           matrix instruction per 128-k stage into one accumulator, the odd last plane meets zeros: the accumulator of
//           spmma_b8_kernel bit for bit.  The metadata moves in 4-byte pieces: no evenness or alignment is asked of `out`.
//   decode  tokens <= LINEAR24_DECODE_MAX and out <= LINEAR24_DECODE_MAX_OUT: a pure weight stream.  One workgroup per 16
//           out features; its waves split the 128-k stages among themselves, stream the blob straight to registers and add their
//           fp32 partial tiles through LDS in wave order: deterministic, no workspace, no atomics.  Other K order than the tile
//           form: held to the arithmetic's bound.
// The gated layer (sm_linear24_glu_fp8: Y = act(gate) * up of a fused gate/up weight) is the GLU instantiation of the same two
// kernels: only the blob rows a fragment is fetched from (linear24_glu_row) and the store (linear24_store_glu) differ.
// Below the kernels: one host template, linear8<GLU, GROUPED, GATHER>, behind all six launching entry points of this file, with the
// one format switch; linear8_launch<FW, FX, ...> is the one form switch.
#include "spmma_b8.h"
#include "linear24_common.h"

namespace sm {

// the entry points' names in their messages: [GLU][plain, grouped, gathered]
static const char* const LINEAR24_8_WHO[2][3] = {{"sm_linear24_fp8", "sm_linear24_grouped_fp8", "sm_linear24_grouped_gather_fp8"},
                                                 {"sm_linear24_glu_fp8", "sm_linear24_grouped_glu_fp8", "sm_linear24_grouped_glu_gather_fp8"}};

struct Linear8Args : Linear24Core {  // vals plane-major [in/64][out][32 B]
  size_t Mtot;  // rows of the blob (= out; the gated kernels: 2 * out)
  const uint8_t* X;
  int nplanes;   // in / 64
  int out_type;  // SM_OUT_*: the type of Y and R
};

// an element of the output type as the shared store sees it: OutElt<OT> + the raw piece of four, 8 bytes (fp16 / bf16) or 16 (fp32)
template <int N> struct RawPiece { typedef u2 type; };
template <> struct RawPiece<4> { typedef u4 type; };
template <int OT>
struct EltOut : OutElt<OT> {
  typedef typename RawPiece<sizeof(typename OutElt<OT>::T)>::type raw_t;
};

// the shared store (s = sw[q] * xs) under the runtime switch over the output type
__device__ __forceinline__ void linear8_store_frag_any(const Linear8Args& p, const f4 acc, unsigned o0, unsigned t, f4 sw, float xs, float bt, f4 bo) {
  if (p.out_type == SM_OUT_F32) linear24_store_frag<EltOut<SM_OUT_F32>, true>(p, acc, o0, t, sw, xs, bt, bo);
  else if (p.out_type == SM_OUT_F16) linear24_store_frag<EltOut<SM_OUT_F16>, true>(p, acc, o0, t, sw, xs, bt, bo);
  else linear24_store_frag<EltOut<SM_OUT_BF16>, true>(p, acc, o0, t, sw, xs, bt, bo);
}

// ... and the gated store under the same switch
__device__ __forceinline__ void linear8_store_glu_any(const Linear8Args& p, const f4 accg, const f4 accu, unsigned h0, unsigned t, f4 swg, f4 swu, float xs,
                                                      f4 bg, f4 bu) {
  if (p.out_type == SM_OUT_F32) linear24_store_glu<EltOut<SM_OUT_F32>, true>(p, accg, accu, h0, t, swg, swu, xs, bg, bu);
  else if (p.out_type == SM_OUT_F16) linear24_store_glu<EltOut<SM_OUT_F16>, true>(p, accg, accu, h0, t, swg, swu, xs, bg, bu);
  else linear24_store_glu<EltOut<SM_OUT_BF16>, true>(p, accg, accu, h0, t, swg, swu, xs, bg, bu);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Tile form.  Stage = 128 dense k = two planes: blob values [BM][64 B] (plane 0 | plane 1 per row, 16 rows per DMA instruction,
// a64_swz on the source), metadata [2][BM][8 B] (4-byte pieces, 32 rows of one plane per instruction: any row count), X
// [BN][128 B] (8 token rows per instruction, whole 128-byte lines, x_swz on the source).  Rows / tokens past the edge are clamped to
// the last valid one: their products land in outputs that are never stored.  An odd plane count: the last stage's second plane
// (values, metadata) and X's k 64 .. 127 come from the zero page, as in spmma_b8_kernel.
// ---------------------------------------------------------------------------------------------------------------------------
// GLU: the tile's BM rows are BM / 2 gate rows and the BM / 2 up rows of the same hidden features, interleaved by 16-row fragment; p.out
// is `hidden`, the width of Y, and the blob has p.Mtot = 2 * p.out rows.
// GROUPED (sm_linear24_grouped_*fp8): as in linear24_tile_kernel -- slots for tiles_n (the grid's bound), linear24_group_view, then this body on expert
// g's own rows of the stacked blob (p.Mtot = groups * rows of one expert: the plane stride).
// GATHER (sm_linear24_grouped_*gather_fp8, GROUPED only): as in linear24_tile_kernel, the X rows are those x_index names; x_scale is read
// at the same source row (the scale belongs to the token that was quantised), a per-token bias stays in Y's sorted rows.
template <class MM, int BM, int BN, int WM, int WN, int NS, bool GLU = false, bool GROUPED = false, bool GATHER = false>
__global__ __launch_bounds__(64 * WM * WN) void linear24_fp8_tile_kernel(const typename Linear24ArgsSel<Linear8Args, GROUPED>::type pk) {
  typename Linear24ArgsSel<Linear8Args, GROUPED>::view_t p = pk;
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  static_assert(FM >= 1 && FN >= 1 && BM % 32 == 0 && BN % 8 == 0, "tile");
  static_assert(!GLU || FM % 2 == 0, "a wave of a gated tile holds whole (gate, up) fragment pairs");
  static_assert(NS >= 2 && NS <= 4, "ring depth");
  static_assert(GROUPED || !GATHER, "the gathered layers are grouped layers");
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
  const unsigned tm = lid / (unsigned)p.tiles_n, tile_n = lid - tm * (unsigned)p.tiles_n;  // (a grouped workgroup's come from its view)
  // row and token indices are unsigned: an edge tile's origin plus its extent may pass 2^31 - 1 (never 2^32)
  unsigned tile_m = tm, n0 = tile_n * BN;
  if constexpr (GROUPED) {
    if (!linear24_group_view<BN>(p, pk.group_offsets, pk.groups, blockIdx.x, (GLU ? 2u : 1u) * (unsigned)p.out, 32u, tile_m, n0)) return;  // (workgroup-uniform)
  }
  const unsigned m0 = tile_m * BM;
  const unsigned mlast = (unsigned)p.out - 1u, tlast = (unsigned)p.tokens - 1u;
  const unsigned hid0 = tile_m * (BM / 2);  // GLU: the tile's first hidden feature

  // the lane's scales and bias values, fetched ahead of the K loop (plain loads, older than every DMA piece: the counted waits cover them)
  const bool bias_out = p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_COL, bias_tok = p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_ROW;
  const bool has_xs = p.x_scale != nullptr;
  f4 bo[FM], sw[FM];
  float bt[FN], xs[FN];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    // (GLU: fragment i is the gate (i even) or up (i odd) rows of hidden features o0 ..; the vectors hold gate's values, then up's)
    const unsigned o0 = GLU ? hid0 + (wm * (TM / 2) + (i / 2) * 16 + 4u * g) : m0 + (wm * TM + i * 16 + 4u * g);
    const unsigned up = GLU && (i & 1) ? (unsigned)p.out : 0u;
    bo[i] = f4{0.f, 0.f, 0.f, 0.f};
    sw[i] = f4{p.alpha, p.alpha, p.alpha, p.alpha};
    if (bias_out) bo[i] = linear24_per_out(p.e.bias + up, o0, (unsigned)p.out);
    if (p.w_scale) sw[i] = p.alpha * linear24_per_out(p.w_scale + up, o0, (unsigned)p.out);
  }
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const unsigned t = n0 + (wn * TN + j * 16 + r), tc = t < tlast ? t : tlast;
    bt[j] = bias_tok ? p.e.bias[tc] : 0.f;
    if constexpr (GATHER) xs[j] = has_xs ? p.x_scale[linear24_gather_row(pk.x_index, pk.x_rows, tc)] : 1.f;
    else xs[j] = has_xs ? p.x_scale[tc] : 1.f;
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
      if constexpr (GLU) gr = linear24_glu_row(hid0, row, (unsigned)p.out);
      src[i] = p.vals + ((size_t)(cs >> 1) * p.Mtot + (size_t)gr) * 32 + 16u * (cs & 1u);
      loff[i] = t * 1024u;
      second[i] = (cs >> 1) != 0;  // per lane
    } else if (NW * i < A_N + M_N) {  // 32 rows x 8 B of one plane's metadata: lane -> row lane / 2, half lane % 2
      const unsigned u = t - A_N, pl = u / MB, blk = u % MB;
      unsigned gr = m0 + (32u * blk + (lane >> 1));
      gr = gr < mlast ? gr : mlast;
      if constexpr (GLU) gr = linear24_glu_row(hid0, 32u * blk + (lane >> 1), (unsigned)p.out);  // (per lane half: a gate and an up fragment)
      src[i] = p.meta + ((size_t)pl * p.Mtot + (size_t)gr) * 8 + 4u * (lane & 1u);
      loff[i] = SA + pl * (BM * 8) + blk * 256u;
      second[i] = pl != 0;
    } else {  // X: 8 token rows x 128 B (k-contiguous)
      const unsigned j = t - (A_N + M_N), row = 8u * j + (lane >> 3), cs = (lane & 7u) ^ x_swz(row);
      unsigned gt = n0 + row;
      gt = gt < tlast ? gt : tlast;
      if constexpr (GATHER) gt = linear24_gather_row(pk.x_index, pk.x_rows, gt);
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
      const u4 lo = *reinterpret_cast<const u4*>(Xs + t * 128u + 16u * (g ^ x_swz(t)));
      const u4 hi = *reinterpret_cast<const u4*>(Xs + t * 128u + 16u * ((4u + g) ^ x_swz(t)));
      const i8v xf = i8v{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
#pragma unroll
      for (int i = 0; i < FM; ++i) acc[i][j] = MM::mma(af[i], xf, acc[i][j], idx[i]);
    }
    cur = cur + 1 == NS ? 0 : cur + 1;
    fill = fill + 1 == NS ? 0 : fill + 1;
  }

  // ---- store: no LDS, no barrier -- each lane's four out features are one piece of Y's row
  if constexpr (GLU) {
#pragma unroll
    for (int i = 0; i < FM; i += 2)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        linear8_store_glu_any(p, acc[i][j], acc[i + 1][j], hid0 + (wm * (TM / 2) + (i / 2) * 16 + 4u * g), n0 + (wn * TN + j * 16 + r), sw[i], sw[i + 1],
                              xs[j], bo[i], bo[i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        linear8_store_frag_any(p, acc[i][j], m0 + (wm * TM + i * 16 + 4u * g), n0 + (wn * TN + j * 16 + r), sw[i], xs[j], bt[j], bo[i]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Decode form: tokens <= 16 FN.  Workgroup = 16 out features x NWV waves; wave w takes the 128-k stages w, w + NWV, ... (ascending),
// U of them requested before the first is multiplied.  Per stage a wave reads 2 x 512 B of values and 2 x 128 B of metadata, each
// contiguous (16 consecutive rows of one plane), non-temporal; X (<= 16 FN rows, shared by every workgroup) comes from L2.  Token
// columns at or beyond `tokens` are fed zeros; so are the second plane and X's k 64 .. 127 of an odd last stage.  The partial tiles
// meet in LDS and are added in wave order 0, 1, ..: the same bits on every run.
// ---------------------------------------------------------------------------------------------------------------------------
// GLU: one workgroup per 16 hidden features; a wave streams the gate fragment and the up fragment of its stage (NF = 2 value and
// metadata loads) against the same X registers, K split and combine order unchanged: g and u have this kernel's plain bits.
template <class MM, int FN, int NWV, int U, bool GLU = false>
__global__ __launch_bounds__(64 * NWV) void linear24_fp8_decode_kernel(const Linear8Args p) {
  static_assert(!GLU || FN == 1, "the gated decode form holds one token fragment");
  constexpr int NF = GLU ? 2 : 1;  // blob fragments per stage
  const unsigned tid = threadIdx.x, lane = tid & 63u, g = lane >> 4, r = lane & 15u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned m0 = blockIdx.x * 16u;
  unsigned row = m0 + r;
  row = row < (unsigned)p.out - 1u ? row : (unsigned)p.out - 1u;  // (clamped rows: computed, never stored)
  // the lane's 16 kept bytes and 4 metadata bytes of a stage: plane g >> 1, half g & 1 of its row
  const char* va = p.vals + ((size_t)(g >> 1) * p.Mtot + (size_t)row) * 32 + 16u * (g & 1u);
  const char* me = p.meta + ((size_t)(g >> 1) * p.Mtot + (size_t)row) * 8 + 4u * (g & 1u);
  const size_t vstep = 2 * p.Mtot * 32, mstep = 2 * p.Mtot * 8;
  const size_t vup = GLU ? (size_t)p.out * 32 : 0, mup = GLU ? (size_t)p.out * 8 : 0;  // from a gate row to its up row
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
  f4 acc[NF * FN];  // GLU: {gate, up}
#pragma unroll
  for (int j = 0; j < NF * FN; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};

  for (int s = (int)wave; s < nkt; s += NWV * U) {
    u4 a[U][NF], x0[U][FN], x1[U][FN];
    int ix[U][NF];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ss = s + u * NWV;  // wave-uniform
      const bool live = ss < nkt, tail = odd && ss == nkt - 1;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        a[u][f] = u4{0u, 0u, 0u, 0u};
        ix[u][f] = 0;
        if (live && !(tail && g >= 2u)) {
          a[u][f] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(va + (size_t)ss * vstep + f * vup));
          ix[u][f] = __builtin_nontemporal_load(reinterpret_cast<const int*>(me + (size_t)ss * mstep + f * mup));
        }
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
#pragma unroll
          for (int f = 0; f < NF; ++f) acc[j * NF + f] = MM::mma(__builtin_bit_cast(i4v, a[u][f]), xf, acc[j * NF + f], ix[u][f]);
        }
      }
    }
  }
  if constexpr (GLU) linear24_decode_tail_glu<Linear8Args, linear8_store_glu_any, true, NWV>(p, acc, m0);
  else linear24_decode_tail<Linear8Args, linear8_store_frag_any, true, FN, NWV>(p, acc, m0);
}

template <class MM, int BM, int BN, int WM, int WN, int NS, bool GLU, bool GROUPED, bool GATHER>
static int launch_linear8_tile(const Linear8Args& a, const Linear24Groups& grp, hipStream_t st, const char* who) {
  return launch_linear24_tile<Linear8Args, GROUPED, linear24_fp8_tile_kernel<MM, BM, BN, WM, WN, NS, GLU, GROUPED, GATHER>, GLU ? BM / 2 : BM, BN, 64 * WM * WN,
                              (size_t)NS * (BM * 80 + BN * 128)>(a, grp, st, who, "linear24_fp8_tile_kernel");
}

// the form switch, per operand format pair (no grouped decode kernel: the grouped rule never answers DECODE)
template <int FW, int FX, bool GLU, bool GROUPED, bool GATHER>
static int linear8_launch(const Linear8Args& a, const Linear24Groups& grp, int form, hipStream_t st, const char* who) {
  typedef MmaF8<FW, FX> MM;
  if constexpr (!GROUPED)
    if (form == SM_LINEAR24_FORM_DECODE)
      return launch_linear24_decode<Linear8Args, linear24_fp8_decode_kernel<MM, 1, 16, 4, GLU>, 64 * 16>(a, st, "linear24_fp8_decode_kernel");
  switch (form) {
    case SM_LINEAR24_FORM_TILE128: return launch_linear8_tile<MM, 128, 128, 2, 2, 3, GLU, GROUPED, GATHER>(a, grp, st, who);
    case SM_LINEAR24_FORM_TILE128x64: return launch_linear8_tile<MM, 128, 64, 4, 1, 3, GLU, GROUPED, GATHER>(a, grp, st, who);
    default: return launch_linear8_tile<MM, 64, 64, 2, 2, 3, GLU, GROUPED, GATHER>(a, grp, st, who);
  }
}

// Every launching entry point of this file: the checks, the rule (asked with the device's compute-unit count), the format switch.
// GLU: `out` is `hidden` and t holds act / bias; GROUPED: grp is read; GATHER (GROUPED only): X through grp.x_index.
template <bool GLU, bool GROUPED, bool GATHER>
static int linear8(const void* blob, const void* X, void* Y, const Linear24Groups& grp, size_t tokens, size_t out, size_t in, size_t ldx, size_t ldy,
                   int fmt_w, int fmt_x, int out_type, const Linear24Tail& t, const float* w_scale, const float* x_scale, sm_stream_t stream) {
  static_assert(GROUPED || !GATHER, "only a grouped layer gathers");
  const char* who = LINEAR24_8_WHO[GLU][GROUPED + GATHER];
  Linear8Args a = {};
  const bool fmt_ok = (fmt_w == SM_FP8_E4M3 || fmt_w == SM_FP8_E5M2) && (fmt_x == SM_FP8_E4M3 || fmt_x == SM_FP8_E5M2);
  const bool out_ok = out_type == SM_OUT_F32 || out_type == SM_OUT_F16 || out_type == SM_OUT_BF16;
  bool run;
  const int rc = linear24_args(a, &run, GLU, who, fmt_ok && out_ok, "fmt not SM_FP8_*, out_type not SM_OUT_*, ", blob, X, Y, tokens, out, in, ldx, ldy, 1,
                               out_type == SM_OUT_F32 ? 16 : 8, t, GROUPED ? &grp : nullptr);
  if (rc != SM_STATUS_SUCCESS || !run) return rc;
  a.Mtot = (GROUPED ? grp.groups : 1) * (GLU ? 2 * out : out);
  a.X = (const uint8_t*)X;
  a.nplanes = (int)(in / 64);
  a.out_type = out_type;
  a.w_scale = w_scale; a.x_scale = x_scale;
  hipStream_t st = (hipStream_t)stream;
  const int form = linear24_rule<GLU, GROUPED>(tokens, grp.groups, out, in, (size_t)device_cu_count());
  if (form == SM_LINEAR24_FORM_NOT_TAKEN) {
    set_error("%s: grid too large", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (fmt_w == SM_FP8_E4M3)
    return fmt_x == SM_FP8_E4M3 ? linear8_launch<SM_FP8_E4M3, SM_FP8_E4M3, GLU, GROUPED, GATHER>(a, grp, form, st, who)
                                : linear8_launch<SM_FP8_E4M3, SM_FP8_E5M2, GLU, GROUPED, GATHER>(a, grp, form, st, who);
  return fmt_x == SM_FP8_E4M3 ? linear8_launch<SM_FP8_E5M2, SM_FP8_E4M3, GLU, GROUPED, GATHER>(a, grp, form, st, who)
                              : linear8_launch<SM_FP8_E5M2, SM_FP8_E5M2, GLU, GROUPED, GATHER>(a, grp, form, st, who);
}

}  // namespace sm

using namespace sm;

extern "C" int sm_linear24_fp8_form(size_t tokens, size_t out_features, size_t in_features, size_t cus, int* form) {
  if (!form) {
    set_error("sm_linear24_fp8_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = linear24_form(tokens, out_features, in_features, cus ? cus : (size_t)device_cu_count());
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_linear24_fp8(const void* blob, const void* X, void* Y, size_t tokens, size_t out_features, size_t in_features, size_t ldx,
                               size_t ldy, int fmt_w, int fmt_x, int out_type, float alpha, float beta, const float* w_scale, const float* x_scale,
                               const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear8<false, false, false>(blob, X, Y, Linear24Groups{}, tokens, out_features, in_features, ldx, ldy, fmt_w, fmt_x, out_type,
                                      Linear24Tail{alpha, beta, epilogue}, w_scale, x_scale, stream);
}

extern "C" int sm_linear24_glu_form(size_t tokens, size_t hidden, size_t in_features, size_t cus, int* form) {
  if (!form) {
    set_error("sm_linear24_glu_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = linear24_glu_form(tokens, hidden, in_features, cus ? cus : (size_t)device_cu_count());
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_linear24_glu_fp8(const void* blob, const void* X, void* Y, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy,
                                   int fmt_w, int fmt_x, int out_type, int act, const float* w_scale, const float* x_scale, const float* bias,
                                   sm_stream_t stream) {
  return linear8<true, false, false>(blob, X, Y, Linear24Groups{}, tokens, hidden, in_features, ldx, ldy, fmt_w, fmt_x, out_type, linear24_glu_tail(act, bias),
                                     w_scale, x_scale, stream);
}

// ---- the grouped layers: `groups` experts of one shape behind one launch (the GROUPED instantiations of the tile kernels) ----------
extern "C" int sm_linear24_grouped_form(size_t tokens, size_t groups, size_t out_features, size_t in_features, size_t cus, int* form) {
  if (!form) {
    set_error("sm_linear24_grouped_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  *form = linear24_grouped_form(tokens, groups, out_features, in_features, cus ? cus : (size_t)device_cu_count());
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_linear24_grouped_fp8(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens,
                                       size_t out_features, size_t in_features, size_t ldx, size_t ldy, int fmt_w, int fmt_x, int out_type, float alpha,
                                       float beta, const float* w_scale, const float* x_scale, const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear8<false, true, false>(blob, X, Y, Linear24Groups{group_offsets, groups}, tokens, out_features, in_features, ldx, ldy, fmt_w, fmt_x, out_type,
                                     Linear24Tail{alpha, beta, epilogue}, w_scale, x_scale, stream);
}
extern "C" int sm_linear24_grouped_gather_fp8(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                              size_t groups, size_t tokens, size_t out_features, size_t in_features, size_t ldx, size_t ldy, int fmt_w,
                                              int fmt_x, int out_type, float alpha, float beta, const float* w_scale, const float* x_scale,
                                              const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear8<false, true, true>(blob, X, Y, Linear24Groups{group_offsets, groups, true, x_index, x_rows}, tokens, out_features, in_features, ldx, ldy,
                                    fmt_w, fmt_x, out_type, Linear24Tail{alpha, beta, epilogue}, w_scale, x_scale, stream);
}

extern "C" int sm_linear24_grouped_glu_fp8(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens, size_t hidden,
                                           size_t in_features, size_t ldx, size_t ldy, int fmt_w, int fmt_x, int out_type, int act, const float* w_scale,
                                           const float* x_scale, const float* bias, sm_stream_t stream) {
  return linear8<true, true, false>(blob, X, Y, Linear24Groups{group_offsets, groups}, tokens, hidden, in_features, ldx, ldy, fmt_w, fmt_x, out_type,
                                    linear24_glu_tail(act, bias), w_scale, x_scale, stream);
}
extern "C" int sm_linear24_grouped_glu_gather_fp8(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                                  size_t groups, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy, int fmt_w,
                                                  int fmt_x, int out_type, int act, const float* w_scale, const float* x_scale, const float* bias,
                                                  sm_stream_t stream) {
  return linear8<true, true, true>(blob, X, Y, Linear24Groups{group_offsets, groups, true, x_index, x_rows}, tokens, hidden, in_features, ldx, ldy, fmt_w,
                                   fmt_x, out_type, linear24_glu_tail(act, bias), w_scale, x_scale, stream);
}
