// linear24_f16.hip -- the 2:4 WEIGHT-sparse linear layer in the token-major layout (sm_linear24_{f16,bf16}, extension):
//     Y[tokens][out] = act(alpha * X[tokens][in] . W_2:4[out][in]^T + beta * R + bias)
// W is the blob sm_compress24_{f16,bf16}(W, m = out, k = in) writes (srcA of v_smfmac_f32_16x16x64, as in spmma_f16.hip); X and Y
// stay as the caller holds them.  That is the instruction's own layout (mma_tile.h, operand maps): B lane l wants, of token l & 15,
// dense k 8g .. 8g+7 and 32+8g .. 32+8g+7 (g = l >> 4) -- two 16-byte pieces of one X row, plain ds_read_b128, no transposing
// read; and the lane ends with four consecutive out features of one token -- 8 contiguous bytes of Y's row, no LDS transpose.
//
// The operand-independent core (rule, argument checks, epilogue and store, decode combine, tile launcher) is linear24_common.h,
// shared with linear24_fp8.hip.  Two forms behind the one entry point (linear24_form(); this layer asks it with LINEAR24_F16_CUS):
//   tile    BM out features x BN tokens per workgroup, 64 dense k per stage (BK = 64, not 128: DESIGN.md 8) brought in by global_load_lds into a ring of NS stage
//           buffers (counted vmcnt, one barrier per stage: the pipeline of spmma_f16_dma_kernel).  K is walked in order, one SMFMAC
//           per 64-k step into one accumulator: the bits of sm_transpose o sm_spmma_{f16,bf16}[_ex] o sm_transpose.
//   decode  tokens <= LINEAR24_DECODE_MAX and out <= LINEAR24_DECODE_MAX_OUT: a pure weight stream.  One workgroup per 16 out features; its waves split K among
//           themselves, stream the blob straight to registers (no other wave shares it) and add their fp32 partial tiles through
//           LDS in wave order: deterministic, no workspace.  Other K order than the tile form: held to the arithmetic's bound.
// The gated layer (sm_linear24_glu_{f16,bf16}: Y = act(gate) * up of a fused gate/up weight) is the GLU instantiation of the same two
// kernels: only the blob rows a fragment is fetched from (linear24_glu_row) and the store (linear24_store_glu) differ.
// Below the kernels: one host template, linear24<BF, GLU, GROUPED, GATHER>, behind all twelve launching entry points of this file.
#include "linear24_common.h"

namespace sm {

// the compute-unit count the rule is asked with: a constant, not the device's, so the dispatch is the same everywhere
constexpr size_t LINEAR24_F16_CUS = 256;
// the entry points' names in their messages: [GLU][plain, grouped, gathered]
static const char* const LINEAR24_16_WHO[2][3] = {
    {"sm_linear24_{f16,bf16}", "sm_linear24_grouped_{f16,bf16}", "sm_linear24_grouped_gather_{f16,bf16}"},
    {"sm_linear24_glu_{f16,bf16}", "sm_linear24_grouped_glu_{f16,bf16}", "sm_linear24_grouped_glu_gather_{f16,bf16}"}};

struct Linear24Args : Linear24Core {  // vals stage-major [in/64][out][64 B]
  const half_t* X;
  int nkt;  // in / 64
};

// One 64-deep stage for one wave: A fragments + index halfwords from the 64-byte-row image (as smfmac_stage reads them), X fragments
// as two ds_read_b128 per 16 tokens, issued by hand with counted lgkmcnt (fragment j+1's reads in flight under fragment j's SMFMACs;
// the plain C++ form would make the compiler drain the in-flight DMA first).  The compiler does not know that the read's outputs are
// pending until the wait that names them; the disassembly of every instantiation was checked for this: between a ds_read_b128 pair and
// the s_waitcnt that covers it no instruction reads or copies the pair's destination registers, and the SMFMACs of a fragment follow
// its wait (sched_barrier).  The X image must be 128-byte aligned for the `^ 64` below.
template <int FM, int FN, bool BF>
__device__ __forceinline__ void linear24_stage(const char* As, const char* Ms, const char* Xs, unsigned row0, unsigned col0, unsigned lane,
                                               f4 (&acc)[FM][FN]) {
  const unsigned g = lane >> 4, r = lane & 15u;
  h8 af[FM];
  int idx[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const unsigned row = row0 + i * 16 + r;
    af[i] = *reinterpret_cast<const h8*>(As + row * 64u + 16u * (g ^ a64_swz(row)));
    idx[i] = (int)*reinterpret_cast<const unsigned short*>(Ms + row * 8u + 2u * g);
  }
  const unsigned xs_addr = (unsigned)(uintptr_t)(lds_char*)Xs;
  u4 lo[2], hi[2];
  auto issue = [&](int j, u4& v0, u4& v1) {
    const unsigned t = col0 + j * 16 + r;
    const unsigned a0 = xs_addr + t * 128u + 16u * (g ^ x_swz(t));
    const unsigned a1 = a0 ^ 64u;  // chunk 4 + g: the same slot arithmetic with bit 2 flipped (rows are 128-byte aligned)
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3" : "=&v"(v0), "=&v"(v1) : "v"(a0), "v"(a1) : "memory");
  };
  issue(0, lo[0], hi[0]);
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int c = j & 1, n = c ^ 1;
    if (j + 1 < FN) {
      issue(j + 1, lo[n], hi[n]);
      asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(lo[c]), "+v"(hi[c]) :: "memory");
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[c]), "+v"(hi[c]) :: "memory");
    }
    __builtin_amdgcn_sched_barrier(0);
    typedef unsigned int u8v __attribute__((ext_vector_type(8)));
    const u8v all = {lo[c][0], lo[c][1], lo[c][2], lo[c][3], hi[c][0], hi[c][1], hi[c][2], hi[c][3]};
    const h16 xf = __builtin_bit_cast(h16, all);
#pragma unroll
    for (int i = 0; i < FM; ++i) acc[i][j] = smfmac16<BF>(af[i], xf, acc[i][j], idx[i]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Tile form.  Stage = 64 dense k: blob values [BM][64 B] (16 rows per DMA instruction, a64_swz on the source), metadata
// [BM][8 B] (4-byte pieces, 32 rows per instruction: any row count, no 16-byte plane alignment asked of `out`), X [BN][128 B]
// (8 token rows per instruction, whole 128-byte lines, x_swz on the source).  Rows / tokens past the edge are clamped to the last
// valid one: their products land in outputs that are never stored (an output depends on its own row and its own token only).
// ---------------------------------------------------------------------------------------------------------------------------
// GLU: the tile's BM rows are BM / 2 gate rows and the BM / 2 up rows of the same hidden features, interleaved by 16-row fragment; p.out
// is `hidden`, the width of Y, and the blob has 2 * p.out rows.
// GROUPED (sm_linear24_grouped_*): tiles_n counts token-tile SLOTS, the grid's bound; the workgroup finds its expert, out tile and token
// tile in group_offsets (linear24_group_view), returns when it is past the last real tile, and else runs this body on the block cut down
// to its expert.
// GATHER (sm_linear24_grouped_*gather_*, GROUPED only): the X rows of the tile are those x_index names (linear24_gather_row), fetched by
// the lanes that issue the X DMA, once, ahead of the first stage; Y, R and a per-token bias stay in the sorted rows.
template <int BM, int BN, int WM, int WN, int NS, bool BF, bool GLU = false, bool GROUPED = false, bool GATHER = false>
__global__ __launch_bounds__(64 * WM * WN) void linear24_tile_kernel(const typename Linear24ArgsSel<Linear24Args, GROUPED>::type pk) {
  typename Linear24ArgsSel<Linear24Args, GROUPED>::view_t p = pk;
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM, TN = BN / WN, FM = TM / 16, FN = TN / 16;
  static_assert(FM >= 1 && FN >= 1 && BM % 32 == 0 && BN % 8 == 0, "tile");
  static_assert(!GLU || FM % 2 == 0, "a wave of a gated tile holds whole (gate, up) fragment pairs");
  static_assert(NS >= 2 && NS <= 4, "ring depth");
  static_assert(GROUPED || !GATHER, "the gathered layers are grouped layers");
  constexpr int SA = BM * 64, SM_ = BM * 8, SX = BN * 128, STAGE = SA + SM_ + SX;
  constexpr int A_N = BM / 16, M_N = BM / 32, X_N = BN / 8, W = A_N + M_N + X_N;
  constexpr int SL = (W + NW - 1) / NW;  // DMA slots per wave
  constexpr int LPS = W / NW;            // least any wave issues per stage: the vmcnt unit
  static_assert(LPS >= 1, "every wave must issue at least one DMA per stage");
  static_assert((SA + SM_) % 128 == 0 && STAGE % 128 == 0, "the X image of every stage buffer is 128-byte aligned (linear24_stage)");
  extern __shared__ __attribute__((aligned(128))) char smem[];

  const unsigned tid = threadIdx.x, lane = tid & 63u, g = lane >> 4, r = lane & 15u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned wm = wave / WN, wn = wave % WN;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tm = lid / (unsigned)p.tiles_n, tile_n = lid - tm * (unsigned)p.tiles_n;  // (a grouped workgroup's come from its view)
  // row and token indices are unsigned: an edge tile's origin plus its extent may pass 2^31 - 1 (never 2^32)
  unsigned tile_m = tm, n0 = tile_n * BN;
  size_t rows = GLU ? 2 * (size_t)p.out : (size_t)p.out;             // rows of the blob: the plane stride
  if constexpr (GROUPED) {
    if (!linear24_group_view<BN>(p, pk.group_offsets, pk.groups, blockIdx.x, (unsigned)rows, 64u, tile_m, n0)) return;  // (workgroup-uniform)
    rows *= (size_t)pk.groups;
  }
  const unsigned m0 = tile_m * BM;
  const unsigned mlast = (unsigned)p.out - 1u, tlast = (unsigned)p.tokens - 1u;
  const unsigned hid0 = tile_m * (BM / 2);                           // GLU: the tile's first hidden feature

  // the lane's bias values, fetched ahead of the K loop (plain loads, older than every DMA piece: the counted waits cover them)
  const bool bias_out = p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_COL, bias_tok = p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_ROW;
  f4 bo[FM];
  float bt[FN];
#pragma unroll
  for (int i = 0; i < FM; ++i) bo[i] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < FN; ++j) bt[j] = 0.f;
  if (bias_out) {
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      if constexpr (GLU) bo[i] = linear24_per_out(p.e.bias + ((i & 1) ? p.out : 0), hid0 + (wm * (TM / 2) + (i / 2) * 16 + 4u * g), (unsigned)p.out);
      else bo[i] = linear24_per_out(p.e.bias, m0 + (wm * TM + i * 16 + 4u * g), (unsigned)p.out);
    }
  }
  if (bias_tok) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const unsigned t = n0 + (wn * TN + j * 16 + r);
      bt[j] = p.e.bias[t < tlast ? t : tlast];
    }
  }

  const char* src[SL];
  size_t step[SL];
  unsigned loff[SL];
#pragma unroll
  for (int i = 0; i < SL; ++i) {
    const unsigned t = wave + (unsigned)NW * i;
    if (t < (unsigned)A_N) {
      const unsigned row = 16u * t + (lane >> 2), cs = (lane & 3u) ^ a64_swz(row);
      unsigned gr = m0 + row;
      gr = gr < mlast ? gr : mlast;
      if constexpr (GLU) gr = linear24_glu_row(hid0, row, (unsigned)p.out);
      src[i] = p.vals + (size_t)gr * 64 + 16u * cs;
      step[i] = rows * 64;
      loff[i] = t * 1024u;
    } else if (t < (unsigned)(A_N + M_N)) {
      const unsigned u = t - A_N;
      unsigned gr = m0 + (32u * u + (lane >> 1));
      gr = gr < mlast ? gr : mlast;
      if constexpr (GLU) gr = linear24_glu_row(hid0, 32u * u + (lane >> 1), (unsigned)p.out);  // (per lane half: a gate and an up fragment)
      src[i] = p.meta + (size_t)gr * 8 + 4u * (lane & 1u);
      step[i] = rows * 8;
      loff[i] = SA + u * 256u;
    } else {
      const unsigned j = t - (A_N + M_N), row = 8u * j + (lane >> 3), cs = (lane & 7u) ^ x_swz(row);
      unsigned gt = n0 + row;
      gt = gt < tlast ? gt : tlast;
      if constexpr (GATHER) gt = linear24_gather_row(pk.x_index, pk.x_rows, gt);
      src[i] = reinterpret_cast<const char*>(p.X + (size_t)gt * p.ldx + 8u * cs);
      step[i] = 128;
      loff[i] = SA + SM_ + j * 1024u;
    }
  }
  auto stage = [&](int kt, int buf) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < SL; ++i) {
      const unsigned t = wave + (unsigned)NW * i;  // wave-uniform
      if (t >= (unsigned)W) continue;
      gptr_t* gp = (gptr_t*)(src[i] + (size_t)kt * step[i]);
      lptr_t* lp = (lptr_t*)(base + loff[i]);
      if (t >= (unsigned)A_N && t < (unsigned)(A_N + M_N)) __builtin_amdgcn_global_load_lds(gp, lp, 4, 0, 0);
      else __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
    }
  };

  f4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  // the ring of spmma_f16_dma_kernel: wait for this wave's DMA of stage kt, barrier, refill the buffer read in iteration kt-1
  const int nkt = p.nkt;
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
    linear24_stage<FM, FN, BF>(As, As + SA, As + SA + SM_, wm * TM, wn * TN, lane, acc);
    cur = cur + 1 == NS ? 0 : cur + 1;
    fill = fill + 1 == NS ? 0 : fill + 1;
  }

  // ---- store: no LDS, no barrier -- each lane's four out features are one piece of Y's row
  if constexpr (GLU) {
#pragma unroll
    for (int i = 0; i < FM; i += 2)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        linear24_store_glu<Elt16<BF>, false>(p, acc[i][j], acc[i + 1][j], hid0 + (wm * (TM / 2) + (i / 2) * 16 + 4u * g), n0 + (wn * TN + j * 16 + r), f4{},
                                             f4{}, 1.f, bo[i], bo[i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j)
        linear24_store_frag<Elt16<BF>, false>(p, acc[i][j], m0 + (wm * TM + i * 16 + 4u * g), n0 + (wn * TN + j * 16 + r), f4{}, 1.f, bt[j], bo[i]);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Decode form: tokens <= 16 FN (the library instantiates FN = 1; the threshold measurement of DESIGN.md 4.13 built FN = 2 and 4).  Workgroup = 16 out features x NWV waves; wave w takes the 64-k stages w, w + NWV, ... (ascending),
// U of them requested before the first is multiplied.  Per stage a wave reads 1 KiB of values and 128 B of metadata, both
// contiguous (16 consecutive rows of one plane), non-temporal; X (<= 64 rows, shared by every workgroup) comes from L2.  Token
// columns at or beyond `tokens` are fed zeros.  The partial tiles meet in LDS and are added in wave order 0, 1, ..: the same
// bits on every run.
// ---------------------------------------------------------------------------------------------------------------------------
// GLU: one workgroup per 16 hidden features; a wave streams the gate fragment and the up fragment of its stage (NF = 2 value and
// metadata loads) against the same X registers, K split and combine order unchanged: g and u have this kernel's plain bits.
template <int FN, int NWV, int U, bool BF, bool GLU = false>
__global__ __launch_bounds__(64 * NWV) void linear24_decode_kernel(const Linear24Args p) {
  static_assert(!GLU || FN == 1, "the gated decode form holds one token fragment");
  constexpr int NF = GLU ? 2 : 1;  // blob fragments per stage
  const size_t rows = GLU ? 2 * (size_t)p.out : (size_t)p.out;
  const unsigned tid = threadIdx.x, lane = tid & 63u, g = lane >> 4, r = lane & 15u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned m0 = blockIdx.x * 16u;
  unsigned row = m0 + r;
  row = row < (unsigned)p.out - 1u ? row : (unsigned)p.out - 1u;  // (clamped rows: computed, never stored)
  const char* va = p.vals + (size_t)row * 64 + 16u * g;
  const char* me = p.meta + (size_t)row * 8 + 2u * g;
  const size_t vstep = rows * 64, mstep = rows * 8;
  const size_t vup = GLU ? (size_t)p.out * 64 : 0, mup = GLU ? (size_t)p.out * 8 : 0;  // from a gate row to its up row
  const half_t* xr[FN];
  bool xv[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int t = 16 * j + (int)r;
    xv[j] = t < p.tokens;
    xr[j] = p.X + (size_t)(xv[j] ? t : 0) * p.ldx + 8u * g;
  }
  f4 acc[NF * FN];  // GLU: {gate, up}
#pragma unroll
  for (int j = 0; j < NF * FN; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};

  for (int s = (int)wave; s < p.nkt; s += NWV * U) {
    u4 a[U][NF], x0[U][FN], x1[U][FN];
    int ix[U][NF];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ss = s + u * NWV;  // wave-uniform
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        a[u][f] = u4{0u, 0u, 0u, 0u};
        ix[u][f] = 0;
        if (ss < p.nkt) {
          a[u][f] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(va + (size_t)ss * vstep + f * vup));
          ix[u][f] = (int)__builtin_nontemporal_load(reinterpret_cast<const unsigned short*>(me + (size_t)ss * mstep + f * mup));
        }
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        x0[u][j] = u4{0u, 0u, 0u, 0u};
        x1[u][j] = u4{0u, 0u, 0u, 0u};
        if (ss < p.nkt && xv[j]) {
          x0[u][j] = *reinterpret_cast<const u4*>(xr[j] + (size_t)ss * 64);
          x1[u][j] = *reinterpret_cast<const u4*>(xr[j] + (size_t)ss * 64 + 32);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (s + u * NWV < p.nkt) {
        typedef unsigned int u8v __attribute__((ext_vector_type(8)));
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const u8v all = {x0[u][j][0], x0[u][j][1], x0[u][j][2], x0[u][j][3], x1[u][j][0], x1[u][j][1], x1[u][j][2], x1[u][j][3]};
#pragma unroll
          for (int f = 0; f < NF; ++f)
            acc[j * NF + f] = smfmac16<BF>(__builtin_bit_cast(h8, a[u][f]), __builtin_bit_cast(h16, all), acc[j * NF + f], ix[u][f]);
        }
      }
    }
  }
  if constexpr (GLU) linear24_decode_tail_glu<Linear24Core, linear24_store_glu<Elt16<BF>, false>, false, NWV>(p, acc, m0);
  else linear24_decode_tail<Linear24Core, linear24_store_frag<Elt16<BF>, false>, false, FN, NWV>(p, acc, m0);
}

template <int BM, int BN, int WM, int WN, int NS, bool BF, bool GLU, bool GROUPED, bool GATHER>
static int launch_linear24_tile16(const Linear24Args& a, const Linear24Groups& grp, hipStream_t st, const char* who) {
  return launch_linear24_tile<Linear24Args, GROUPED, linear24_tile_kernel<BM, BN, WM, WN, NS, BF, GLU, GROUPED, GATHER>, GLU ? BM / 2 : BM, BN, 64 * WM * WN,
                              (size_t)NS * (BM * 72 + BN * 128)>(a, grp, st, who, "linear24_tile_kernel");
}

}  // namespace sm

using namespace sm;

// Every entry point of this file: the checks, the rule, the launch.  GLU: `out` is `hidden` and t holds act / bias; GROUPED: grp is read
// (the tile forms only: no grouped decode kernel, and the grouped rule never answers DECODE); GATHER (GROUPED only): X through grp.x_index.
template <bool BF, bool GLU, bool GROUPED, bool GATHER>
static int linear24(const void* blob, const void* X, void* Y, const Linear24Groups& grp, size_t tokens, size_t out, size_t in, size_t ldx, size_t ldy,
                    const Linear24Tail& t, sm_stream_t stream) {
  static_assert(GROUPED || !GATHER, "only a grouped layer gathers");
  const char* who = LINEAR24_16_WHO[GLU][GROUPED + GATHER];
  Linear24Args a = {};
  bool run;
  const int rc = linear24_args(a, &run, GLU, who, true, "", blob, X, Y, tokens, out, in, ldx, ldy, 2, 8, t, GROUPED ? &grp : nullptr);
  if (rc != SM_STATUS_SUCCESS || !run) return rc;
  a.X = (const half_t*)X;
  a.nkt = (int)(in / 64);
  hipStream_t st = (hipStream_t)stream;
  const int form = linear24_rule<GLU, GROUPED>(tokens, grp.groups, out, in, LINEAR24_F16_CUS);
  if constexpr (!GROUPED)
    if (form == SM_LINEAR24_FORM_DECODE)
      return launch_linear24_decode<Linear24Args, linear24_decode_kernel<1, 16, 4, BF, GLU>, 64 * 16>(a, st, "linear24_decode_kernel");
  switch (form) {
    case SM_LINEAR24_FORM_TILE128: return launch_linear24_tile16<128, 128, 2, 2, 3, BF, GLU, GROUPED, GATHER>(a, grp, st, who);
    case SM_LINEAR24_FORM_TILE128x64: return launch_linear24_tile16<128, 64, 4, 1, 3, BF, GLU, GROUPED, GATHER>(a, grp, st, who);
    case SM_LINEAR24_FORM_TILE64: return launch_linear24_tile16<64, 64, 2, 2, 3, BF, GLU, GROUPED, GATHER>(a, grp, st, who);
  }
  set_error("%s: grid too large", who);
  return SM_STATUS_NOT_SUPPORTED;
}

extern "C" int sm_linear24_f16(const void* blob, const void* X, void* Y, size_t tokens, size_t out_features, size_t in_features, size_t ldx,
                               size_t ldy, float alpha, float beta, const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear24<false, false, false, false>(blob, X, Y, Linear24Groups{}, tokens, out_features, in_features, ldx, ldy, Linear24Tail{alpha, beta, epilogue},
                                              stream);
}
extern "C" int sm_linear24_bf16(const void* blob, const void* X, void* Y, size_t tokens, size_t out_features, size_t in_features, size_t ldx,
                                size_t ldy, float alpha, float beta, const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear24<true, false, false, false>(blob, X, Y, Linear24Groups{}, tokens, out_features, in_features, ldx, ldy, Linear24Tail{alpha, beta, epilogue},
                                             stream);
}

extern "C" int sm_linear24_glu_f16(const void* blob, const void* X, void* Y, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy,
                                   int act, const float* bias, sm_stream_t stream) {
  return linear24<false, true, false, false>(blob, X, Y, Linear24Groups{}, tokens, hidden, in_features, ldx, ldy, linear24_glu_tail(act, bias), stream);
}
extern "C" int sm_linear24_glu_bf16(const void* blob, const void* X, void* Y, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy,
                                    int act, const float* bias, sm_stream_t stream) {
  return linear24<true, true, false, false>(blob, X, Y, Linear24Groups{}, tokens, hidden, in_features, ldx, ldy, linear24_glu_tail(act, bias), stream);
}

// ---- the grouped layers: `groups` experts of one shape behind one launch (the GROUPED instantiations of the tile kernels); GATHER: the
// same with X read through x_index (sm_linear24_grouped_*gather_*: grp.gather set, the GATHER instantiations) -------------------------
extern "C" int sm_linear24_grouped_f16(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens,
                                       size_t out_features, size_t in_features, size_t ldx, size_t ldy, float alpha, float beta,
                                       const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear24<false, false, true, false>(blob, X, Y, Linear24Groups{group_offsets, groups}, tokens, out_features, in_features, ldx, ldy,
                                             Linear24Tail{alpha, beta, epilogue}, stream);
}
extern "C" int sm_linear24_grouped_bf16(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens,
                                        size_t out_features, size_t in_features, size_t ldx, size_t ldy, float alpha, float beta,
                                        const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear24<true, false, true, false>(blob, X, Y, Linear24Groups{group_offsets, groups}, tokens, out_features, in_features, ldx, ldy,
                                            Linear24Tail{alpha, beta, epilogue}, stream);
}
extern "C" int sm_linear24_grouped_gather_f16(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                              size_t groups, size_t tokens, size_t out_features, size_t in_features, size_t ldx, size_t ldy, float alpha,
                                              float beta, const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear24<false, false, true, true>(blob, X, Y, Linear24Groups{group_offsets, groups, true, x_index, x_rows}, tokens, out_features, in_features, ldx,
                                            ldy, Linear24Tail{alpha, beta, epilogue}, stream);
}
extern "C" int sm_linear24_grouped_gather_bf16(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                               size_t groups, size_t tokens, size_t out_features, size_t in_features, size_t ldx, size_t ldy, float alpha,
                                               float beta, const sm_epilogue_t* epilogue, sm_stream_t stream) {
  return linear24<true, false, true, true>(blob, X, Y, Linear24Groups{group_offsets, groups, true, x_index, x_rows}, tokens, out_features, in_features, ldx,
                                           ldy, Linear24Tail{alpha, beta, epilogue}, stream);
}

extern "C" int sm_linear24_grouped_glu_f16(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens,
                                           size_t hidden, size_t in_features, size_t ldx, size_t ldy, int act, const float* bias, sm_stream_t stream) {
  return linear24<false, true, true, false>(blob, X, Y, Linear24Groups{group_offsets, groups}, tokens, hidden, in_features, ldx, ldy,
                                            linear24_glu_tail(act, bias), stream);
}
extern "C" int sm_linear24_grouped_glu_bf16(const void* blob, const void* X, void* Y, const int* group_offsets, size_t groups, size_t tokens,
                                            size_t hidden, size_t in_features, size_t ldx, size_t ldy, int act, const float* bias, sm_stream_t stream) {
  return linear24<true, true, true, false>(blob, X, Y, Linear24Groups{group_offsets, groups}, tokens, hidden, in_features, ldx, ldy,
                                           linear24_glu_tail(act, bias), stream);
}
extern "C" int sm_linear24_grouped_glu_gather_f16(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                                  size_t groups, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy, int act,
                                                  const float* bias, sm_stream_t stream) {
  return linear24<false, true, true, true>(blob, X, Y, Linear24Groups{group_offsets, groups, true, x_index, x_rows}, tokens, hidden, in_features, ldx, ldy,
                                           linear24_glu_tail(act, bias), stream);
}
extern "C" int sm_linear24_grouped_glu_gather_bf16(const void* blob, const void* X, void* Y, const int* group_offsets, const int* x_index, size_t x_rows,
                                                   size_t groups, size_t tokens, size_t hidden, size_t in_features, size_t ldx, size_t ldy, int act,
                                                   const float* bias, sm_stream_t stream) {
  return linear24<true, true, true, true>(blob, X, Y, Linear24Groups{group_offsets, groups, true, x_index, x_rows}, tokens, hidden, in_features, ldx, ldy,
                                          linear24_glu_tail(act, bias), stream);
}
