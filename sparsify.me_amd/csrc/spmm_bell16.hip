// spmm_bell16.hip -- Blocked-ELL x dense on the 16-bit matrix cores (row a6 in fp16 / bfloat16):
//   sm_spmm_bell_{f16,bf16}          one A
//   sm_spmm_bell_batched_{f16,bf16}  one A and one C per batch entry, B shared (the reference's driver, spmm.hxx:90-111)
// Same semantics as sm_spmm_bell_f32 (spmm.hxx:57-67,107-110 declare these operands CUDA_R_16F with fp32 compute):
// C (rows x n, ldc = rows) = alpha * A * B (cols x n, ldb = cols) + beta * C, fp32 accumulation, one rounding.
//
// Mapping.  Both dense operands are K-contiguous: a column of B (one n) is a row of B^T along k, and a row of A is a row along
// k.  So both stage images are the [rows][128 B] a_off image of mma_tile.h (64 k per row, XOR-swizzled chunks), read with
// ds_read_b128, and v_mfma_f32_16x16x32 takes A as srcA and B^T as srcB: each lane ends with four consecutive ROWS of one
// column of C, which is one 8-byte piece of the column-major C.
//
// The A side of a 64-deep stage is BUILT in LDS instead of loaded: each wave owns 16 rows of the 128-row tile, zeroes them and
// scatters the stored values of those rows whose block column falls in the stage.  Nothing dense ever reaches HBM.
//   Fast path: every producer writes a block row's indices ascending.  Then the values of one row that land in stage kt are a
//   contiguous slice values[row][p_begin(kt) .. p_begin(kt + 1)) of at most 64 elements, the same for every row of the block
//   row.  A per-tile prologue reads the tile's indices once, checks that the stored ones are strictly ascending and in range
//   (empty ids, >= cols / block_size, only after them), and writes p_begin for every (block row, stage) into an LDS table.  A
//   stage then costs each lane one value and one index load per owned row, issued one stage ahead, with no search.
//   Generic path (a tile whose indices fail the check, or whose table does not fit): every lane walks the whole row per stage.
// Both paths produce the same dense stage image, and the MFMA sum runs over k in a fixed order: the result does not depend on
// the order in which a block row stores its blocks, bit for bit.  No atomics, no workspace, no host synchronisation.
#include "mma_tile.h"

namespace sm {

constexpr int BELL16_TM = 128;    // rows of A per tile
constexpr int BELL16_NW = 8;      // waves per workgroup; each builds BELL16_TM / BELL16_NW rows of the A image
constexpr int BELL16_MAXB = 64;   // batch entries per launch: the pointer tables travel in the kernel arguments
constexpr size_t BELL16_LDS_MAX = 160 * 1024 - 256;

struct Bell16Args {
  const unsigned short* values[BELL16_MAXB];
  const uint64_t* idx[BELL16_MAXB];
  half_t* C[BELL16_MAXB];
  const half_t* B;
  int rows, cols, n, bs, ell_cols, bcols, nbc, nkt;
  int tiles_m, tiles_n;
  unsigned magic;  // ceil(2^32 / bs) for bs > 1: pos / bs == umulhi(pos, magic) for pos, bs < 2^16
  int table;       // 1: the per-tile stage table fits in LDS (fast path possible); 0: generic path on every tile
  float alpha, beta;
};

__device__ __forceinline__ unsigned bell_div(unsigned pos, unsigned bs, unsigned magic) {
  return bs == 1u ? pos : __umulhi(pos, magic);
}

template <int TN, int WM, int WN, bool BF, bool VEC>
__global__ __launch_bounds__(64 * BELL16_NW) void spmm_bell16_kernel(const Bell16Args p) {
  constexpr int TM = BELL16_TM, NW = BELL16_NW, NT = 64 * NW, RPW = TM / NW;
  static_assert(WM * WN == NW, "wave grid");
  constexpr int TMW = TM / WM, TNW = TN / WN, FM = TMW / 16, FN = TNW / 16;
  static_assert(FM >= 1 && FN >= 1, "wave tile");
  constexpr int SA = TM * 128, SB = TN * 128, STAGE = SA + SB;
  constexpr int B_CH = TN * 8 / NT;  // 16-byte chunks of the B^T stage image per thread
  static_assert(B_CH >= 1, "B chunks");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* tab = reinterpret_cast<unsigned short*>(smem + 2 * STAGE);
  __shared__ int tile_bad;

  const unsigned tid = threadIdx.x, lane = tid & 63u, g = lane >> 4, r16 = lane & 15u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned wm = wave / WN, wn = wave % WN;
  const unsigned tiles = (unsigned)p.tiles_m * (unsigned)p.tiles_n;
  const unsigned lid = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned b = lid / tiles, trem = lid - b * tiles;
  const unsigned tile_m = trem / (unsigned)p.tiles_n, tile_n = trem - tile_m * (unsigned)p.tiles_n;
  const int m0 = (int)tile_m * TM, n0 = (int)tile_n * TN;
  const unsigned short* __restrict__ V = p.values[b];
  const uint64_t* __restrict__ I = p.idx[b];
  half_t* C = p.C[b];
  const int bs = p.bs, nkt = p.nkt, P = nkt + 1;
  const int br0 = m0 / bs;
  const int last_row = (m0 + TM < p.rows ? m0 + TM : p.rows) - 1;
  const int nbr = last_row / bs - br0 + 1;

  // ---- prologue: check the tile's block rows and build the stage table (p_begin per block row and stage, kt = 0 .. nkt).
  // Every entry is handled on its own, with its neighbours' ids (no running count, no chain of dependent loads): a wave takes
  // 64 consecutive entries of one block row per item and U items per round, whose loads are all issued before any is used.
  if (tid == 0) tile_bad = p.table ? 0 : 1;
  __syncthreads();
  if (p.table) {
    if (p.bcols == 0) {  // nothing stored anywhere: every slice is empty
      for (int q = (int)tid; q < nbr * P; q += NT) tab[q] = 0;
    } else {
      constexpr int U = 4;
      const int ch = (p.bcols + 63) / 64, items = nbr * ch, last = p.bcols - 1;
      for (int q0 = (int)wave; q0 < items; q0 += NW * U) {
        uint64_t bc[U], pr[U], nx[U];
        int ee[U], bb[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int q = q0 + NW * u < items ? q0 + NW * u : items - 1;  // clamped: the loads stay unconditional
          const int br = q / ch, e = (q - br * ch) * 64 + (int)lane;
          const int ec = e < last ? e : last;
          const uint64_t* ci = I + (size_t)(br0 + br) * p.bcols;
          bc[u] = ci[ec];
          pr[u] = ci[ec > 0 ? ec - 1 : 0];
          nx[u] = ci[ec < last ? ec + 1 : last];
          ee[u] = e;
          bb[u] = br;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (q0 + NW * u >= items) break;
          const int e = ee[u];
          if (e > last) continue;
          unsigned short* t = tab + bb[u] * P;
          const bool v = bc[u] < (uint64_t)p.nbc;
          const bool pv = e > 0 && pr[u] < (uint64_t)p.nbc, nv = e < last && nx[u] < (uint64_t)p.nbc;
          // the stored blocks form a strictly ascending prefix of the block row
          if (v && e > 0 && !(pv && pr[u] < bc[u])) tile_bad = 1;
          if (v) {
            const int f = (int)bc[u] * bs, l = f + bs - 1;  // bc < nbc: f + bs <= cols
            const int pl = pv ? (int)pr[u] * bs + bs - 1 : -1;
            for (int kt = (pl + 64) / 64; kt <= l / 64; ++kt) {
              const int skip = kt * 64 - f;
              t[kt] = (unsigned short)(e * bs + (skip > 0 ? skip : 0));
            }
            // the last stored block ends the row's slice for every later stage
            if (!nv)
              for (int kt = l / 64 + 1; kt <= nkt; ++kt) t[kt] = (unsigned short)((e + 1) * bs);
          } else if (e == 0) {  // nothing stored in this block row (a stored block after this one fails the check)
            for (int kt = 0; kt <= nkt; ++kt) t[kt] = 0;
          }
        }
      }
    }
  }
  __syncthreads();
  const bool fast = tile_bad == 0;

  // ---- per-stage loads, issued one stage ahead
  u4 rb[B_CH];
  unsigned short av[RPW];
  unsigned ai[RPW];
  int ao[RPW];
  auto load_stage = [&](int kt) {
    const int k0 = kt * 64;
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const unsigned q = tid + (unsigned)NT * i, nr = q >> 3, kc = q & 7u;
      const int gn = n0 + (int)nr, gk = k0 + 8 * (int)kc;
      u4 v = {0u, 0u, 0u, 0u};
      if (gn < p.n && gk < p.cols) {
        const half_t* src = p.B + (size_t)gn * p.cols + gk;
        if (VEC) {
          v = *reinterpret_cast<const u4*>(src);  // cols % 8 == 0: a chunk is all in or all out
        } else {
          h8 e;
#pragma unroll
          for (int t = 0; t < 8; ++t) e[t] = (gk + t < p.cols) ? src[t] : (half_t)0.0f;
          v = __builtin_bit_cast(u4, e);
        }
      }
      rb[i] = v;
    }
    if (!fast) return;
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int row = (int)wave * RPW + i, gr = m0 + row;
      ai[i] = ~0u;  // no value of this row in the stage at this lane
      av[i] = 0;
      ao[i] = 0;
      if (gr >= p.rows) continue;
      const int brl = gr / bs - br0;
      const int pb = tab[brl * P + kt], pe = tab[brl * P + kt + 1];
      const int pos = pb + (int)lane;
      if (pos >= pe) continue;
      const unsigned e = bell_div((unsigned)pos, (unsigned)bs, p.magic);
      av[i] = V[(size_t)gr * p.ell_cols + pos];
      ai[i] = reinterpret_cast<const unsigned*>(I)[2 * ((size_t)(br0 + brl) * p.bcols + e)];  // low word: a stored id < 2^31
      ao[i] = pos - (int)e * bs - k0;  // + id * bs = the column inside the stage
    }
  };
  auto put = [&](char* As, int row, int col, unsigned short v) {
    *reinterpret_cast<unsigned short*>(As + a_off((unsigned)row, (unsigned)col >> 3) + 2u * ((unsigned)col & 7u)) = v;
  };
  auto store_stage = [&](char* As, int kt) {
    char* Bs = As + SA;
#pragma unroll
    for (int i = 0; i < B_CH; ++i) {
      const unsigned q = tid + (unsigned)NT * i;
      *reinterpret_cast<u4*>(Bs + a_off(q >> 3, q & 7u)) = rb[i];
    }
    // this wave's rows: zero, then scatter (one wave, LDS order)
#pragma unroll
    for (int j = 0; j < RPW * 8 / 64; ++j) {
      const unsigned q = lane + 64u * j;
      *reinterpret_cast<u4*>(As + a_off(wave * RPW + (q >> 3), q & 7u)) = u4{0u, 0u, 0u, 0u};
    }
    if (fast) {
#pragma unroll
      for (int i = 0; i < RPW; ++i)
        if (ai[i] != ~0u) {
          const int col = (int)ai[i] * bs + ao[i];
          if ((unsigned)col < 64u) put(As, (int)wave * RPW + i, col, av[i]);  // always true for a checked tile
        }
    } else {
      const int k0 = kt * 64;
      for (int i = 0; i < RPW; ++i) {
        const int row = (int)wave * RPW + i, gr = m0 + row;
        if (gr >= p.rows) break;
        const uint64_t* ci = I + (size_t)(gr / bs) * p.bcols;
        for (int pos = (int)lane; pos < p.ell_cols; pos += 64) {
          const int e = pos / bs, t = pos - e * bs;
          const uint64_t bc = ci[e];
          if (bc >= (uint64_t)p.nbc) continue;
          const int col = (int)bc * bs + t - k0;
          if (col >= 0 && col < 64) put(As, row, col, V[(size_t)gr * p.ell_cols + pos]);
        }
      }
    }
  };

  f4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

  if (nkt > 0) load_stage(0);
  for (int kt = 0; kt < nkt; ++kt) {
    char* As = smem + (kt & 1) * STAGE;
    store_stage(As, kt);
    // one barrier per stage: the buffer written next was last read two stages ago, before this barrier
    __syncthreads();
    if (kt + 1 < nkt) load_stage(kt + 1);
    const char* Bs = As + SA;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      h8 af[FM], bf[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = *reinterpret_cast<const h8*>(As + a_off(wm * TMW + i * 16 + r16, 4u * s + g));
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[j] = *reinterpret_cast<const h8*>(Bs + a_off(wn * TNW + j * 16 + r16, 4u * s + g));
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = mfma16<BF>(af[i], bf[j], acc[i][j]);
    }
  }

  // ---- epilogue: lane holds C[rows 4g .. 4g + 3][column r16] of each fragment = 4 consecutive elements of a C column
  const bool c4 = (p.rows % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & 7u) == 0);
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int gr = m0 + (int)(wm * TMW + i * 16 + 4u * g), gc = n0 + (int)(wn * TNW + j * 16 + r16);
      if (gc >= p.n || gr >= p.rows) continue;
      half_t* dst = C + (size_t)gc * p.rows + gr;
      if (p.beta == 0.0f && c4) {  // rows % 4 == 0: the piece is all in
        h4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = to_elt<BF>(p.alpha * acc[i][j][q]);
        *reinterpret_cast<h4*>(dst) = o;
        continue;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (gr + q >= p.rows) continue;
        float v = p.alpha * acc[i][j][q];
        if (p.beta != 0.0f) v += p.beta * to_f32<BF>(dst[q]);
        dst[q] = to_elt<BF>(v);
      }
    }
}

template <int TN, int WM, int WN, bool BF>
static int bell16_launch_cfg(Bell16Args& a, size_t nb, bool vec, hipStream_t st) {
  constexpr size_t STAGE2 = 2 * ((size_t)BELL16_TM * 128 + (size_t)TN * 128);
  a.tiles_n = (a.n + TN - 1) / TN;
  const size_t nbr_max = (size_t)(BELL16_TM - 1) / (size_t)a.bs + 2;
  const size_t table = round_up(nbr_max * (size_t)(a.nkt + 1) * 2, 16);
  a.table = (a.ell_cols <= 65535 && STAGE2 + table <= BELL16_LDS_MAX) ? 1 : 0;
  const size_t lds = STAGE2 + (a.table ? table : 0);
  const size_t grid = (size_t)a.tiles_m * a.tiles_n * nb;  // (bell16_validate: 0 < grid <= 2^31 - 1 for the narrowest tile, so for this one)
  const char* const who = "sm_spmm_bell16";
  if (vec) return launch_grid<&spmm_bell16_kernel<TN, WM, WN, BF, true>>(grid, 64 * BELL16_NW, BELL16_LDS_MAX, lds, st, who, "spmm_bell16_kernel", a);
  return launch_grid<&spmm_bell16_kernel<TN, WM, WN, BF, false>>(grid, 64 * BELL16_NW, BELL16_LDS_MAX, lds, st, who, "spmm_bell16_kernel", a);
}


// Argument checks, decided before any HIP call.  Returns SM_STATUS_SUCCESS with *work = false when there is nothing to do.
static int bell16_validate(const char* what, const void* const* values, const uint64_t* const* idx, size_t rows, size_t cols,
                           size_t bs, size_t ell_cols, const void* B, void* const* C, size_t n, size_t batch, bool* work) {
  *work = false;
  bool null_entry = !values || !idx || !C;
  for (size_t i = 0; !null_entry && i < batch; ++i) null_entry = !values[i] || !idx[i] || !C[i];
  if (null_entry || !B || bs == 0 || ell_cols % bs != 0) {
    set_error("%s: invalid argument", what);
    return SM_STATUS_INVALID_VALUE;
  }
  if (rows > 0x7fffffffull || cols > 0x7fffffffull || n > 0x7fffffffull || ell_cols > 0x7fffffffull) {
    set_error("%s: dimension exceeds 2^31-1", what);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (rows == 0 || n == 0 || batch == 0) return SM_STATUS_SUCCESS;
  const size_t per = batch < (size_t)BELL16_MAXB ? batch : (size_t)BELL16_MAXB;
  if (ceil_div(rows, BELL16_TM) * ceil_div(n, 64) * per > 0x7fffffffull) {  // the narrowest tile's grid
    set_error("%s: grid too large", what);
    return SM_STATUS_NOT_SUPPORTED;
  }
  *work = true;
  return SM_STATUS_SUCCESS;
}

template <bool BF>
static int bell16_run(const char* what, const void* const* values, const uint64_t* const* idx, size_t rows, size_t cols, size_t bs,
                      size_t ell_cols, const void* B, void* const* C, size_t n, size_t batch, float alpha, float beta, sm_stream_t stream) {
  bool work = false;
  if (const int rc = bell16_validate(what, values, idx, rows, cols, bs, ell_cols, B, C, n, batch, &work)) return rc;
  if (!work) return SM_STATUS_SUCCESS;
  Bell16Args a = {};
  a.B = (const half_t*)B;
  a.rows = (int)rows; a.cols = (int)cols; a.n = (int)n; a.bs = (int)(bs < 0x7fffffffull ? bs : 0x7fffffffull);
  a.ell_cols = (int)ell_cols; a.bcols = (int)(ell_cols / bs); a.nbc = (int)(cols / bs);
  a.nkt = (int)ceil_div(cols, 64);
  a.tiles_m = (int)ceil_div(rows, BELL16_TM);
  a.magic = (bs > 1 && bs < 65536) ? (unsigned)((0x100000000ull + bs - 1) / bs) : 0u;
  a.alpha = alpha; a.beta = beta;
  const bool vec = cols % 8 == 0 && (reinterpret_cast<uintptr_t>(B) & 15u) == 0;
  hipStream_t st = (hipStream_t)stream;
  for (size_t b0 = 0; b0 < batch; b0 += BELL16_MAXB) {
    const size_t nb = batch - b0 < (size_t)BELL16_MAXB ? batch - b0 : (size_t)BELL16_MAXB;
    for (size_t i = 0; i < nb; ++i) {
      a.values[i] = (const unsigned short*)values[b0 + i];
      a.idx[i] = idx[b0 + i];
      a.C[i] = (half_t*)C[b0 + i];
    }
    int rc;
    // Tile width: as wide as n (up to 256), so that each A tile is built once per 256 columns.  What binds is that build (the
    // VALU work and the memory round trip of every stage, profiles/bell16_counters.txt), not idle CUs: narrowing the tile to
    // fill the grid builds A more often and was measured slower (784 x 256 x 2304, b = 32: 0.19 -> 0.40 ms with 64-wide
    // tiles, 896 workgroups instead of 224; 196 x 512 x 4608: 0.37 -> 0.40 ms).
    if (n <= 64) rc = bell16_launch_cfg<64, 4, 2, BF>(a, nb, vec, st);
    else if (n <= 128) rc = bell16_launch_cfg<128, 4, 2, BF>(a, nb, vec, st);
    else rc = bell16_launch_cfg<256, 2, 4, BF>(a, nb, vec, st);
    if (rc != SM_STATUS_SUCCESS) return rc;
  }
  return SM_STATUS_SUCCESS;
}

}  // namespace sm

using namespace sm;

extern "C" {

int sm_spmm_bell_f16(const void* values, const uint64_t* column_indices, size_t rows, size_t cols, size_t block_size, size_t ell_cols,
                     const void* B, void* C, size_t n, float alpha, float beta, sm_stream_t stream) {
  return bell16_run<false>("sm_spmm_bell_f16", &values, &column_indices, rows, cols, block_size, ell_cols, B, &C, n, 1, alpha, beta, stream);
}
int sm_spmm_bell_bf16(const void* values, const uint64_t* column_indices, size_t rows, size_t cols, size_t block_size, size_t ell_cols,
                      const void* B, void* C, size_t n, float alpha, float beta, sm_stream_t stream) {
  return bell16_run<true>("sm_spmm_bell_bf16", &values, &column_indices, rows, cols, block_size, ell_cols, B, &C, n, 1, alpha, beta, stream);
}
int sm_spmm_bell_batched_f16(const void* const* values, const uint64_t* const* column_indices, size_t rows, size_t cols, size_t block_size,
                             size_t ell_cols, const void* B, void* const* C, size_t n, size_t batch, float alpha, float beta, sm_stream_t stream) {
  return bell16_run<false>("sm_spmm_bell_batched_f16", values, column_indices, rows, cols, block_size, ell_cols, B, C, n, batch, alpha, beta, stream);
}
int sm_spmm_bell_batched_bf16(const void* const* values, const uint64_t* const* column_indices, size_t rows, size_t cols, size_t block_size,
                              size_t ell_cols, const void* B, void* const* C, size_t n, size_t batch, float alpha, float beta, sm_stream_t stream) {
  return bell16_run<true>("sm_spmm_bell_batched_bf16", values, column_indices, rows, cols, block_size, ell_cols, B, C, n, batch, alpha, beta, stream);
}

}  // extern "C"
