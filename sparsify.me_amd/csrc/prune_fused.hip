// prune_fused.hip -- the prune / check / compress steps of sparsifyme::spmma() (reference
// include/sparsify.me/spmma.hxx:82-104: cusparseLtSpMMAPrune TILE in place, cusparseLtSpMMAPruneCheck + readback,
// cusparseLtSpMMACompress) as ONE pass over A: read the dense operand once, write the pruned operand, the compressed
// blob and the validity flag.  Bytes per element of A (s = 2): read s, write s + s/2 + 1/8 -- 2.56 s instead of the
// 2 s + s + 1.56 s of the three separate launches.  HBM-bound; the TILE rule is ~260 VALU per 4x4 tile (select24.h).
//
// Work item = 4 rows x 8 columns (two TILE tiles, or eight strips) of one batch matrix: a lane moves 16 bytes per row
// per access, lanes run along k, so a wave-instruction covers up to 1 KiB of one row; the four 8-byte value pieces of
// an item go to four consecutive blob rows of one stage plane, the item's four metadata bytes are gathered across
// the lane quad with DPP so that one lane stores a dword per row.
#include "sm_common.h"
#include "select24.h"

namespace sm {

struct PruneFusedArgs {
  const uint16_t* A_in;
  uint16_t* A_out;      // may be null (no pruned copy wanted) or alias A_in
  uint16_t* vals;       // blob values, stage-major [kc/64][M][32]; null = no blob
  unsigned char* meta;  // blob metadata [kc/64][M][8]
  int* d_valid;         // null = no flag
  size_t m, ld, strideA, M;
  unsigned rows;        // FLAT: rows of the one tall matrix (m * batch); else unused
  unsigned trows;       // tile rows per batch matrix (non-FLAT)
  unsigned gtr_total;   // tile rows in all
  unsigned ppr;         // 8-column items per row (k / 8)
  unsigned lpr_log2;    // lanes along k per tile row: the largest power of two <= 64 that divides ppr
};

// Mapping (no integer division on the FLAT path): a wave covers 64 >> lpr_log2 consecutive tile rows x LPR consecutive
// 8-column items per pass -- each row of a pass is read in whole 128-byte lines or more -- and walks the row's
// k / (8 LPR) passes before it moves to its next group of tile rows (grid-stride over waves).  The next pass's four
// 16-byte loads are issued before the current pass's selection starts.
// FLAT: the batch is one tall matrix (contiguous batches and m % 4 == 0, or batch == 1).
// BLOB = false (round 6): the prune + flag pass of the no-blob API sequence (sm_prune24_spmma_* for n > 128: vals == null) -- the blob's
// STRIP re-selection of every pruned strip (8 x 16 vector instructions per item with the TILE rule, ~11 % of the kernel's) and the metadata
// gathering are compiled out instead of computed and dropped.
template <bool BF, bool TILE, bool FLAT, bool BLOB = true>
__global__ __launch_bounds__(256) void prune_compress_kernel(const PruneFusedArgs p) {
  bool bad = false;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave_g = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
  const unsigned lg = p.lpr_log2, rw = lane >> lg, pcl = lane & ((1u << lg) - 1u), rpw = 64u >> lg;
  const unsigned nj = p.ppr >> lg;
  const unsigned ngroups = (p.gtr_total + rpw - 1u) / rpw;  // wave-uniform

  struct Pos {
    size_t aoff;      // element offset of the item's first row in A
    size_t R0;        // blob row of the item's first row
    unsigned nrows;   // valid rows of the item (0..4)
    unsigned pc;
  };
  auto locate = [&](unsigned g, unsigned j) {
    Pos q;
    const unsigned gtr = g * rpw + rw;
    q.pc = (j << lg) + pcl;
    if constexpr (FLAT) {
      const unsigned r0 = gtr * 4u;
      q.nrows = gtr < p.gtr_total ? (p.rows - r0 < 4u ? p.rows - r0 : 4u) : 0u;
      q.aoff = (size_t)r0 * p.ld + (size_t)q.pc * 8u;
      q.R0 = r0;
    } else {
      const unsigned b = gtr / p.trows, tr = gtr - b * p.trows, r0 = tr * 4u;
      const unsigned left = (unsigned)p.m - r0;
      q.nrows = gtr < p.gtr_total ? (left < 4u ? left : 4u) : 0u;
      q.aoff = (size_t)b * p.strideA + (size_t)r0 * p.ld + (size_t)q.pc * 8u;
      q.R0 = (size_t)b * p.m + r0;
    }
    return q;
  };
  auto load = [&](const Pos& q, u4 (&v)[4]) {
    const uint16_t* src = p.A_in + q.aoff;
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      v[r] = r < q.nrows ? __builtin_nontemporal_load(reinterpret_cast<const u4*>(src)) : u4{0u, 0u, 0u, 0u};
      src += p.ld;
    }
  };

  // wave-level work units u = g * nj + j, grid-stride over waves; (g, j) advance without a division per pass
  const unsigned long long units = (unsigned long long)ngroups * nj;
  if (wave_g >= units) return;
  unsigned g = wave_g / nj, j = wave_g - g * nj;
  const unsigned dg = nwaves / nj, dj = nwaves - dg * nj;
  unsigned long long u = wave_g;
  Pos cur = locate(g, j);
  u4 v[4];
  load(cur, v);
  for (;;) {
    // next pass of this wave (wave-uniform counters)
    unsigned gn = g + dg, jn = j + dj;
    if (jn >= nj) {
      jn -= nj;
      ++gn;
    }
    const bool more = u + nwaves < units;
    Pos nxt = cur;
    u4 vn[4];
    if (more) {
      nxt = locate(gn, jn);
      load(nxt, vn);
    }

    // pruned dwords o, and what sm_compress24 stores for the pruned strip: the STRIP selection of ITS values (kept
    // pair in position order + nibble).  For the STRIP rule that is the selection itself; for the TILE rule it differs
    // from the TILE positions exactly when TILE kept a zero (the blob then names the lowest-index zeros), and a blob
    // must be the bytes of compress(prune(A)).
    uint32_t o[4][4], kp[4][2], nb[4][2];
    bool ok2 = true;
    if constexpr (TILE) {
#pragma unroll
      for (unsigned t = 0; t < 2; ++t) {
        float mag[4][4];
#pragma unroll
        for (unsigned r = 0; r < 4; ++r) {
          mag2<BF>(v[r][2 * t], mag[r][0], mag[r][1]);
          mag2<BF>(v[r][2 * t + 1], mag[r][2], mag[r][3]);
        }
        unsigned top, bot;
        tile_select_pairs(mag, top, bot);
        const unsigned pr[4] = {top >> 3, top & 7u, bot >> 3, bot & 7u};
#pragma unroll
        for (unsigned r = 0; r < 4; ++r) {
          const uint32_t rm = pair_rowmask(pr[r]);
          // NOT an independent check: rm comes from pair_rowmask (always two bits), so on this path the flag is zero by
          // construction -- it can only rise if a pair index leaves 0..5 (then rm has a stray pattern).  The independent
          // inspection of written data is sm_prune24_check_* (what the three-launch fallback below runs on A_out, and what
          // tests/test_gpu_parity.py runs on this kernel's output).
          ok2 &= __builtin_popcount(rm) <= 2 && pr[r] < 6u;
          strip_mask(v[r][2 * t], v[r][2 * t + 1], rm, o[r][2 * t], o[r][2 * t + 1]);
          if constexpr (BLOB) strip_select_f16(o[r][2 * t], o[r][2 * t + 1], kp[r][t], nb[r][t]);
          else { kp[r][t] = 0; nb[r][t] = 0; }
        }
      }
    } else {
#pragma unroll
      for (unsigned r = 0; r < 4; ++r)
#pragma unroll
        for (unsigned t = 0; t < 2; ++t) {
          strip_select_f16(v[r][2 * t], v[r][2 * t + 1], kp[r][t], nb[r][t]);
          const uint32_t rm = (1u << (nb[r][t] & 3u)) | (1u << (nb[r][t] >> 2));
          ok2 &= __builtin_popcount(rm) <= 2;
          strip_mask(v[r][2 * t], v[r][2 * t + 1], rm, o[r][2 * t], o[r][2 * t + 1]);
        }
    }
    bad |= !ok2;
    const size_t stage = cur.pc >> 3;
    const unsigned q2 = cur.pc & 7u;  // byte of the row's 8 metadata bytes / 8-byte piece of its 64 value bytes
    uint16_t* dst = p.A_out ? p.A_out + cur.aoff : nullptr;
    uint16_t* vdst = (BLOB && p.vals) ? p.vals + (stage * p.M + cur.R0) * 32 + q2 * 4 : nullptr;
    unsigned char* mdst = (BLOB && p.vals) ? p.meta + (stage * p.M + cur.R0) * 8 + q2 : nullptr;
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      unsigned b0 = 0, b1 = 0, b2 = 0, b3 = 0;
      if constexpr (BLOB) {
        const int mb = (int)(nb[r][0] | (nb[r][1] << 4));
        // the four metadata bytes of a lane quad (same rows, same stage, consecutive q2) -> one dword
        b0 = (unsigned)__builtin_amdgcn_update_dpp(0, mb, 0x00, 0xf, 0xf, true);
        b1 = (unsigned)__builtin_amdgcn_update_dpp(0, mb, 0x55, 0xf, 0xf, true);
        b2 = (unsigned)__builtin_amdgcn_update_dpp(0, mb, 0xaa, 0xf, 0xf, true);
        b3 = (unsigned)__builtin_amdgcn_update_dpp(0, mb, 0xff, 0xf, 0xf, true);
      }
      if (r < cur.nrows) {
        if (dst) *reinterpret_cast<u4*>(dst) = u4{o[r][0], o[r][1], o[r][2], o[r][3]};
        if constexpr (BLOB) {
          if (vdst) {
            __builtin_nontemporal_store(u2{kp[r][0], kp[r][1]}, reinterpret_cast<u2*>(vdst + r * 32));
            if ((lane & 3u) == 0) *reinterpret_cast<unsigned*>(mdst + r * 8) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
          }
        }
      }
      if (dst) dst += p.ld;
    }
    if (!more) break;
    u += nwaves;
    g = gn;
    j = jn;
    cur = nxt;
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) v[r] = vn[r];
  }
  if (p.d_valid && __any(bad)) {
    if (lane == 0) raise_flag(p.d_valid);
  }
}


// ---------------------------------------------------------------------------------------------
// fp32 form (round 3): the type the reference's own driver instantiates (examples/spmma.cu:24 -> spmma.hxx:82-104).  Same
// work item (4 rows x 8 columns = two TILE tiles / eight strips; two 16-byte loads per row and lane), same wave mapping,
// same blob geometry with 4-byte elements (values [kc/64][M][32] floats, metadata [kc/64][M][8 B]): per item and row
// 32 bytes of pruned A, one 16-byte piece of kept values, one metadata byte (a lane quad's four bytes leave as one dword).
// The rules are the fp32 ones of prune.hip: magnitudes = bit patterns with the sign cleared (NaN -> +inf for the TILE
// sums), STRIP by compare-and-count (strip_keepmask), and the blob of a pruned strip is the STRIP selection of ITS values.
// ---------------------------------------------------------------------------------------------
struct PruneFusedArgs32 {
  const uint32_t* A_in;
  uint32_t* A_out;
  uint32_t* vals;
  unsigned char* meta;
  int* d_valid;
  size_t m, ld, strideA, M;
  unsigned rows, trows, gtr_total, ppr, lpr_log2;
};

__device__ __forceinline__ float mag_of_f32bits(uint32_t v) {
  const uint32_t k = v & 0x7fffffffu;
  return k > 0x7f800000u ? __builtin_inff() : __builtin_bit_cast(float, k);
}

template <bool TILE, bool FLAT>
__global__ __launch_bounds__(256) void prune_compress_f32_kernel(const PruneFusedArgs32 p) {
  bool bad = false;
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave_g = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
  const unsigned lg = p.lpr_log2, rw = lane >> lg, pcl = lane & ((1u << lg) - 1u), rpw = 64u >> lg;
  const unsigned nj = p.ppr >> lg;
  const unsigned ngroups = (p.gtr_total + rpw - 1u) / rpw;

  struct Pos {
    size_t aoff, R0;
    unsigned nrows, pc;
  };
  auto locate = [&](unsigned g, unsigned j) {
    Pos q;
    const unsigned gtr = g * rpw + rw;
    q.pc = (j << lg) + pcl;
    if constexpr (FLAT) {
      const unsigned r0 = gtr * 4u;
      q.nrows = gtr < p.gtr_total ? (p.rows - r0 < 4u ? p.rows - r0 : 4u) : 0u;
      q.aoff = (size_t)r0 * p.ld + (size_t)q.pc * 8u;
      q.R0 = r0;
    } else {
      const unsigned b = gtr / p.trows, tr = gtr - b * p.trows, r0 = tr * 4u;
      const unsigned left = (unsigned)p.m - r0;
      q.nrows = gtr < p.gtr_total ? (left < 4u ? left : 4u) : 0u;
      q.aoff = (size_t)b * p.strideA + (size_t)r0 * p.ld + (size_t)q.pc * 8u;
      q.R0 = (size_t)b * p.m + r0;
    }
    return q;
  };
  auto load = [&](const Pos& q, u4 (&v)[4][2]) {
    const uint32_t* src = p.A_in + q.aoff;
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      if (r < q.nrows) {
        v[r][0] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src));
        v[r][1] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src) + 1);
      } else {
        v[r][0] = v[r][1] = u4{0u, 0u, 0u, 0u};
      }
      src += p.ld;
    }
  };

  const unsigned long long units = (unsigned long long)ngroups * nj;
  if (wave_g >= units) return;
  unsigned g = wave_g / nj, j = wave_g - g * nj;
  const unsigned dg = nwaves / nj, dj = nwaves - dg * nj;
  unsigned long long u = wave_g;
  Pos cur = locate(g, j);
  u4 v[4][2];
  load(cur, v);
  for (;;) {
    unsigned gn = g + dg, jn = j + dj;
    if (jn >= nj) {
      jn -= nj;
      ++gn;
    }
    const bool more = u + nwaves < units;
    Pos nxt = cur;
    u4 vn[4][2];
    if (more) {
      nxt = locate(gn, jn);
      load(nxt, vn);
    }

    unsigned keep[2] = {0u, 0u};  // 16-bit keep masks (bit 4 r + c) of the item's two tiles
    if constexpr (TILE) {
#pragma unroll
      for (unsigned t = 0; t < 2; ++t) {
        float mag[4][4];
#pragma unroll
        for (unsigned r = 0; r < 4; ++r)
#pragma unroll
          for (unsigned c = 0; c < 4; ++c) mag[r][c] = mag_of_f32bits(v[r][t][c]);
        keep[t] = tile_keepmask(mag);
        __builtin_amdgcn_sched_barrier(0);  // one tile after the other (registers)
      }
    } else {
#pragma unroll
      for (unsigned t = 0; t < 2; ++t)
#pragma unroll
        for (unsigned r = 0; r < 4; ++r)
          keep[t] |= strip_keepmask(key_of(v[r][t][0]), key_of(v[r][t][1]), key_of(v[r][t][2]), key_of(v[r][t][3])) << (4u * r);
    }
    const size_t stage = cur.pc >> 3;
    const unsigned q2 = cur.pc & 7u;
    uint32_t* dst = p.A_out ? p.A_out + cur.aoff : nullptr;
    uint32_t* vdst = p.vals ? p.vals + (stage * p.M + cur.R0) * 32 + q2 * 4 : nullptr;
    unsigned char* mdst = p.vals ? p.meta + (stage * p.M + cur.R0) * 8 + q2 : nullptr;
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      uint32_t o[2][4], kv[4];
      unsigned nb[2];
#pragma unroll
      for (unsigned t = 0; t < 2; ++t) {
        const unsigned rm = (keep[t] >> (4u * r)) & 15u;
#pragma unroll
        for (unsigned c = 0; c < 4; ++c) o[t][c] = ((rm >> c) & 1u) ? v[r][t][c] : 0u;
        // the flag is derived from the VALUES about to be stored, as sm_prune24_check_f32 derives it from the stored matrix
        // (more than two of a strip's four != 0; -0 counts as zero) -- not from the keep mask, which has two bits by construction
        bad |= ((key_of(o[t][0]) != 0u) + (key_of(o[t][1]) != 0u) + (key_of(o[t][2]) != 0u) + (key_of(o[t][3]) != 0u)) > 2;
        // what sm_compress24_f32 stores for the pruned strip: the STRIP selection of ITS values (== rm unless a zero was kept)
        const unsigned ks = strip_keepmask(key_of(o[t][0]), key_of(o[t][1]), key_of(o[t][2]), key_of(o[t][3]));
        nb[t] = nibble_of(ks);
        const unsigned p0 = nb[t] & 3u, p1 = nb[t] >> 2;
        uint32_t a0 = o[t][0], a1 = o[t][1];
        a0 = p0 == 1 ? o[t][1] : a0;
        a0 = p0 == 2 ? o[t][2] : a0;
        a1 = p1 == 2 ? o[t][2] : a1;
        a1 = p1 == 3 ? o[t][3] : a1;
        kv[2 * t] = a0;
        kv[2 * t + 1] = a1;
      }
      const int mb = (int)(nb[0] | (nb[1] << 4));
      const unsigned b0 = (unsigned)__builtin_amdgcn_update_dpp(0, mb, 0x00, 0xf, 0xf, true);
      const unsigned b1 = (unsigned)__builtin_amdgcn_update_dpp(0, mb, 0x55, 0xf, 0xf, true);
      const unsigned b2 = (unsigned)__builtin_amdgcn_update_dpp(0, mb, 0xaa, 0xf, 0xf, true);
      const unsigned b3 = (unsigned)__builtin_amdgcn_update_dpp(0, mb, 0xff, 0xf, 0xf, true);
      if (r < cur.nrows) {
        if (dst) {
          reinterpret_cast<u4*>(dst)[0] = u4{o[0][0], o[0][1], o[0][2], o[0][3]};
          reinterpret_cast<u4*>(dst)[1] = u4{o[1][0], o[1][1], o[1][2], o[1][3]};
        }
        if (vdst) {
          __builtin_nontemporal_store(u4{kv[0], kv[1], kv[2], kv[3]}, reinterpret_cast<u4*>(vdst + r * 32));
          if ((lane & 3u) == 0) *reinterpret_cast<unsigned*>(mdst + r * 8) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
        }
      }
      if (dst) dst += p.ld;
    }
    if (!more) break;
    u += nwaves;
    g = gn;
    j = jn;
    cur = nxt;
#pragma unroll
    for (unsigned r = 0; r < 4; ++r) {
      v[r][0] = vn[r][0];
      v[r][1] = vn[r][1];
    }
  }
  if (p.d_valid && __any(bad)) {
    if (lane == 0) raise_flag(p.d_valid);
  }
}

}  // namespace sm

using namespace sm;

// prune.hip
extern "C" int sm_prune24_f16(const void*, void*, size_t, size_t, size_t, int, sm_stream_t);
extern "C" int sm_prune24_bf16(const void*, void*, size_t, size_t, size_t, int, sm_stream_t);
namespace sm {
int prune_check_accumulate_u16(const void* A, size_t m, size_t k, size_t ld, int* d_valid, hipStream_t st);  // ORs into *d_valid
// prune.hip (round 6): TILE prune of one contiguous 16-bit matrix with ragged rows through LDS spans, the flag raised in the same pass
int prune24_tile_span_u16(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, bool bf, int* d_valid, hipStream_t st);
}
extern "C" int sm_compress24_f16(const void*, size_t, size_t, size_t, size_t, size_t, void*, sm_stream_t);

namespace sm {
unsigned prune24_span_rows(const void* A_in, const void* A_out, size_t m, size_t k, size_t ld);  // prune.hip: 0 = the span form does not take it
}

// ---------------------------------------------------------------------------------------------
// THE DISPATCH RULE of sm_prune24_compress24_{f16,bf16,f32} -- ONE pure host function of the call's sizes, strides, element size, alg,
// pointer VALUES (never dereferenced; blob / A_out: null or not, and their alignment) and the CU count: the entry points switch on its
// answer, sm_prune24_compress24_form exports it.
// ---------------------------------------------------------------------------------------------
struct OnePassPick {
  int form;  // SM_PRUNE24_COMPRESS24_FORM_*
  // the one-pass kernel's launch (forms _ONEPASS_*)
  bool flat;      // FLAT instantiation: the batch is one tall matrix (contiguous batches and m % 4 == 0, or batch == 1)
  unsigned rows, trows, gtr_total, ppr, lpr_log2, nj, grid;
  bool capped;    // the grid was cut to 8 blocks per CU
  // the three-launch fallback (forms _FALLBACK_*)
  size_t nbm, fb_rows;  // matrices the prune / check loops run over, rows of each
};
static OnePassPick prune_compress24_form(size_t elt, const void* A_in, const void* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                                         const void* blob, int alg, size_t cus /*0: this device's*/) {
  OnePassPick p = {};
  if (!A_in || ld < k || (alg != SM_PRUNE_STRIP && alg != SM_PRUNE_TILE) || (blob && !aligned16(blob))) {
    p.form = SM_PRUNE24_COMPRESS24_FORM_INVALID;
    return p;
  }
  if (m == 0 || k == 0 || batch == 0) {
    p.form = SM_PRUNE24_COMPRESS24_FORM_EMPTY;
    return p;
  }
  const size_t per16 = 16 / elt;
  const bool fast = k % 64 == 0 && ld % per16 == 0 && strideA % per16 == 0 && aligned16(A_in) && (!A_out || aligned16(A_out)) &&
                    batch * ceil_div(m, (size_t)4) < 0x3fffffffull && k / 8 < 0xffffffffull && m * batch < 0xfffffff0ull;
  if (!fast) {
    // shapes the one-pass kernel does not take (k % 64 != 0: the 7x7x3 stem layer; unaligned rows): the same three
    // steps as separate launches, per batch matrix (a TILE never straddles two matrices)
    if (!A_out && alg == SM_PRUNE_TILE && blob) {
      p.form = SM_PRUNE24_COMPRESS24_FORM_NOT_SUPPORTED;
      return p;
    }
    // the batch as one tall matrix when its matrices are back to back and no TILE can straddle two of them
    const bool tall = batch == 1 || (strideA == m * ld && (alg == SM_PRUNE_STRIP || m % 4 == 0));
    p.nbm = tall ? 1 : batch;
    p.fb_rows = tall ? m * batch : m;
    // (round 6) TILE on one contiguous 16-bit matrix with ragged rows (the stem layer, k = 147): the span form prunes AND raises the flag in
    // one pass -- no separate check pass (the flag is derived from the stored values, as the one-pass kernel derives it)
    if (elt == 2 && A_out && alg == SM_PRUNE_TILE && tall && prune24_span_rows(A_in, A_out, p.fb_rows, k, ld)) p.form = SM_PRUNE24_COMPRESS24_FORM_FALLBACK_TALL_SPAN;
    else p.form = tall ? SM_PRUNE24_COMPRESS24_FORM_FALLBACK_TALL : SM_PRUNE24_COMPRESS24_FORM_FALLBACK_PER_BATCH;
    return p;
  }
  // 16-bit TILE without a blob: the prune + flag pass alone, the blob's re-selection compiled out (the fp32 kernel has no such instantiation)
  p.form = alg == SM_PRUNE_STRIP ? SM_PRUNE24_COMPRESS24_FORM_ONEPASS_STRIP
                                 : (elt == 2 && !blob ? SM_PRUNE24_COMPRESS24_FORM_ONEPASS_TILE_NOBLOB : SM_PRUNE24_COMPRESS24_FORM_ONEPASS_TILE);
  p.flat = batch == 1 || (strideA == m * ld && m % 4 == 0);
  p.rows = (unsigned)(p.flat ? m * batch : 0);
  p.trows = (unsigned)ceil_div(m, (size_t)4);
  p.gtr_total = (unsigned)(p.flat ? ceil_div(m * batch, (size_t)4) : batch * p.trows);
  p.ppr = (unsigned)(k / 8);
  p.lpr_log2 = 3;  // k % 64 == 0: ppr is a multiple of 8
  while (p.lpr_log2 < 6 && p.ppr % (2u << p.lpr_log2) == 0) ++p.lpr_log2;
  p.nj = p.ppr >> p.lpr_log2;
  const size_t wave_units = ceil_div((size_t)p.gtr_total, (size_t)(64u >> p.lpr_log2));
  size_t blocks = ceil_div(wave_units, (size_t)4);
  const size_t cap = (cus ? cus : (size_t)device_cu_count()) * 8;  // 2 blocks per SIMD: the kernel holds ~3 waves per SIMD
  p.capped = blocks > cap;
  if (p.capped) blocks = cap;
  p.grid = (unsigned)(blocks ? blocks : 1);
  return p;
}

template <bool BF>
static int prune_compress16(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                            void* blob, int* d_valid, int alg, sm_stream_t stream) {
  const char* name = BF ? "sm_prune24_compress24_bf16" : "sm_prune24_compress24_f16";
  const OnePassPick pick = prune_compress24_form(2, A_in, A_out, m, k, ld, batch, strideA, blob, alg, 0);
  if (pick.form == SM_PRUNE24_COMPRESS24_FORM_INVALID) {
    set_error("%s: invalid argument", name);
    return SM_STATUS_INVALID_VALUE;
  }
  if (pick.form == SM_PRUNE24_COMPRESS24_FORM_NOT_SUPPORTED) {  // decided before anything is touched, the flag word included
    set_error("%s: TILE + blob without A_out needs k %% 64 == 0 and 16-byte aligned rows", name);
    return SM_STATUS_NOT_SUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  if (d_valid && hipMemsetAsync(d_valid, 0, sizeof(int), st) != hipSuccess) return check_launch("hipMemsetAsync(d_valid)");
  switch (pick.form) {
    case SM_PRUNE24_COMPRESS24_FORM_EMPTY:
      return SM_STATUS_SUCCESS;
    case SM_PRUNE24_COMPRESS24_FORM_FALLBACK_TALL_SPAN:
    case SM_PRUNE24_COMPRESS24_FORM_FALLBACK_TALL:
    case SM_PRUNE24_COMPRESS24_FORM_FALLBACK_PER_BATCH: {
      int rc = SM_STATUS_SUCCESS;
      const void* src = A_in;
      const size_t nbm = pick.nbm, rows = pick.fb_rows;
      bool flag_done = false;
      if (A_out) {
        if (pick.form == SM_PRUNE24_COMPRESS24_FORM_FALLBACK_TALL_SPAN) {
          rc = prune24_tile_span_u16(A_in, A_out, rows, k, ld, BF, d_valid, st);
          flag_done = true;
        } else {
          for (size_t b = 0; b < nbm && rc == SM_STATUS_SUCCESS; ++b) {
            const uint16_t* ai = (const uint16_t*)A_in + b * strideA;
            uint16_t* ao = (uint16_t*)A_out + b * strideA;
            rc = BF ? sm_prune24_bf16(ai, ao, rows, k, ld, alg, stream) : sm_prune24_f16(ai, ao, rows, k, ld, alg, stream);
          }
        }
        src = A_out;
      }
      if (rc == SM_STATUS_SUCCESS && d_valid && A_out && !flag_done) {
        // the flag of every batch matrix is OR-ed into *d_valid (zeroed above)
        for (size_t b = 0; b < nbm && rc == SM_STATUS_SUCCESS; ++b)
          rc = prune_check_accumulate_u16((const uint16_t*)A_out + b * strideA, rows, k, ld, d_valid, st);
      }
      if (rc == SM_STATUS_SUCCESS && blob) rc = sm_compress24_f16(src, m, k, ld, batch, strideA, blob, stream);
      return rc;
    }
    default:
      break;
  }
  const BlobLayout L = blob_layout(m, k, 2, batch);
  if (blob) {  // zero the alignment gaps so a blob is a pure function of its input (as sm_compress24_*)
    const size_t vbytes = L.M * (L.kc / 2) * 2, mbytes = L.M * (L.kc / 8);
    if (L.meta_off > vbytes && hipMemsetAsync((char*)blob + vbytes, 0, L.meta_off - vbytes, st) != hipSuccess)
      return check_launch("hipMemsetAsync");
    if (L.total > L.meta_off + mbytes &&
        hipMemsetAsync((char*)blob + L.meta_off + mbytes, 0, L.total - L.meta_off - mbytes, st) != hipSuccess)
      return check_launch("hipMemsetAsync");
  }
  PruneFusedArgs a = {};
  a.A_in = (const uint16_t*)A_in;
  a.A_out = (uint16_t*)A_out;
  a.vals = (uint16_t*)blob;
  a.meta = blob ? (unsigned char*)blob + L.meta_off : nullptr;
  a.d_valid = d_valid;
  a.m = m; a.ld = ld; a.strideA = strideA; a.M = L.M;
  a.rows = pick.rows; a.trows = pick.trows; a.gtr_total = pick.gtr_total; a.ppr = pick.ppr; a.lpr_log2 = pick.lpr_log2;
  const unsigned grid = pick.grid;
  const bool flat = pick.flat;
  switch (pick.form) {
    case SM_PRUNE24_COMPRESS24_FORM_ONEPASS_TILE_NOBLOB:
      if (flat) prune_compress_kernel<BF, true, true, false><<<grid, 256, 0, st>>>(a);
      else prune_compress_kernel<BF, true, false, false><<<grid, 256, 0, st>>>(a);
      break;
    case SM_PRUNE24_COMPRESS24_FORM_ONEPASS_TILE:
      if (flat) prune_compress_kernel<BF, true, true><<<grid, 256, 0, st>>>(a);
      else prune_compress_kernel<BF, true, false><<<grid, 256, 0, st>>>(a);
      break;
    default:
      if (flat) prune_compress_kernel<BF, false, true><<<grid, 256, 0, st>>>(a);
      else prune_compress_kernel<BF, false, false><<<grid, 256, 0, st>>>(a);
      break;
  }
  return check_launch("prune_compress_kernel");
}

extern "C" int sm_prune24_compress24_f16(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                                         void* blob, int* d_valid, int alg, sm_stream_t stream) {
  return prune_compress16<false>(A_in, A_out, m, k, ld, batch, strideA, blob, d_valid, alg, stream);
}
extern "C" int sm_prune24_compress24_bf16(const void* A_in, void* A_out, size_t m, size_t k, size_t ld, size_t batch,
                                          size_t strideA, void* blob, int* d_valid, int alg, sm_stream_t stream) {
  return prune_compress16<true>(A_in, A_out, m, k, ld, batch, strideA, blob, d_valid, alg, stream);
}

// prune.hip
extern "C" int sm_prune24_f32(const float*, float*, size_t, size_t, size_t, int, sm_stream_t);
extern "C" int sm_compress24_f32(const float*, size_t, size_t, size_t, size_t, size_t, void*, sm_stream_t);
namespace sm {
int prune_check_accumulate_u32(const void* A, size_t m, size_t k, size_t ld, int* d_valid, hipStream_t st);  // ORs into *d_valid
}

extern "C" int sm_prune24_compress24_f32(const float* A_in, float* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA,
                                         void* blob, int* d_valid, int alg, sm_stream_t stream) {
  const char* name = "sm_prune24_compress24_f32";
  const OnePassPick pick = prune_compress24_form(4, A_in, A_out, m, k, ld, batch, strideA, blob, alg, 0);
  if (pick.form == SM_PRUNE24_COMPRESS24_FORM_INVALID) {
    set_error("%s: invalid argument", name);
    return SM_STATUS_INVALID_VALUE;
  }
  if (pick.form == SM_PRUNE24_COMPRESS24_FORM_NOT_SUPPORTED) {  // decided before anything is touched, the flag word included
    set_error("%s: TILE + blob without A_out needs k %% 64 == 0 and 16-byte aligned rows", name);
    return SM_STATUS_NOT_SUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  if (d_valid && hipMemsetAsync(d_valid, 0, sizeof(int), st) != hipSuccess) return check_launch("hipMemsetAsync(d_valid)");
  switch (pick.form) {
    case SM_PRUNE24_COMPRESS24_FORM_EMPTY:
      return SM_STATUS_SUCCESS;
    case SM_PRUNE24_COMPRESS24_FORM_FALLBACK_TALL:
    case SM_PRUNE24_COMPRESS24_FORM_FALLBACK_PER_BATCH: {  // the same three steps as separate launches (k % 64 != 0, unaligned rows)
      int rc = SM_STATUS_SUCCESS;
      const float* src = A_in;
      const size_t nbm = pick.nbm, rows = pick.fb_rows;
      if (A_out) {
        for (size_t b = 0; b < nbm && rc == SM_STATUS_SUCCESS; ++b) rc = sm_prune24_f32(A_in + b * strideA, A_out + b * strideA, rows, k, ld, alg, stream);
        src = A_out;
      }
      if (rc == SM_STATUS_SUCCESS && d_valid && A_out)
        for (size_t b = 0; b < nbm && rc == SM_STATUS_SUCCESS; ++b) rc = prune_check_accumulate_u32(A_out + b * strideA, rows, k, ld, d_valid, st);
      if (rc == SM_STATUS_SUCCESS && blob) rc = sm_compress24_f32(src, m, k, ld, batch, strideA, blob, stream);
      return rc;
    }
    default:
      break;
  }
  const BlobLayout L = blob_layout(m, k, 4, batch);
  if (blob) {
    const size_t vbytes = L.M * (L.kc / 2) * 4, mbytes = L.M * (L.kc / 8);
    if (L.meta_off > vbytes && hipMemsetAsync((char*)blob + vbytes, 0, L.meta_off - vbytes, st) != hipSuccess) return check_launch("hipMemsetAsync");
    if (L.total > L.meta_off + mbytes && hipMemsetAsync((char*)blob + L.meta_off + mbytes, 0, L.total - L.meta_off - mbytes, st) != hipSuccess)
      return check_launch("hipMemsetAsync");
  }
  PruneFusedArgs32 a = {};
  a.A_in = (const uint32_t*)A_in;
  a.A_out = (uint32_t*)A_out;
  a.vals = (uint32_t*)blob;
  a.meta = blob ? (unsigned char*)blob + L.meta_off : nullptr;
  a.d_valid = d_valid;
  a.m = m; a.ld = ld; a.strideA = strideA; a.M = L.M;
  a.rows = pick.rows; a.trows = pick.trows; a.gtr_total = pick.gtr_total; a.ppr = pick.ppr; a.lpr_log2 = pick.lpr_log2;
  const unsigned grid = pick.grid;
  if (pick.form == SM_PRUNE24_COMPRESS24_FORM_ONEPASS_TILE) {
    if (pick.flat) prune_compress_f32_kernel<true, true><<<grid, 256, 0, st>>>(a);
    else prune_compress_f32_kernel<true, false><<<grid, 256, 0, st>>>(a);
  } else {
    if (pick.flat) prune_compress_f32_kernel<false, true><<<grid, 256, 0, st>>>(a);
    else prune_compress_f32_kernel<false, false><<<grid, 256, 0, st>>>(a);
  }
  return check_launch("prune_compress_f32_kernel");
}

extern "C" int sm_prune24_compress24_form(const void* A_in, const void* A_out, size_t m, size_t k, size_t ld, size_t batch, size_t strideA, const void* blob,
                                          size_t elt_bytes, int alg, size_t cus, int* form, unsigned* plan) {
  if (!form || (elt_bytes != 2 && elt_bytes != 4)) {
    set_error("sm_prune24_compress24_form: invalid argument (form == NULL or elt_bytes not 2 or 4)");
    return SM_STATUS_INVALID_VALUE;
  }
  const OnePassPick p = prune_compress24_form(elt_bytes, A_in, A_out, m, k, ld, batch, strideA, blob, alg, cus);
  *form = p.form;
  if (plan) {
    const bool one = p.form >= SM_PRUNE24_COMPRESS24_FORM_ONEPASS_TILE;
    plan[0] = one ? (p.flat ? 1u : 0u) : 0u;
    plan[1] = one ? p.lpr_log2 : 0u;
    plan[2] = one ? p.nj : 0u;
    plan[3] = one ? p.grid : 0u;
    plan[4] = one ? (p.capped ? 1u : 0u) : 0u;
    plan[5] = one ? 0u : (unsigned)(p.nbm > 0xffffffffull ? 0xffffffffull : p.nbm);
  }
  return SM_STATUS_SUCCESS;
}
