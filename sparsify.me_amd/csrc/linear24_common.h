// linear24_common.h -- the core of the token-major 2:4 linear layer, shared by its two operand front ends: linear24_f16.hip
// (sm_linear24_{f16,bf16}, 64 dense k per stage) and linear24_fp8.hip (sm_linear24_fp8, 128).  The front ends keep what depends on
// the operand type -- the stage layout, the K loops, the matrix instruction; everything else is here, once: the dispatch rule, the
// argument checks (linear24_args, one function for plain, gated, grouped and gathered calls), the X-image swizzle, the fragment
// epilogue and store, the decode form's combine, the tile launcher (launch_linear24_tile, plain or GROUPED) -- and what the grouped
// (per-expert) entry points add: their rule, the slot bound, the workgroup's view of its expert.
#pragma once
#include "spmma_args.h"

namespace sm {

// the largest `tokens` the decode form takes (the table it is read from) ...
constexpr size_t LINEAR24_DECODE_MAX = 16;
// ... and the largest `out`: above it (more than 4 sixteen-row workgroups per CU) the 64 x 64 tile form is the faster weight stream
// at every token count (profiles/linear_table.txt: out = 22016 and 28672 against out <= 12288)
constexpr size_t LINEAR24_DECODE_MAX_OUT = 16384;

// The dispatch rule, stated once: both layers switch on it, sm_linear24_fp8_form exports it.  Tiles: the largest of 128 x 128,
// 128 x 64 and 64 x 64 that still gives each of `cus` compute units a workgroup (fewer, larger tiles re-read X and the blob less).
inline int linear24_form(size_t tokens, size_t out, size_t in, size_t cus) {
  if (in % 64 != 0 || tokens > 0x7fffffffull || out > 0x7fffffffull || in > 0x7fffffffull) return SM_LINEAR24_FORM_NOT_TAKEN;
  if (tokens == 0 || out == 0) return SM_LINEAR24_FORM_EMPTY;
  if (tokens <= LINEAR24_DECODE_MAX && out <= LINEAR24_DECODE_MAX_OUT) return SM_LINEAR24_FORM_DECODE;
  const size_t t128 = ceil_div(out, 128) * ceil_div(tokens, 128), t64 = ceil_div(out, 128) * ceil_div(tokens, 64);
  if (tokens > 64 && t128 >= cus) return t128 > 0x7fffffffull ? SM_LINEAR24_FORM_NOT_TAKEN : SM_LINEAR24_FORM_TILE128;  // (the grid limit)
  if (t64 >= cus) return t64 > 0x7fffffffull ? SM_LINEAR24_FORM_NOT_TAKEN : SM_LINEAR24_FORM_TILE128x64;
  return ceil_div(out, 64) * ceil_div(tokens, 64) > 0x7fffffffull ? SM_LINEAR24_FORM_NOT_TAKEN : SM_LINEAR24_FORM_TILE64;
}

// The gated (gate/up) layer's rule is BY DEFINITION the plain rule on the fused weight's 2 * hidden rows (a tile of BM blob rows is
// BM / 2 hidden features: the workgroup counts are the plain rule's), plus the limit that keeps 2 * hidden a 31-bit row count.  The
// decode limits are carried over by weight bytes; nobody has measured them for the gated kernels.
constexpr size_t LINEAR24_GLU_MAX_HIDDEN = 0x3fffffffull;
inline int linear24_glu_form(size_t tokens, size_t hidden, size_t in, size_t cus) {
  if (hidden > LINEAR24_GLU_MAX_HIDDEN) return SM_LINEAR24_FORM_NOT_TAKEN;
  return linear24_form(tokens, 2 * hidden, in, cus);
}

// ---- the grouped layers (sm_linear24_grouped_*): `groups` experts of one shape, tokens sorted by expert, ONE launch ------------------
// The largest group count a call takes: the device-side walk over group_offsets is one load per group (linear24_group_view).
constexpr size_t LINEAR24_MAX_GROUPS = SM_LINEAR24_MAX_GROUPS;

// Token-tile slots of a grouped launch: min(tokens, ceil(tokens / BN) + groups - 1), an upper bound on sum_g ceil(c_g / BN) for every
// distribution of at most `tokens` tokens over the groups.  Proof: a non-empty group has ceil(c / BN) = floor((c - 1) / BN) + 1, so
// with n non-empty groups the sum is <= floor((T - n) / BN) + n <= floor((T - 1) / BN) + n <= ceil(T / BN) + groups - 1 (T = sum c_g
// <= tokens); and ceil(c / BN) <= c gives the other term.  The counts live on the device: the grid is sized by the bound, and a slot
// beyond the last real tile returns at once.
inline size_t linear24_grouped_slots(size_t tokens, size_t groups, size_t bn) {
  const size_t s = ceil_div(tokens, bn) + groups - 1;
  return s < tokens ? s : tokens;
}

// The grouped rule, stated once: both grouped layers switch on it, sm_linear24_grouped_form exports it.  It is the plain tile rule
// with the MEAN group size ceil(tokens / groups) deciding whether a 128-token tile is worth having, and never the decode form (no
// grouped decode kernel: DESIGN.md 8).  The thresholds are the plain rule's, carried over, not measured.  out: rows of ONE expert.
// The grid limit is read on tiles_m * slots, the grid the launcher asks for.
inline int linear24_grouped_form(size_t tokens, size_t groups, size_t out, size_t in, size_t cus) {
  if (in % 64 != 0 || tokens > 0x7fffffffull || out > 0x7fffffffull || in > 0x7fffffffull) return SM_LINEAR24_FORM_NOT_TAKEN;
  if (groups > LINEAR24_MAX_GROUPS || (groups != 0 && out > 0x7fffffffull / groups)) return SM_LINEAR24_FORM_NOT_TAKEN;
  if (tokens == 0 || out == 0 || groups == 0) return SM_LINEAR24_FORM_EMPTY;
  const size_t mean = ceil_div(tokens, groups);
  const size_t t128 = ceil_div(out, 128) * ceil_div(tokens, 128), t64 = ceil_div(out, 128) * ceil_div(tokens, 64);
  auto grid = [&](size_t bm, size_t bn, int form) {
    return ceil_div(out, bm) * linear24_grouped_slots(tokens, groups, bn) > 0x7fffffffull ? SM_LINEAR24_FORM_NOT_TAKEN : form;
  };
  if (mean > 64 && t128 >= cus) return grid(128, 128, SM_LINEAR24_FORM_TILE128);
  if (t64 >= cus) return grid(128, 64, SM_LINEAR24_FORM_TILE128x64);
  return grid(64, 64, SM_LINEAR24_FORM_TILE64);
}

// ... and the gated one: BY DEFINITION the grouped rule on 2 * hidden rows per expert; hidden <= 0x3fffffff / groups is its
// groups * rows <= 2^31 - 1 read on hidden.
inline int linear24_grouped_glu_form(size_t tokens, size_t groups, size_t hidden, size_t in, size_t cus) {
  if (hidden > LINEAR24_GLU_MAX_HIDDEN) return SM_LINEAR24_FORM_NOT_TAKEN;
  return linear24_grouped_form(tokens, groups, 2 * hidden, in, cus);
}

// What a grouped entry point adds to the argument checks below: the offsets (device) and the group count; and a gathered one
// (sm_linear24_grouped_*gather_*) the row index of X (device) and X's row count.
struct Linear24Groups {
  const int* offsets;
  size_t groups;
  bool gather;         // x_index / x_rows are read (and checked) only when set
  const int* x_index;  // tokens values, device
  size_t x_rows;
};

// What the shared pieces read of a launch; each front end's argument block adds its X and its K extent.
struct Linear24Core {
  const char* vals;  // the blob's values, plane-major
  const char* meta;  // the blob's metadata, plane-major [in/64][out][8 B]
  void* Y;
  const float* w_scale;  // per out feature, or null (the 16-bit layer has no scales: both null, never read)
  const float* x_scale;  // per token, or null
  size_t ldx, ldy;   // elements
  float alpha, beta;  // (in front of the ints: the compiler reads alpha's splat as one 16-byte load, which must not reach a pointer)
  int out, tokens;   // out: the width of Y.  The gated kernels (GLU) read it as `hidden`: their blob has 2 * out rows
  int tiles_m, tiles_n;
  int packed;        // Y (and R, when read) take four-element pieces: aligned to four elements, out % 4 == 0, ldy % 4 == 0
  EpiArgs e;         // bias_dim in Y's coordinates (SM_BIAS_COL: per out feature); R has Y's shape, type and ldy (R = Y when none was given)
                     // the gated kernels: bias = 2 * hidden values (gate's, then up's) or null, act = SM_GLU_ACT_*, nothing else read
};

// What follows the product, as an entry point states it: alpha, beta and the epilogue of a plain one; of a gated one (alpha = 1,
// beta = 0, no epilogue struct) the activation and the bias.
struct Linear24Tail {
  float alpha, beta;
  const sm_epilogue_t* ep;
  int act;            // SM_GLU_ACT_*
  const float* bias;  // 2 * hidden values (gate's, then up's) or null
};
inline Linear24Tail linear24_glu_tail(int act, const float* bias) { return Linear24Tail{1.0f, 0.0f, nullptr, act, bias}; }

// The entry points' argument checks, in their order and with their statuses, and the fields of Linear24Core they settle.  `who`
// names the entry point in every message; extra_ok / extra: checks of the entry point's own that belong to the second test, and
// their words in its message.  x_elt: bytes of an element of X (the blob's element too); piece: bytes of four elements of Y.
// *run = false with SM_STATUS_SUCCESS: an empty problem, nothing to launch.  grp (the grouped entry points, else null): `out` is then
// ONE expert's row count and the blob that of the stacked weight; the checks gain the offsets, the group limit and groups * rows.
// glu (sm_linear24_*glu_*), in the order include/sparsifyme.h states: the activation first where a plain call checks its epilogue, then
// the plain layer's list read on out = `hidden`; the blob is that of W[2 * hidden][in], so hidden <= LINEAR24_GLU_MAX_HIDDEN.
inline int linear24_args(Linear24Core& a, bool* run, bool glu, const char* who, bool extra_ok, const char* extra, const void* blob, const void* X, void* Y,
                         size_t tokens, size_t out, size_t in, size_t ldx, size_t ldy, size_t x_elt, size_t piece, const Linear24Tail& t,
                         const Linear24Groups* grp) {
  *run = false;
  const size_t max_out = glu ? LINEAR24_GLU_MAX_HIDDEN : 0x7fffffffull;
  if (glu) {
    if (t.act != SM_GLU_ACT_NONE && t.act != SM_GLU_ACT_RELU && t.act != SM_GLU_ACT_SILU) {
      set_error("%s: invalid argument (act is not SM_GLU_ACT_*)", who);
      return SM_STATUS_INVALID_VALUE;
    }
    a.e = EpiArgs{t.bias, (const half_t*)Y, 0, SM_BIAS_COL, t.act, 0.0f, 1};
  } else {
    bool plain;  // (not used: a plain epilogue takes the same kernels, whose bias / activation steps are skipped at run time)
    if (const int rc = epilogue_args(t.ep, Y, 0, out, t.beta, a.e, &plain, who)) return rc;
  }
  if (!blob || !X || !Y || !aligned16(blob) || !extra_ok || ldx < in || ldy < out || (grp && !grp->offsets) ||
      (grp && grp->gather && (!grp->x_index || grp->x_rows == 0))) {
    set_error("%s: invalid argument (null operand, blob not 16-byte aligned, %s%sldx < in_features or ldy < %s)", who,
              !grp ? "" : (grp->gather ? "null group_offsets, null x_index, x_rows == 0, " : "null group_offsets, "), extra, glu ? "hidden" : "out_features");
    return SM_STATUS_INVALID_VALUE;
  }
  if (tokens > 0x7fffffffull || out > max_out || in > 0x7fffffffull || (grp && grp->gather && grp->x_rows > 0x7fffffffull)) {
    set_error("%s: dimension exceeds 2^31-1%s", who, glu ? " (tokens, in_features, 2 * hidden)" : "");
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (grp && (grp->groups > LINEAR24_MAX_GROUPS || (grp->groups != 0 && out > max_out / grp->groups))) {
    set_error("%s: groups exceeds SM_LINEAR24_MAX_GROUPS or groups * %s exceeds 2^31-1", who, glu ? "2 * hidden" : "out_features");
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (in % 64 != 0 || !aligned16(X) || ldx % (16 / x_elt) != 0) {
    set_error("%s: in_features %% 64 == 0 and 16-byte aligned rows of X (pointer, ldx %% %d) are required", who, (int)(16 / x_elt));
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (tokens == 0 || out == 0 || (grp && grp->groups == 0)) return SM_STATUS_SUCCESS;
  a.vals = (const char*)blob;
  a.meta = (const char*)blob + blob_layout(glu ? 2 * out : out, in, x_elt, grp ? grp->groups : 1).meta_off;
  a.Y = Y;
  a.ldx = ldx; a.ldy = ldy;
  a.out = (int)out; a.tokens = (int)tokens;
  a.alpha = t.alpha; a.beta = t.beta;
  const bool r_ok = t.beta == 0.0f || (reinterpret_cast<uintptr_t>(a.e.R) & (piece - 1)) == 0;
  a.packed = (out % 4 == 0 && ldy % 4 == 0 && (reinterpret_cast<uintptr_t>(Y) & (piece - 1)) == 0 && r_ok) ? 1 : 0;
  *run = true;
  return SM_STATUS_SUCCESS;
}

// The rule an entry point switches on, by its kind (groups: read by the grouped kinds only)
template <bool GLU, bool GROUPED>
inline int linear24_rule(size_t tokens, size_t groups, size_t out, size_t in, size_t cus) {
  if constexpr (GROUPED) return GLU ? linear24_grouped_glu_form(tokens, groups, out, in, cus) : linear24_grouped_form(tokens, groups, out, in, cus);
  else return GLU ? linear24_glu_form(tokens, out, in, cus) : linear24_form(tokens, out, in, cus);
}

// The argument block of a GROUPED tile kernel: the front end's own block + the offsets.  The plain instantiations keep taking the
// front end's block itself, so their code is what it was.  x_index / x_rows: read by the GATHER instantiations only (row t of Y reads
// row clamp(x_index[t], 0, x_rows - 1) of X); the others never load them.
template <class Args>
struct Linear24Grouped : Args {
  const int* group_offsets;  // groups + 1 values, device
  int groups;
  int x_rows;
  const int* x_index;        // tokens values, device, or null
};
template <class Args, bool GROUPED> struct Linear24ArgsSel { typedef Args type; typedef const Args& view_t; };
template <class Args> struct Linear24ArgsSel<Args, true> { typedef Linear24Grouped<Args> type; typedef Args view_t; };

// The tile form's launcher: the tile counts, then the launch (launch_grid, sm_common.h: the 2^31 - 1 limit on tiles_m * tiles_n, the
// opt-in to more than 64 KiB of dynamic LDS per kernel instantiation).  NT threads per workgroup, LDS bytes of the whole ring.
// BM: the features of Y (a.out) a workgroup covers -- the kernel's tile rows, or half of them for a gated kernel, whose tile is BM
// gate rows + BM up rows.  GROUPED: tiles_n is the slot bound (linear24_grouped_slots) and the offsets (and what a gathered call
// adds) are handed on; grp is not read otherwise.
template <class Args, bool GROUPED, void (*KERNEL)(typename Linear24ArgsSel<Args, GROUPED>::type), int BM, int BN, int NT, size_t LDS>
static int launch_linear24_tile(const Args& a0, const Linear24Groups& grp, hipStream_t st, const char* who, const char* kernel_name) {
  typename Linear24ArgsSel<Args, GROUPED>::type a;
  static_cast<Args&>(a) = a0;
  a.tiles_m = (a.out + BM - 1) / BM;
  if constexpr (GROUPED) {
    a.group_offsets = grp.offsets;
    a.groups = (int)grp.groups;
    a.x_rows = grp.gather ? (int)grp.x_rows : 0;
    a.x_index = grp.gather ? grp.x_index : nullptr;
    a.tiles_n = (int)linear24_grouped_slots((size_t)a.tokens, grp.groups, BN);
  } else {
    a.tiles_n = (a.tokens + BN - 1) / BN;
  }
  return launch_grid<KERNEL>((size_t)a.tiles_m * (size_t)a.tiles_n, NT, LDS, LDS, st, who, kernel_name, a);
}

// ... and the decode form's: one workgroup of NT threads per 16 out features
template <class Args, void (*KERNEL)(Args), int NT>
static int launch_linear24_decode(const Args& a, hipStream_t st, const char* kernel_name) {
  KERNEL<<<dim3((unsigned)ceil_div((size_t)a.out, 16)), dim3(NT), 0, st>>>(a);
  return check_launch(kernel_name);
}

// A grouped workgroup's view of the launch: from its block id to (group, out tile, local token tile), then the argument block cut down
// to that group.  Group g owns tokens [lo, hi): lo = clamp(off[g], 0, tokens) raised to the end of the groups before it,
// hi = clamp(off[g + 1], lo, tokens) -- for non-decreasing offsets the ranges of include/sparsifyme.h; where offsets decrease the
// overlap goes to the earlier group, so that the ranges stay disjoint, their tiles stay within the slot bound, and no group outside
// the overlap loses a tile.  nt_g = ceil((hi - lo) / BN) token tiles each.
// The real tiles are ordered as the per-expert launches of the plain layer would be, one after the other: group-major, within a group
// the plain kernel's (out tile, token tile) order -- so the workgroups that run together share one expert's X rows and walk its
// weight once, as they do in the plain layer (with the out tile outermost across ALL groups every workgroup of a wave of the grid
// had token rows of its own and X came from beyond L2 again for every out tile: the 8192-token cells of profiles/
// linear_grouped_table.txt were 8 - 38 % behind the per-expert loop).  T = tiles_m * sum_g nt_g of them; xcd_remap is applied on T,
// not on the grid, so each XCD gets a contiguous eighth of the REAL tiles; blocks T .. gridDim.x - 1 return.
// Two walks over group_offsets -- the first for T, the second for the group -- of at most LINEAR24_MAX_GROUPS loads each, from one
// address per step, the same in every lane and every wave of the workgroup (scalar loads; nothing is written).  Returns false for a
// block beyond the last real tile (the same answer in the whole workgroup: the caller returns before its first DMA and barrier).
// Otherwise p is the plain kernel's block for expert g alone: vals / meta / w_scale / the per-out bias advanced by g * grows rows
// (vrow: bytes of a blob row in one plane), p.tokens = hi (the token clamp and the store bound), n0 the tile's first token; Y, R,
// x_scale and a per-token bias stay in global token coordinates.  Everything is wave-uniform and held in SGPRs.
template <int BN, class Args>
__device__ __forceinline__ bool linear24_group_view(Args& p, const int* off, int groups, unsigned bid, unsigned grows, unsigned vrow, unsigned& tile_m,
                                                    unsigned& n0) {
  const int tokens = p.tokens;
  const unsigned tiles_m = (unsigned)p.tiles_m;
  auto clamp = [&](int v) { return v < 0 ? 0 : (v > tokens ? tokens : v); };
  unsigned total = 0;
  {
    int cur = 0, next = clamp(off[0]);
    for (int g = 0; g < groups; ++g) {
      const int lo = next > cur ? next : cur;
      next = clamp(off[g + 1]);
      cur = next > lo ? next : lo;
      total += ((unsigned)(cur - lo) + (unsigned)BN - 1u) / (unsigned)BN;
    }
  }
  total *= tiles_m;  // <= tiles_m * slots = gridDim.x
  if (bid >= total) return false;
  const unsigned lid = xcd_remap(bid, total);  // (a bijection on [0, total) for any total: every real tile has a block)
  int cur = 0, next = clamp(off[0]);
  unsigned base = 0;
  for (int g = 0; g < groups; ++g) {
    const int lo = next > cur ? next : cur;
    next = clamp(off[g + 1]);
    const int hi = next > lo ? next : lo;
    const unsigned nt = ((unsigned)(hi - lo) + (unsigned)BN - 1u) / (unsigned)BN;
    if (lid - base < nt * tiles_m) {
      const unsigned within = lid - base;
      tile_m = (unsigned)__builtin_amdgcn_readfirstlane((int)(within / nt));
      const unsigned local = within - tile_m * nt;
      const size_t r0 = (size_t)__builtin_amdgcn_readfirstlane(g) * grows;
      p.vals += r0 * vrow;
      p.meta += r0 * 8;
      if (p.w_scale) p.w_scale += r0;
      if (p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_COL) p.e.bias += r0;
      p.tokens = __builtin_amdgcn_readfirstlane(hi);
      n0 = (unsigned)__builtin_amdgcn_readfirstlane(lo) + local * (unsigned)BN;
      return true;
    }
    base += nt * tiles_m;
    cur = hi;
  }
  return false;
}

// The X image of a stage: [tokens][128 B], 16-byte chunk c of token row t at slot c ^ ((t >> 1) & 7).  A ds_read_b128 access group is
// 16 lanes of which 8 read chunk c of rows {0-3, 12-15} (+16i) and 8 read chunk c ^ 1 of rows {4-11}: with the row's parity choosing the
// half of the 256-byte bank line and (t >> 1) the slot, the 16 lanes cover 16 different 16-byte slots -- all 64 banks once
// (4.14 for the same reads over bytes).
__device__ __forceinline__ unsigned x_swz(unsigned t) { return (t >> 1) & 7u; }

// The row of X behind sorted token row t (< tokens) of a GATHER instantiation: x_index[t] clamped into [0, x_rows), so that whatever
// the array holds no byte outside the x_rows rows of X (and of the fp8 layers' x_scale) is read.
__device__ __forceinline__ unsigned linear24_gather_row(const int* x_index, int x_rows, unsigned t) {
  const int v = x_index[t];
  return (unsigned)(v < 0 ? 0 : (v < x_rows ? v : x_rows - 1));
}

// the lane's four per-out-feature values of a vector (bias, w_scale); indices past the edge are clamped, not branched round (their
// outputs are never stored), so that the loads stay in flight under the K loop
__device__ __forceinline__ f4 linear24_per_out(const float* v, unsigned o0, unsigned out) {
  f4 b;
#pragma unroll
  for (int q = 0; q < 4; ++q) b[q] = v[o0 + q < out ? o0 + q : out - 1];
  return b;
}

// The 16-bit element of Y and R as the store sees it (the fp8 layer's three output types: OutElt<OT>, linear24_fp8.hip): the type,
// the raw piece that moves four of them at once, the conversions.
template <bool BF>
struct Elt16 {
  typedef half_t T;
  typedef u2 raw_t;
  static __device__ __forceinline__ float load(const half_t* p) { return to_f32<BF>(*p); }
  static __device__ __forceinline__ half_t conv(float v) { return to_elt<BF>(v); }
};

// s of s * acc for out feature q of the lane's four: alpha, or with SCALED sw[q] * x_scale[t] (a NULL x_scale skipped)
template <bool SCALED>
__device__ __forceinline__ float linear24_scale(const Linear24Core& p, f4 sw, float xs, int q) {
  if constexpr (SCALED) return p.x_scale ? sw[q] * xs : sw[q];
  else return p.alpha;
}

// One fragment's epilogue and store: the lane holds out features o0 .. o0+3 of token t.  s * acc + beta * R evaluated as
// store_c_tile_epi / store_c_f8 evaluate it (beta * R added only when beta != 0), the bias as an addition of its own, the activation,
// one rounding.  s = alpha, or with SCALED (sw[q] = alpha * w_scale[o0 + q], alpha when there is none) s = sw[q] * x_scale[t].
// R == Y is in place: the lane reads its piece before it writes it, and no other lane touches it.  Indices are unsigned: an edge
// tile's origin plus its extent may pass 2^31 - 1 (never 2^32).
template <class E, bool SCALED>
__device__ __forceinline__ void linear24_store_frag(const Linear24Core& p, const f4 acc, unsigned o0, unsigned t, f4 sw, float xs, float bt, f4 bo) {
  typedef typename E::T T;
  typedef typename E::raw_t raw_t;
  struct Piece { T v[4]; };
  const unsigned out = (unsigned)p.out;
  if (t >= (unsigned)p.tokens || o0 >= out) return;
  const bool use_r = p.beta != 0.0f;
  T* dst = reinterpret_cast<T*>(p.Y) + (size_t)t * p.ldy + o0;
  const T* rs = reinterpret_cast<const T*>(p.e.R) + (size_t)t * p.ldy + o0;
  const bool bias = p.e.bias != nullptr, bias_tok = bias && p.e.bias_dim == SM_BIAS_ROW, bias_out = bias && p.e.bias_dim == SM_BIAS_COL;
  auto scale = [&](int q) { return linear24_scale<SCALED>(p, sw, xs, q); };
  f4 v4;
  if (p.packed) {
    raw_t rraw = {};
    if (use_r) rraw = *reinterpret_cast<const raw_t*>(rs);
    const Piece rv = __builtin_bit_cast(Piece, rraw);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = scale(q) * acc[q];
      if (use_r) v += p.beta * E::load(&rv.v[q]);
      v4[q] = v;
    }
    v4 = epi_act4(epi_bias4(v4, bias_tok, bt, bias_out, bo), p.e.act, p.e.act_arg);
    Piece o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o.v[q] = E::conv(v4[q]);
    *reinterpret_cast<raw_t*>(dst) = __builtin_bit_cast(raw_t, o);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = scale(q) * acc[q];
      if (use_r && o0 + q < out) v += p.beta * E::load(rs + q);
      v4[q] = v;
    }
    v4 = epi_act4(epi_bias4(v4, bias_tok, bt, bias_out, bo), p.e.act, p.e.act_arg);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (o0 + q < out) dst[q] = E::conv(v4[q]);
  }
}

// ---- the gated (gate/up) layer: Y[t][h] = act(g) * u, g from blob row h, u from blob row hidden + h (p.out = hidden) ----------------

// The blob row behind local row `lrow` of a gated tile at hidden origin h0: 16-row fragment f = lrow / 16 is, f even, gate rows
// h0 + 16 (f / 2) + r, and f odd the up rows of the same features -- so that a wave's accumulators 2i, 2i + 1 are a (gate, up) pair of
// the same lane map.  Features past the edge are clamped to hidden - 1 (up: 2 hidden - 1): computed, never stored.
__device__ __forceinline__ unsigned linear24_glu_row(unsigned h0, unsigned lrow, unsigned hidden) {
  const unsigned f = lrow >> 4, h = h0 + 16u * (f >> 1) + (lrow & 15u);
  return (h < hidden - 1u ? h : hidden - 1u) + ((f & 1u) ? hidden : 0u);
}

// The gate's activation on the lane's four values.  NONE and RELU are epi_act4's (the values agree: SM_GLU_ACT_RELU == SM_ACT_RELU).
// SiLU, to the operation: e = expf(-g) (the device library's, <= 1 ulp), d = 1 + e, a = g / d (correctly rounded division);
// e = +inf (g below about -88.7, -inf included, where g / d would be -0 or NaN): a = -0.  NaN in, NaN out; +inf gives +inf.
__device__ __forceinline__ f4 linear24_glu_act4(f4 g, int act) {
#pragma clang fp contract(off)
  static_assert(SM_GLU_ACT_NONE == SM_ACT_NONE && SM_GLU_ACT_RELU == SM_ACT_RELU, "epi_act4 serves the first two");
  if (act != SM_GLU_ACT_SILU) return epi_act4(g, act, 0.0f);
  f4 a;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float e = expf(-g[q]);
    const float d = 1.0f + e;
    a[q] = e == __builtin_inff() ? -0.0f : g[q] / d;
  }
  return a;
}

// One (gate, up) fragment pair's store: the lane holds g and u of features h0 .. h0+3 of token t.  Each is s * acc, then the bias as an
// addition of its own -- the expression linear24_store_frag evaluates before its activation (alpha = 1, beta = 0), through the same
// functions; then a = act(g), y = a * u as ONE fp32 multiply (no contraction from act onward), one rounding.
template <class E, bool SCALED>
__device__ __forceinline__ void linear24_store_glu(const Linear24Core& p, const f4 accg, const f4 accu, unsigned h0, unsigned t, f4 swg, f4 swu, float xs,
                                                   f4 bg, f4 bu) {
  typedef typename E::T T;
  typedef typename E::raw_t raw_t;
  struct Piece { T v[4]; };
  const unsigned hidden = (unsigned)p.out;
  if (t >= (unsigned)p.tokens || h0 >= hidden) return;
  T* dst = reinterpret_cast<T*>(p.Y) + (size_t)t * p.ldy + h0;
  const bool bias = p.e.bias != nullptr;
  f4 g4, u4v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    g4[q] = linear24_scale<SCALED>(p, swg, xs, q) * accg[q];
    u4v[q] = linear24_scale<SCALED>(p, swu, xs, q) * accu[q];
  }
  g4 = epi_bias4(g4, false, 0.f, bias, bg);
  u4v = epi_bias4(u4v, false, 0.f, bias, bu);
  f4 y;
  {
#pragma clang fp contract(off)
    y = linear24_glu_act4(g4, p.e.act) * u4v;
  }
  if (p.packed) {
    Piece o;
#pragma unroll
    for (int q = 0; q < 4; ++q) o.v[q] = E::conv(y[q]);
    *reinterpret_cast<raw_t*>(dst) = __builtin_bit_cast(raw_t, o);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (h0 + q < hidden) dst[q] = E::conv(y[q]);
  }
}

// The gated decode form's tail: every wave's partial (gate, up) pair meets in LDS (2 x NWV KiB), wave 0 finishes both -- adding the
// partials in wave order 0, 1, .. as linear24_decode_tail does, so that g and u have the plain decode kernel's bits -- fetches the
// lane's biases and scales and hands the pair to STORE.  Workgroup = 16 hidden features from m0, tokens <= 16.
template <class Args, void (*STORE)(const Args&, f4, f4, unsigned, unsigned, f4, f4, float, f4, f4), bool SCALED, int NWV>
__device__ __forceinline__ void linear24_decode_tail_glu(const Args& p, const f4 (&acc)[2], unsigned m0) {
  __shared__ f4 part[NWV][2][64];
  const unsigned tid = threadIdx.x, lane = tid & 63u, g = lane >> 4, r = lane & 15u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  part[wave][0][lane] = acc[0];
  part[wave][1][lane] = acc[1];
  __syncthreads();
  if (tid >= 64u) return;
  // (a loop of three turns, not straight-line code: with all 2 * NWV reads in flight at once the wave would need 8 * NWV registers
  // for them -- beyond the 128 a 16-wave workgroup leaves each wave)
  f4 sg = part[0][0][lane], su = part[0][1][lane];
#pragma unroll 5
  for (int w = 1; w < NWV; ++w) {
    sg += part[w][0][lane];
    su += part[w][1][lane];
  }
  const unsigned hidden = (unsigned)p.out, h0 = m0 + 4u * g, t = r;
  const bool tv = t < (unsigned)p.tokens;
  f4 bg = {0.f, 0.f, 0.f, 0.f}, bu = bg, swg = {p.alpha, p.alpha, p.alpha, p.alpha}, swu = swg;
  float xs = 1.f;
  if (p.e.bias != nullptr) {
    bg = linear24_per_out(p.e.bias, h0, hidden);
    bu = linear24_per_out(p.e.bias + hidden, h0, hidden);
  }
  if constexpr (SCALED) {
    if (p.w_scale) {
      swg = p.alpha * linear24_per_out(p.w_scale, h0, hidden);
      swu = p.alpha * linear24_per_out(p.w_scale + hidden, h0, hidden);
    }
    if (p.x_scale && tv) xs = p.x_scale[t];
  }
  STORE(p, sg, su, h0, t, swg, swu, xs, bg, bu);
}

// The decode form's tail: every wave's partial fragments meet in LDS, wave j finishes fragment j -- lane for lane the accumulator
// map -- adding the partials in wave order 0, 1, .. (the same bits on every run), fetches the lane's bias and scales and hands the
// sum to STORE (linear24_store_frag, or a switch over its instantiations).  Workgroup = 16 out features from m0 x NWV waves.
template <class Args, void (*STORE)(const Args&, f4, unsigned, unsigned, f4, float, float, f4), bool SCALED, int FN, int NWV>
__device__ __forceinline__ void linear24_decode_tail(const Args& p, const f4 (&acc)[FN], unsigned m0) {
  static_assert(FN * 64 <= 64 * NWV, "one thread per output piece in the combine");
  __shared__ f4 part[NWV][FN][64];
  const unsigned tid = threadIdx.x, lane = tid & 63u, g = lane >> 4, r = lane & 15u;
  const unsigned wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
  for (int j = 0; j < FN; ++j) part[wave][j][lane] = acc[j];
  __syncthreads();
  if (tid >= (unsigned)(FN * 64)) return;
  const unsigned j = wave;
  f4 s = part[0][j][lane];
#pragma unroll
  for (int w = 1; w < NWV; ++w) s += part[w][j][lane];
  const unsigned o0 = m0 + 4u * g, t = 16u * j + r;
  const bool tv = t < (unsigned)p.tokens;
  f4 bo = {0.f, 0.f, 0.f, 0.f}, sw = {p.alpha, p.alpha, p.alpha, p.alpha};
  float bt = 0.f, xs = 1.f;
  if (p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_COL) bo = linear24_per_out(p.e.bias, o0, (unsigned)p.out);
  if (p.e.bias != nullptr && p.e.bias_dim == SM_BIAS_ROW && tv) bt = p.e.bias[t];
  if constexpr (SCALED) {
    if (p.w_scale) sw = p.alpha * linear24_per_out(p.w_scale, o0, (unsigned)p.out);
    if (p.x_scale && tv) xs = p.x_scale[t];
  }
  STORE(p, s, o0, t, sw, xs, bt, bo);
}

}  // namespace sm
