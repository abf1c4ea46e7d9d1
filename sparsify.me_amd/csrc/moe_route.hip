// moe_route.hip -- sm_moe_route (extension): the router's expert ids to what the grouped layers and the combine step read, on the device.
//     P = tokens * top_k pairs, pair p = t * top_k + j.  A STABLE COUNTING SORT of the pairs by expert id; ids outside [0, groups) are
//     dropped.  group_offsets[g] = kept pairs with id < g; sorted_pair[s] = the pairs of expert e in ascending p for s in
//     [off[e], off[e + 1]); sorted_token[s] = sorted_pair[s] / top_k; both -1 for s in [V, P), V = off[groups]; pair_pos[p] = s or -1.
// Every output is an integer the definition fixes: every form gives the same values, on every run.
//
// One routine (route_counts, route_ranks) sorts a CHUNK of at most MOE_ROUTE_CHUNK consecutive pairs inside one workgroup of MOE_ROUTE_NW
// waves; wave w owns a contiguous quarter of the chunk's pairs, rounded up to whole 64-pair steps (the segment: route_segment), so that
// (chunk, wave, position in the segment) is the order of p:
//   counts  cnt[w][g] = pairs of expert g in wave w's segment (LDS integer atomics on counters the kernel zeroed itself: exact whatever
//           the order);
//   ranks   cnt[w][g] is replaced by the first slot of wave w's pairs of expert g (a start handed in per expert + the counts of the
//           waves before it), then every wave walks its segment 64 pairs at a time IN ORDER: the lanes that hold the same id find each
//           other by ballot (one round per distinct id of the step, the lowest lane first; registers only), then a lane's slot is the
//           counter + the number of lower lanes with its id, and one lane per id moves the counter on: one LDS read and one LDS write
//           per step, every read ahead of every write.  No atomics: only wave w touches cnt[w][*].
// Forms (sm_moe_route_form):
//   SINGLE  P <= SM_MOE_ROUTE_SINGLE_MAX_PAIRS = one chunk: one launch, one workgroup; counts, the scan over the experts and the ranks
//           all in its LDS.  No workspace.  P == 0 (EMPTY with groups > 0) runs it too: it writes the groups + 1 zeros.
//   MULTI   one workgroup per chunk.  (1) counts of every chunk -> workspace[chunk][groups] (every entry written: nothing to zero
//           first); (2) one workgroup: per expert the exclusive scan over the chunks, in place, then the scan over the experts'
//           totals -> group_offsets; (3) per chunk: counts again (they cost less than a second workspace array), ranks from
//           group_offsets[g] + workspace[chunk][g], the stable scatter, and -1 into the chunk's share of [V, P).
// The kernels of one call follow each other on the stream; no memset node, no allocation, no synchronisation.
#include "sm_common.h"

namespace sm {

constexpr int MOE_ROUTE_NW = 4, MOE_ROUTE_NT = 64 * MOE_ROUTE_NW;
constexpr size_t MOE_ROUTE_CHUNK = SM_MOE_ROUTE_CHUNK;
constexpr size_t MOE_ROUTE_MAX_GROUPS = SM_LINEAR24_MAX_GROUPS;
static_assert(SM_MOE_ROUTE_SINGLE_MAX_PAIRS == SM_MOE_ROUTE_CHUNK, "the SINGLE form is one chunk");
static_assert(MOE_ROUTE_CHUNK % (64 * MOE_ROUTE_NW) == 0, "a wave's segment is whole 64-pair steps");

// Pairs per wave of the chunk that starts at pair p0: a quarter of the chunk's min(CHUNK, P - p0) pairs in whole 64-pair steps, so that a
// short chunk (the decode case: tens of pairs) is not walked by one wave alone.  <= CHUNK / NW.
__host__ __device__ inline unsigned route_segment(unsigned P, unsigned p0) {
  const unsigned n = P - p0 < (unsigned)MOE_ROUTE_CHUNK ? P - p0 : (unsigned)MOE_ROUTE_CHUNK;
  return (n + 64u * MOE_ROUTE_NW - 1u) / (64u * MOE_ROUTE_NW) * 64u;
}

inline int moe_route_form(size_t tokens, size_t top_k, size_t groups, size_t* pairs) {
  *pairs = 0;
  if (groups > MOE_ROUTE_MAX_GROUPS) return SM_MOE_ROUTE_FORM_INVALID;
  if (top_k != 0 && tokens > 0x7fffffffull / top_k) return SM_MOE_ROUTE_FORM_INVALID;  // P > 2^31 - 1
  const size_t P = tokens * top_k;
  *pairs = P;
  if (P == 0 || groups == 0) return SM_MOE_ROUTE_FORM_EMPTY;
  return P <= SM_MOE_ROUTE_SINGLE_MAX_PAIRS ? SM_MOE_ROUTE_FORM_SINGLE : SM_MOE_ROUTE_FORM_MULTI;
}

struct MoeRouteArgs {
  const int* ids;
  int* group_offsets;
  int* sorted_token;
  int* sorted_pair;
  int* pair_pos;
  int* hist;  // MULTI: [chunks][groups]
  unsigned P, top_k, groups, chunks;
};

// cnt[w][g] = pairs with id g among wave w's segment of the chunk that starts at pair p0.  Ends with a barrier.
__device__ __forceinline__ void route_counts(const MoeRouteArgs& a, unsigned p0, int (*cnt)[MOE_ROUTE_MAX_GROUPS]) {
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  for (unsigned i = tid; i < (unsigned)MOE_ROUTE_NW * a.groups; i += MOE_ROUTE_NT) cnt[i / a.groups][i % a.groups] = 0;
  __syncthreads();
  const unsigned seg = route_segment(a.P, p0), lo = p0 + wave * seg;
  for (unsigned i = lane; i < seg; i += 64u) {
    const unsigned p = lo + i;
    if (p < a.P) {
      const int id = a.ids[p];
      if (id >= 0 && (unsigned)id < a.groups) atomicAdd(&cnt[wave][id], 1);
    }
  }
  __syncthreads();
}

// The stable scatter of the chunk at p0.  On entry cnt[w][g] holds the counts and start[g] (LDS) the slot of the chunk's first pair of
// expert g; the loop over g turns cnt[w][g] into wave w's first slot of expert g, the ordered walk hands the slots out.
__device__ __forceinline__ void route_ranks(const MoeRouteArgs& a, unsigned p0, int (*cnt)[MOE_ROUTE_MAX_GROUPS], const int* start) {
  const unsigned tid = threadIdx.x, lane = tid & 63u;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  for (unsigned g = tid; g < a.groups; g += MOE_ROUTE_NT) {
    int run = start[g];
#pragma unroll
    for (int w = 0; w < MOE_ROUTE_NW; ++w) {
      const int c = cnt[w][g];
      cnt[w][g] = run;
      run += c;
    }
  }
  __syncthreads();
  const unsigned seg = route_segment(a.P, p0), lo = p0 + wave * seg;
  for (unsigned i0 = 0; i0 < seg && lo + i0 < a.P; i0 += 64u) {  // (wave-uniform bounds)
    const unsigned p = lo + i0 + lane;
    int id = -1;
    if (p < a.P) {
      id = a.ids[p];
      if (id < 0 || (unsigned)id >= a.groups) id = -1;
    }
    int rank = 0, total = 0;  // among the step's lanes with this lane's id: the lower ones, all of them
    unsigned long long todo = __ballot(id >= 0);
    while (todo != 0ull) {  // one round per distinct id of the step; every lane of the wave takes every round
      const int leader = __builtin_ctzll(todo);
      const int lid = __builtin_amdgcn_readlane(id, leader);
      const unsigned long long same = __ballot(id == lid);
      if (id == lid) {
        rank = __builtin_popcountll(same & ((1ull << lane) - 1ull));
        total = __builtin_popcountll(same);
      }
      todo &= ~same;
    }
    int slot = -1;
    if (id >= 0) {
      volatile int* ctr = &cnt[wave][id];  // (volatile: another lane of this wave wrote it in an earlier step)
      const int base = *ctr;
      slot = base + rank;
      __builtin_amdgcn_wave_barrier();  // every lane's read of its counter stands before the writes: one lane per id, distinct addresses
      if (rank == 0) *ctr = base + total;
    }
    if (p < a.P) {
      a.pair_pos[p] = slot;
      if (slot >= 0) {  // (slot < V <= P by construction: a slot is a count of kept pairs)
        a.sorted_pair[slot] = (int)p;
        a.sorted_token[slot] = (int)(p / a.top_k);
      }
    }
  }
}

// In-place exclusive scan of v[0 .. n) (LDS, n <= MOE_ROUTE_MAX_GROUPS = 4 per thread) by the whole workgroup; returns the total.
// part: MOE_ROUTE_NT ints of LDS.  Begins and ends with a barrier.
__device__ __forceinline__ int route_scan(int* v, unsigned n, int* part) {
  static_assert(MOE_ROUTE_MAX_GROUPS <= 4 * MOE_ROUTE_NT, "four experts per thread");
  const unsigned tid = threadIdx.x;
  __syncthreads();
  int x[4], sum = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    x[q] = 4u * tid + q < n ? v[4u * tid + q] : 0;
    sum += x[q];
  }
  part[tid] = sum;
  __syncthreads();
  for (unsigned d = 1; d < (unsigned)MOE_ROUTE_NT; d <<= 1) {  // Hillis-Steele, inclusive
    const int add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int run = part[tid] - sum;
  const int total = part[MOE_ROUTE_NT - 1];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (4u * tid + q < n) v[4u * tid + q] = run;
    run += x[q];
  }
  __syncthreads();
  return total;
}

// [V, P) of both sorted arrays gets -1: positions s0 .. s0 + n - 1 of it are this workgroup's
__device__ __forceinline__ void route_tail(const MoeRouteArgs& a, unsigned V, unsigned s0, unsigned n) {
  for (unsigned i = threadIdx.x; i < n; i += MOE_ROUTE_NT) {
    const unsigned s = s0 + i;
    if (s >= V && s < a.P) {
      a.sorted_pair[s] = -1;
      a.sorted_token[s] = -1;
    }
  }
}

__global__ __launch_bounds__(MOE_ROUTE_NT) void moe_route_single_kernel(const MoeRouteArgs a) {
  __shared__ int cnt[MOE_ROUTE_NW][MOE_ROUTE_MAX_GROUPS];
  __shared__ int start[MOE_ROUTE_MAX_GROUPS];
  __shared__ int part[MOE_ROUTE_NT];
  route_counts(a, 0u, cnt);
  for (unsigned g = threadIdx.x; g < a.groups; g += MOE_ROUTE_NT) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < MOE_ROUTE_NW; ++w) t += cnt[w][g];
    start[g] = t;
  }
  const int V = route_scan(start, a.groups, part);
  for (unsigned g = threadIdx.x; g < a.groups; g += MOE_ROUTE_NT) a.group_offsets[g] = start[g];
  if (threadIdx.x == 0) a.group_offsets[a.groups] = V;
  route_ranks(a, 0u, cnt, start);
  route_tail(a, (unsigned)V, 0u, a.P);
}

__global__ __launch_bounds__(MOE_ROUTE_NT) void moe_route_hist_kernel(const MoeRouteArgs a) {
  __shared__ int cnt[MOE_ROUTE_NW][MOE_ROUTE_MAX_GROUPS];
  const unsigned c = blockIdx.x;
  route_counts(a, c * (unsigned)MOE_ROUTE_CHUNK, cnt);
  for (unsigned g = threadIdx.x; g < a.groups; g += MOE_ROUTE_NT) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < MOE_ROUTE_NW; ++w) t += cnt[w][g];
    a.hist[(size_t)c * a.groups + g] = t;
  }
}

__global__ __launch_bounds__(MOE_ROUTE_NT) void moe_route_scan_kernel(const MoeRouteArgs a) {
  __shared__ int start[MOE_ROUTE_MAX_GROUPS];
  __shared__ int part[MOE_ROUTE_NT];
  for (unsigned g = threadIdx.x; g < a.groups; g += MOE_ROUTE_NT) {
    int run = 0;
    for (unsigned c = 0; c < a.chunks; ++c) {
      int* h = a.hist + (size_t)c * a.groups + g;
      const int v = *h;
      *h = run;
      run += v;
    }
    start[g] = run;
  }
  const int V = route_scan(start, a.groups, part);
  for (unsigned g = threadIdx.x; g < a.groups; g += MOE_ROUTE_NT) a.group_offsets[g] = start[g];
  if (threadIdx.x == 0) a.group_offsets[a.groups] = V;
}

__global__ __launch_bounds__(MOE_ROUTE_NT) void moe_route_scatter_kernel(const MoeRouteArgs a) {
  __shared__ int cnt[MOE_ROUTE_NW][MOE_ROUTE_MAX_GROUPS];
  __shared__ int start[MOE_ROUTE_MAX_GROUPS];
  const unsigned c = blockIdx.x, p0 = c * (unsigned)MOE_ROUTE_CHUNK;
  route_counts(a, p0, cnt);
  for (unsigned g = threadIdx.x; g < a.groups; g += MOE_ROUTE_NT) start[g] = a.group_offsets[g] + a.hist[(size_t)c * a.groups + g];
  __syncthreads();
  route_ranks(a, p0, cnt, start);
  route_tail(a, (unsigned)a.group_offsets[a.groups], p0, (unsigned)MOE_ROUTE_CHUNK);
}

}  // namespace sm

using namespace sm;

extern "C" int sm_moe_route_form(size_t tokens, size_t top_k, size_t groups, int* form) {
  if (!form) {
    set_error("sm_moe_route_form: invalid argument (form is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  size_t P;
  *form = moe_route_form(tokens, top_k, groups, &P);
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_moe_route_workspace_size(size_t tokens, size_t top_k, size_t groups, size_t* bytes) {
  if (!bytes) {
    set_error("sm_moe_route_workspace_size: invalid argument (bytes is NULL)");
    return SM_STATUS_INVALID_VALUE;
  }
  size_t P;
  const int form = moe_route_form(tokens, top_k, groups, &P);
  if (form == SM_MOE_ROUTE_FORM_INVALID) {
    set_error("sm_moe_route_workspace_size: tokens * top_k exceeds 2^31-1 or groups exceeds SM_LINEAR24_MAX_GROUPS");
    return SM_STATUS_NOT_SUPPORTED;
  }
  *bytes = form == SM_MOE_ROUTE_FORM_MULTI ? ceil_div(P, MOE_ROUTE_CHUNK) * groups * sizeof(int) : 0;
  return SM_STATUS_SUCCESS;
}

extern "C" int sm_moe_route(const int* expert_ids, size_t tokens, size_t top_k, size_t groups, int* group_offsets, int* sorted_token, int* sorted_pair,
                            int* pair_pos, void* workspace, size_t workspace_bytes, sm_stream_t stream) {
  size_t P;
  const int form = moe_route_form(tokens, top_k, groups, &P);
  const size_t need = form == SM_MOE_ROUTE_FORM_MULTI ? ceil_div(P, MOE_ROUTE_CHUNK) * groups * sizeof(int) : 0;
  if (!expert_ids || !group_offsets || !sorted_token || !sorted_pair || !pair_pos || (need != 0 && !workspace) || workspace_bytes < need) {
    set_error("sm_moe_route: invalid argument (null operand, null or too small workspace: sm_moe_route_workspace_size)");
    return SM_STATUS_INVALID_VALUE;
  }
  if (form == SM_MOE_ROUTE_FORM_INVALID) {
    set_error("sm_moe_route: tokens * top_k exceeds 2^31-1 or groups exceeds SM_LINEAR24_MAX_GROUPS");
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (groups == 0) return SM_STATUS_SUCCESS;
  MoeRouteArgs a = {expert_ids, group_offsets, sorted_token, sorted_pair, pair_pos, (int*)workspace, (unsigned)P, (unsigned)(top_k ? top_k : 1), (unsigned)groups,
                    (unsigned)ceil_div(P, MOE_ROUTE_CHUNK)};
  hipStream_t st = (hipStream_t)stream;
  if (form != SM_MOE_ROUTE_FORM_MULTI) {  // SINGLE, and P == 0: the groups + 1 zeros
    moe_route_single_kernel<<<dim3(1), dim3(MOE_ROUTE_NT), 0, st>>>(a);
    return check_launch("moe_route_single_kernel");
  }
  moe_route_hist_kernel<<<dim3(a.chunks), dim3(MOE_ROUTE_NT), 0, st>>>(a);
  if (const int rc = check_launch("moe_route_hist_kernel")) return rc;
  moe_route_scan_kernel<<<dim3(1), dim3(MOE_ROUTE_NT), 0, st>>>(a);
  if (const int rc = check_launch("moe_route_scan_kernel")) return rc;
  moe_route_scatter_kernel<<<dim3(a.chunks), dim3(MOE_ROUTE_NT), 0, st>>>(a);
  return check_launch("moe_route_scatter_kernel");
}
