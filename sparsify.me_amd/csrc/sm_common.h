// Shared host/device helpers for libsparsifyme.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>

#include "../../include/sparsifyme.h"

namespace sm {

typedef _Float16 half_t;
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16 __attribute__((ext_vector_type(16)));
typedef short s4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f16x __attribute__((ext_vector_type(16)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef unsigned int u2 __attribute__((ext_vector_type(2)));

// Records the message sm_last_error() returns (thread local, defined in api.hip).
void set_error(const char* fmt, ...);

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return SM_STATUS_LAUNCH_FAILED;
  }
  return SM_STATUS_SUCCESS;
}

// One-shot opt-in of a kernel to more than 64 KiB of dynamic LDS, done once PER DEVICE (the attribute belongs to the
// function object of the current device; one bit per device ordinal, set after the call succeeded, so two threads
// racing on the first launch at worst both set it).  A refused opt-in is reported here, not as a later launch error.
struct LdsOptIn {
  std::atomic<unsigned long long> done[4];  // 256 device ordinals
};
int ensure_dyn_lds(LdsOptIn& s, const void* fn, size_t bytes, const char* what);
// Compute units of the current device, queried once per device ordinal (hipGetDeviceProperties costs tens of
// microseconds; launchers that size a grid by the CU count call this on every launch).
int device_cu_count();

// The tail of every tile-grid launcher, stated once: a 1-D grid of `nwg` workgroups of `threads` threads with `lds` bytes of dynamic
// LDS.  In this order: an empty grid is SM_STATUS_SUCCESS with nothing touched; more than 2^31 - 1 workgroups is "<who>: grid too
// large"; the opt-in to `lds_optin` bytes when that is more than 64 KiB; the launch; check_launch.  The kernel is a template
// parameter, so that the opt-in state below is ONE PER KERNEL INSTANTIATION (a state shared by two kernels would skip the second
// one's opt-in, and its first launch above 64 KiB would fail).  lds_optin is the most the instantiation can ever ask for (or simply
// the hardware's 160 KiB), `lds` what this launch touches; LDS_NO_OPTIN for a kernel that never passes 64 KiB: no opt-in, no
// hipGetDevice.  kernel_name: what ensure_dyn_lds and check_launch call the kernel in their messages.
constexpr size_t LDS_NO_OPTIN = 0;
#ifdef __HIPCC__
template <auto KERNEL, class... Args>
static int launch_grid(size_t nwg, unsigned threads, size_t lds_optin, size_t lds, hipStream_t st, const char* who, const char* kernel_name,
                       const Args&... args) {
  if (nwg == 0) return SM_STATUS_SUCCESS;
  if (nwg > 0x7fffffffu) {
    set_error("%s: grid too large", who);
    return SM_STATUS_NOT_SUPPORTED;
  }
  if (lds_optin > 64 * 1024) {
    static LdsOptIn optin;
    if (const int rc = ensure_dyn_lds(optin, reinterpret_cast<const void*>(KERNEL), lds_optin, kernel_name)) return rc;
  }
  KERNEL<<<dim3((unsigned)nwg), dim3(threads), lds, st>>>(args...);
  return check_launch(kernel_name);
}
#endif

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline size_t ceil_div(size_t x, size_t y) { return (x + y - 1) / y; }
inline size_t mul_sat(size_t a, size_t b) { return (a != 0 && b > SIZE_MAX / a) ? SIZE_MAX : a * b; }  // saturating
// Raise a device flag from one lane of a wave: the relaxed read first, so that once the flag is up the thousands of waves that also
// found something do not queue their atomics on one address (an all-invalid 462 MB operand spent 100 us of a 214 us check pass there).
#ifdef __HIPCC__
__device__ __forceinline__ void raise_flag(int* flag) {
  if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) atomicOr(flag, 1);
}
#endif
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Layout of the 2:4 compressed blob (include/sparsifyme.h header comment).
struct BlobLayout {
  size_t kc, M, meta_off, total;
};
inline BlobLayout blob_layout(size_t m, size_t k, size_t elt, size_t batch) {
  BlobLayout L;
  L.kc = round_up(k, 64);
  L.M = m * batch;
  L.meta_off = round_up(L.M * (L.kc / 2) * elt, 256);
  L.total = L.meta_off + round_up(L.M * (L.kc / 8), 256);
  return L;
}

// Grid size for grid-stride streaming kernels: enough blocks to fill 256 CUs x 8, capped.
// `uncapped`: one item per thread and no second trip (round 5: the copy probe's finding -- workgroups handed out in address order keep the chip's traffic
// inside a few megabytes at a time; a capped grid's stride loop smears it.  It pays where the kernel is a plain copy-like stream: STRIP prune of the 462 MB
// operand 176 -> 155 us, 231 MB 85 -> 80; the check, compress, TILE and one-pass kernels do not move, profiles/prune_ab_r05as.txt).
inline unsigned stream_grid(size_t work_items, unsigned block, bool uncapped = false) {
  size_t g = ceil_div(work_items, block);
  if (!uncapped && g > 256 * 16) g = 256 * 16;
  if (g > 0x7fffffffull) g = 0x7fffffffull;
  if (g == 0) g = 1;
  return (unsigned)g;
}

}  // namespace sm
