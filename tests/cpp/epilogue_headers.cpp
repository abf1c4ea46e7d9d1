// epilogue_headers -- the epilogue overloads of include/sparsify.me/spmma.hxx by VALUE: sparsifyme::spmma_fused(..., spmma_epilogue_t)
// and spmma_plan_t::multiply(..., spmma_epilogue_t) against a host fp64 evaluation of
//   D = act(alpha * A . B + beta * R + bias)
// on an A that already is 2:4 (two zeros in every strip of four, so the STRIP selection keeps exactly its non-zeros and the
// host needs no selection rule), for fp16 and bfloat16, column and row bias, ReLU and hardswish, residual out of place and in
// place, one fused shape, one ragged-k (span) shape and one n % 8 != 0 shape that the header runs as compress + multiply.
// Bound: the project's GEMM bound (tests/test_gpu_parity.py) with k + 2 accumulation steps and the activation's Lipschitz constant.
// Prints "<name>: ok" / "MISMATCH" per check and "<n> checks, <f> failed".
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include <sparsify.me/containers/vector.hxx>
#include <sparsify.me/spmma.hxx>

using namespace sparsifyme;

static unsigned lcg_state = 12345u;
static float lcg() {  // uniform(-1, 1)
  lcg_state = lcg_state * 1664525u + 1013904223u;
  return (float)((lcg_state >> 8) & 0xffffu) / 32768.0f - 1.0f;
}

template <typename T>
struct limits;
template <>
struct limits<_Float16> {
  static constexpr double round = 0x1p-10, tiny = 0x1p-24;
  static constexpr const char* name = "f16";
};
template <>
struct limits<__bf16> {
  static constexpr double round = 0x1p-7, tiny = 0x1p-126;
  static constexpr const char* name = "bf16";
};

static double act64(int act, double x) {
  if (act == SM_ACT_RELU) return std::max(x, 0.0);
  if (act == SM_ACT_HARDSWISH) return x * std::min(std::max(x + 3.0, 0.0), 6.0) / 6.0;
  return x;
}

static int checks = 0, failed = 0;

template <typename T>
static void one(std::size_t m, std::size_t n, std::size_t k, std::size_t b, int bias_dim, int act, bool in_place, bool through_plan) {
  const float alpha = 12.0f / std::sqrt((float)k), beta = 1.0f;
  host_vector<T> hA(m * k * b), hB(k * n * b), hR(m * n * b);
  host_vector<float> hbias(bias_dim == SM_BIAS_COL ? n : m);
  for (std::size_t i = 0; i < hA.size(); ++i) {
    const std::size_t col = i % k, e = col % 4, keep0 = ((i / k) * 7 + col / 4) % 3;  // positions (0,1), (1,2) or (2,3) of the strip stay
    const float v = lcg();
    hA[i] = static_cast<T>((e == keep0 || e == keep0 + 1) ? (v == 0.0f ? 0.5f : v) : 0.0f);
  }
  for (auto& x : hB) x = static_cast<T>(lcg());
  for (auto& x : hR) x = static_cast<T>(lcg());
  for (auto& x : hbias) x = lcg();
  device_vector<T> A = hA, B = hB, R = hR, D = hR;  // (in place: D starts as the residual)
  device_vector<float> bias = hbias;
  spmma_epilogue_t ep;
  ep.bias = bias.data().get();
  ep.bias_dim = bias_dim;
  ep.act = act;
  ep.residual = in_place ? nullptr : R.data().get();
  int rc = SM_STATUS_SUCCESS;
  if (through_plan) {
    spmma_plan_t<T> plan(m, k, b);
    rc = plan.compress(A.data().get());
    if (rc == SM_STATUS_SUCCESS) rc = plan.multiply(B.data().get(), D.data().get(), n, ep, alpha, beta);
    (void)hipDeviceSynchronize();
  } else {
    (void)spmma_fused(A.data().get(), B.data().get(), D.data().get(), m, n, k, b, ep, alpha, beta);
  }
  const host_vector<T> hD = D.to_host();
  const double lip = act == SM_ACT_HARDSWISH ? 1.5 : 1.0;
  double worst = 0.0;
  for (std::size_t bb = 0; bb < b; ++bb)
    for (std::size_t i = 0; i < m; ++i)
      for (std::size_t j = 0; j < n; ++j) {
        double s = 0.0, sa = 0.0;
        for (std::size_t q = 0; q < k; ++q) {
          const double a = (double)(float)hA[(bb * m + i) * k + q], x = (double)(float)hB[(bb * k + q) * n + j];
          s += a * x;
          sa += std::fabs(a * x);
        }
        const double r = (double)(float)hR[(bb * m + i) * n + j], bv = hbias[bias_dim == SM_BIAS_COL ? j : i];
        const double ref = act64(act, alpha * s + beta * r + bv);
        const double bound = limits<T>::round * std::fabs(ref) + lip * 2.0 * (k + 2) * 0x1p-24 * (alpha * sa + std::fabs(beta * r) + std::fabs(bv)) + limits<T>::tiny;
        const double err = std::fabs((double)(float)hD[(bb * m + i) * n + j] - ref);
        worst = std::max(worst, err / bound);
      }
  ++checks;
  const bool ok = rc == SM_STATUS_SUCCESS && worst <= 1.0;
  if (!ok) ++failed;
  std::cout << (through_plan ? "plan.multiply" : "spmma_fused") << "<" << limits<T>::name << "> " << m << "x" << n << "x" << k << "x" << b
            << (bias_dim == SM_BIAS_COL ? " bias col" : " bias row") << (act == SM_ACT_RELU ? " relu" : act == SM_ACT_HARDSWISH ? " hardswish" : " none")
            << (in_place ? " in place" : " residual") << " (err / bound " << worst << "): " << (ok ? "ok" : "MISMATCH") << std::endl;
}

template <typename T>
static void all() {
  one<T>(196, 64, 128, 2, SM_BIAS_COL, SM_ACT_RELU, false, false);
  one<T>(196, 64, 128, 2, SM_BIAS_ROW, SM_ACT_HARDSWISH, true, false);
  one<T>(130, 136, 192, 1, SM_BIAS_COL, SM_ACT_RELU, true, false);
  one<T>(128, 64, 147, 2, SM_BIAS_COL, SM_ACT_HARDSWISH, false, false);  // ragged k: the span form
  one<T>(64, 40, 72, 2, SM_BIAS_ROW, SM_ACT_RELU, false, false);          // n % 8 != 0 ... and k % 64 != 0: compress + multiply inside the header
  one<T>(196, 64, 128, 2, SM_BIAS_COL, SM_ACT_RELU, false, true);
  one<T>(130, 24, 64, 3, SM_BIAS_ROW, SM_ACT_NONE, true, true);
}

int main() {
  if (sm_device_check() != SM_STATUS_SUCCESS) {
    std::cerr << "epilogue_headers: " << sm_last_error() << std::endl;
    return EXIT_FAILURE;
  }
  all<_Float16>();
  all<__bf16>();
  std::cout << checks << " checks, " << failed << " failed" << std::endl;
  return failed ? EXIT_FAILURE : EXIT_SUCCESS;
}
