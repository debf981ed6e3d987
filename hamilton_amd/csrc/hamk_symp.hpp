// hamk_symp.hpp -- symplectic fixed-step stepping on the lane mapping (one trajectory per lane, n <= 16): the implicit
// midpoint rule, solved by a FIXED number of fixed-point iterations, and its three-substep symmetric composition.
// No reference counterpart (the reference integrates with GSL's RKF45 only).
//
// One substep of size h from y = [q; p]:
//     z^0 = y;    z^{k+1} = y + (h/2) f(z^k),  k = 0 .. iters - 1;    y <- 2 z^{iters} - y
// exactly `iters` right-hand sides.  Where the iteration has converged, z is the midpoint (y_old + y_new) / 2 and the
// substep is the implicit midpoint rule: symplectic, symmetric, second order.  The count is an argument, never a
// convergence test: a lane that does not converge costs what every other lane costs, the launch cannot spin, and the
// result is a pure function of (y, h, iters) -- bit-reproducible whatever the neighbours do.  What the caller gets
// instead of a test is `residual`: per trajectory the largest last-iteration update
//     max_j |z^{iters}_j - z^{iters-1}_j| / max(1, |y_j|)
// over all steps and substeps of the launch -- too large a value says that `iters` was too small for this dt.
//
// order 4: three substeps of ha, hb, ha per step (Yoshida's triple jump: ha = dt / (2 - 2^(1/3)), hb = dt - 2 ha; the
// host computes them in fp64 and passes them in).  order 2: one substep, nsub = 1, ha = dt.  A negative dt steps back.
//
// The right-hand side is ham_eqs<S, S::MODE_H> with its default TRIG_FULL, the instantiation of hamk_hameqs_k: no LDS
// table, the symbolic / H / D / R path as the system has it.  The state is loaded once, lives in registers for the whole
// launch and is stored once.  The loops over steps, substeps and iterations all stay rolled: one copy of the right-hand
// side, code size independent of `iters`.
//
// This header rides beside hamk_device.hpp in a COMPANION module of the lane variant (hamk_build.cpp build_symp): the
// variant's generated source with its HAMK_INSTANTIATE(HamkSys) replaced by HAMK_INSTANTIATE_SYMP(HamkSys).
#pragma once
#include "hamk_device.hpp"

namespace hamk {

template <class S>
HAMK_DEV void symp_body(double* __restrict__ q, double* __restrict__ p, i64 B, int nsteps, int nsub, double ha, double hb,
                        int iters, double* __restrict__ residual, int* __restrict__ status) {
  constexpr int N = S::N;
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double yq[N], yp[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { yq[j] = q[(i64)j * B + i]; yp[j] = p[(i64)j * B + i]; }
  int st = 0;
  double res = 0.0;
  TrigCache<S::NTRIG_F> tc;
#pragma unroll 1
  for (int s = 0; s < nsteps; ++s) {
#pragma unroll 1
    for (int u = 0; u < nsub; ++u) {
      const double hh = 0.5 * ((u == 1) ? hb : ha);             // wave-uniform: a scalar select
      double zq[N], zp[N];
#pragma unroll
      for (int j = 0; j < N; ++j) { zq[j] = yq[j]; zp[j] = yp[j]; }
      double last = 0.0;
#pragma unroll 1
      for (int k = 0; k < iters; ++k) {
        double dq[N], dp[N];
        ham_eqs<S, S::MODE_H>(zq, zp, dq, dp, st, tc);
        if (k == iters - 1) {                                   // (uniform) the update of the last iteration, for `residual`
#pragma unroll
          for (int j = 0; j < N; ++j) {
            last = fmax(last, fabs(fma(hh, dq[j], yq[j]) - zq[j]) / fmax(1.0, fabs(yq[j])));
            last = fmax(last, fabs(fma(hh, dp[j], yp[j]) - zp[j]) / fmax(1.0, fabs(yp[j])));
          }
        }
#pragma unroll
        for (int j = 0; j < N; ++j) { zq[j] = fma(hh, dq[j], yq[j]); zp[j] = fma(hh, dp[j], yp[j]); }
      }
      res = fmax(res, last);
#pragma unroll
      for (int j = 0; j < N; ++j) { yq[j] = fma(2.0, zq[j], -yq[j]); yp[j] = fma(2.0, zp[j], -yp[j]); }
    }
  }
  bool bad = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[(i64)j * B + i] = yq[j];
    p[(i64)j * B + i] = yp[j];
    bad = bad || is_nonfinite_bits(yq[j]) || is_nonfinite_bits(yp[j]);
  }
  if (bad) st |= ST_NONFINITE;
  if (residual) residual[i] = res;
  if (status) status[i] = st;
}

}  // namespace hamk

// The one kernel of the companion module.  Plain __launch_bounds__(256): no "1 wave per SIMD" hint (the note above
// HAMK_RK4_BOUNDS in hamk_device.hpp).
#define HAMK_INSTANTIATE_SYMP(S)                                                                                  \
  extern "C" __global__ void __launch_bounds__(256) hamk_symp_steps_k(double* q, double* p, long long B,          \
                                                                       int nsteps, int nsub, double ha, double hb, \
                                                                       int iters, double* residual, int* status) { \
    hamk::symp_body<S>(q, p, B, nsteps, nsub, ha, hb, iters, residual, status);                                   \
  }
