// hamk_lyap.hpp -- largest-Lyapunov-exponent stepping fused with classic RK4 on the lane mapping (one trajectory per lane,
// n <= 16): Benettin's two-trajectory method.  No reference counterpart.
//
// Per trajectory: the state y = [q; p], a deviation vector w = [wq; wp] and a running logsum.  One interval:
//     1.  s = y + d0 w                                       (one fma per component)
//     2.  `every` times:  y <- RK4(y, dt);  s <- RK4(s, dt)
//     3.  delta = s - y;  d = sqrt(sum_j delta_j^2);  logsum += log(d / d0);  w = delta / d
// A launch runs `nintervals` intervals; the largest Lyapunov exponent estimate is logsum / (nintervals every dt), the host's
// division.  y, w and logsum are loaded once, live in registers for the whole launch and are stored once.
//
// w is used EXACTLY AS GIVEN: the kernel does not normalise it at entry.  A unit vector (Euclidean norm over all 2n components)
// is the caller's business; a w of norm c adds log c to the first term of logsum.  That, and logsum being read, added to and
// written back (the adds happen in the same order however a run is cut), is what makes a run cut into calls -- w and logsum
// carried over -- reproduce the one-call bits.
//
// The two trajectories go through ONE copy of the step: the inner loop advances `a` and then exchanges a and b, twice per step,
// so the main trajectory's arithmetic is the shadow's instruction for instruction and depends on neither w nor d0.  The step
// is hamk_fused_rk4.hpp's HAMK_RK4_STAGES, which states the right-hand side and the rolled stage loop; the loops over intervals, steps
// and the two trajectories stay rolled as well: one copy of the right-hand side, code size independent of the arguments.
//
// status: the OR of HAMK_ST_SINGULAR of every right-hand side (both trajectories), HAMK_ST_NONFINITE where the final state, w or
// logsum is not finite (d = 0 gives log 0 = -inf and w = 0 / 0, flagged this way).
//
// This header rides beside hamk_device.hpp in a COMPANION module of the lane variant (hamk_build.cpp build_companion): the
// variant's generated source with its HAMK_INSTANTIATE(HamkSys) replaced by HAMK_INSTANTIATE_LYAP(HamkSys).
#pragma once
#include "hamk_fused_rk4.hpp"

namespace hamk {

template <class S>
HAMK_DEV void lyap_body(double* __restrict__ q, double* __restrict__ p, double* __restrict__ wq, double* __restrict__ wp, i64 B,
                        double dt, int nintervals, int every, double d0, double* __restrict__ logsum, int* __restrict__ status) {
  constexpr int N = S::N;
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double aq[N], ap[N], bq[N], bp[N];                          // a: the trajectory being advanced; b: the one that waits
#pragma unroll
  for (int j = 0; j < N; ++j) {
    aq[j] = q[(i64)j * B + i]; ap[j] = p[(i64)j * B + i];
    bq[j] = wq[(i64)j * B + i]; bp[j] = wp[(i64)j * B + i];   // (w until the first interval turns it into the shadow)
  }
  double ls = logsum[i];
  int st = 0;
  TrigCache<S::NTRIG_F> tc;
  const double h2 = 0.5 * dt, h6 = dt * (1.0 / 6.0), h3 = dt * (1.0 / 3.0);
#pragma unroll 1
  for (int iv = 0; iv < nintervals; ++iv) {
#pragma unroll
    for (int j = 0; j < N; ++j) { bq[j] = fma(d0, bq[j], aq[j]); bp[j] = fma(d0, bp[j], ap[j]); }
#pragma unroll 1
    for (int s = 0; s < every; ++s) {
#pragma unroll 1
      for (int t = 0; t < 2; ++t) {                           // t = 0: a is y, b is s; t = 1: the other way round
        double kq[N], kp[N], cq[N], cp[N];
        HAMK_RK4_STAGES(S, 0, aq, ap, dt, h2, h6, h3, kq, kp, cq, cp, kq, kp, kq, kp, st, tc)   // not dense: the four placeholders
#pragma unroll
        for (int j = 0; j < N; ++j) {                         // the advanced one goes to wait, the other one is next
          aq[j] = bq[j]; ap[j] = bp[j];
          bq[j] = cq[j]; bp[j] = cp[j];
        }
      }
    }
    double d2 = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) { bq[j] -= aq[j]; d2 = fma(bq[j], bq[j], d2); }
#pragma unroll
    for (int j = 0; j < N; ++j) { bp[j] -= ap[j]; d2 = fma(bp[j], bp[j], d2); }
    const double d = ::sqrt(d2);
    ls += ::log(d / d0);
#pragma unroll
    for (int j = 0; j < N; ++j) { bq[j] = bq[j] / d; bp[j] = bp[j] / d; }
  }
  bool bad = is_nonfinite_bits(ls);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[(i64)j * B + i] = aq[j];
    p[(i64)j * B + i] = ap[j];
    wq[(i64)j * B + i] = bq[j];
    wp[(i64)j * B + i] = bp[j];
    bad = bad || is_nonfinite_bits(aq[j]) || is_nonfinite_bits(ap[j]) || is_nonfinite_bits(bq[j]) || is_nonfinite_bits(bp[j]);
  }
  logsum[i] = ls;
  if (bad) st |= ST_NONFINITE;
  if (status) status[i] = st;
}

}  // namespace hamk

// The one kernel of the companion module.  Plain __launch_bounds__(256), as hamk_symp.hpp's.
#define HAMK_INSTANTIATE_LYAP(S)                                                                                      \
  extern "C" __global__ void __launch_bounds__(256) hamk_lyap_steps_k(double* q, double* p, double* wq, double* wp,   \
                                                                       long long B, double dt, int nintervals,        \
                                                                       int every, double d0, double* logsum,          \
                                                                       int* status) {                                 \
    hamk::lyap_body<S>(q, p, wq, wp, B, dt, nintervals, every, d0, logsum, status);                                   \
  }
