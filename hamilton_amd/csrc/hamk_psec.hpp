// hamk_psec.hpp -- Poincare sections fused with classic RK4 on the lane mapping (one trajectory per lane, n <= 16): the crossings of
// one component of y = [q; p] through a surface, located inside the step and recorded inside the launch.  No reference counterpart.
//
// Per trajectory: the state y and a hit count.  One step:
//     1.  y1 = RK4(y0, dt), keeping k1 and k2 + k3 beside the accumulator (k4 is what the last stage leaves in k)
//     2.  the cell index of the section component yc (coord < n: q[coord], otherwise p[coord - n]) before and after:
//             c(y) = floor((yc - level) / period)   (period > 0: the family yc = level mod period)
//             c(y) = yc >= level ? 0 : -1           (period == 0: the plane yc = level)
//         kept as a double.  Upward: c(y1) > c(y0), target = level + c(y1) period; downward: c(y1) < c(y0), target = level +
//         c(y0) period.  direction +1 / -1 / 0 counts upward / downward / both; at most ONE crossing per step (dt is expected
//         to resolve the motion).  A step with a non-finite yc at either end records nothing.
//     3.  on a crossing: theta in [0, 1] with Yc(theta) = target on RK4's own third-order continuous extension Y(theta), by
//         hamk_fused_rk4.hpp's dense_root (that header states Y and the iteration).  The hit is Y(theta) in all 2n components --
//         the section component as computed, not snapped to the target -- and goes to row nhit of qhit / phit [max_hits][n][B]
//         and thit [max_hits][B] IF that row exists; nhit counts it either way, so nhit > max_hits is how a caller learns of an
//         overflow.  thit = (double)(step0 + step index) + theta, in units of dt.
// y and nhit are loaded once, live in registers for the whole launch and are stored once.  nhit is read, added to and written
// back, and both summands of thit are the same whichever way a run is cut: N steps in one call equal N1 + N2 in two calls with
// step0 = N1 and the buffers carried over, bit for bit.  The state's arithmetic does not involve the surface: q, p do not depend
// on coord, level, period, direction or max_hits.
//
// The step is hamk_fused_rk4.hpp's HAMK_RK4_STAGES in its dense form and the section component is picked by its dense_component;
// the step loop stays rolled as the stage loop does: one copy of the right-hand side.  The crossing branch is lane-divergent and
// holds arithmetic and stores only.
//
// The hit store is the one place that writes beyond what a lane owns by its index alone: the row comes from nhit, memory of the
// caller's, so it is stored only where (unsigned)row < (unsigned)max_hits, and its index ((i64)row N + j) B + i is 64-bit.
//
// status: the OR of HAMK_ST_SINGULAR of every right-hand side, HAMK_ST_NONFINITE where the final state is not finite.
//
// This header rides beside hamk_device.hpp in a COMPANION module of the lane variant (hamk_build.cpp build_companion): the
// variant's generated source with its HAMK_INSTANTIATE(HamkSys) replaced by HAMK_INSTANTIATE_PSEC(HamkSys).
#pragma once
#include "hamk_fused_rk4.hpp"

namespace hamk {

// the cell index of a FINITE section component, a double
HAMK_DEV double psec_cell(double yc, double level, double period) {
  return period > 0.0 ? ::floor((yc - level) / period) : (yc >= level ? 0.0 : -1.0);
}

template <class S>
HAMK_DEV void psec_body(double* __restrict__ q, double* __restrict__ p, i64 B, double dt, int nsteps, int coord, double level,
                        double period, int direction, int max_hits, double* __restrict__ qhit, double* __restrict__ phit,
                        double* __restrict__ thit, int* __restrict__ nhit, i64 step0, int* __restrict__ status) {
  constexpr int N = S::N;
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double aq[N], ap[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { aq[j] = q[(i64)j * B + i]; ap[j] = p[(i64)j * B + i]; }
  int cnt = nhit[i];
  int st = 0;
  TrigCache<S::NTRIG_F> tc;
  const double h2 = 0.5 * dt, h6 = dt * (1.0 / 6.0), h3 = dt * (1.0 / 3.0);
#pragma unroll 1
  for (int s = 0; s < nsteps; ++s) {
    double kq[N], kp[N], cq[N], cp[N], k1q[N], k1p[N], k23q[N], k23p[N];
    HAMK_RK4_STAGES(S, 1, aq, ap, dt, h2, h6, h3, kq, kp, cq, cp, k1q, k1p, k23q, k23p, st, tc)
    // the section component before and after, and its three slopes (k4 is in k): coord is wave-uniform
    double y0c, y1c, k1c, k23c, k4c;
    dense_component<N>(coord, aq, ap, cq, cp, k1q, k1p, k23q, k23p, kq, kp, y0c, y1c, k1c, k23c, k4c);
    if (!is_nonfinite_bits(y0c) && !is_nonfinite_bits(y1c)) {
      const double c0 = psec_cell(y0c, level, period), c1 = psec_cell(y1c, level, period);
      const bool up = c1 > c0 && direction >= 0, down = c1 < c0 && direction <= 0;
      if (up || down) {                                        // lane-divergent: arithmetic and stores only
        const double target = fma(up ? c1 : c0, period, level);
        const double th = dense_root(y0c, y1c, k1c, k23c, k4c, target, dt);
        const int row = cnt;
        cnt = (int)((unsigned)cnt + 1u);
        if ((unsigned)row < (unsigned)max_hits) {
          const double t2 = th * th, t3 = t2 * th;                 // dense_weights(th), in place: hamk_fused_rk4.hpp says why
          const double b1 = th - 1.5 * t2 + (2.0 / 3.0) * t3, b2 = t2 - (2.0 / 3.0) * t3, b4 = (2.0 / 3.0) * t3 - 0.5 * t2;
#pragma unroll
          for (int j = 0; j < N; ++j) {
            const i64 at = ((i64)row * N + j) * B + i;
            qhit[at] = aq[j] + dt * (b1 * k1q[j] + b2 * k23q[j] + b4 * kq[j]);
            phit[at] = ap[j] + dt * (b1 * k1p[j] + b2 * k23p[j] + b4 * kp[j]);
          }
          if (thit) thit[(i64)row * B + i] = (double)(step0 + (i64)s) + th;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) { aq[j] = cq[j]; ap[j] = cp[j]; }
  }
  bool bad = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[(i64)j * B + i] = aq[j];
    p[(i64)j * B + i] = ap[j];
    bad = bad || is_nonfinite_bits(aq[j]) || is_nonfinite_bits(ap[j]);
  }
  nhit[i] = cnt;
  if (bad) st |= ST_NONFINITE;
  if (status) status[i] = st;
}

}  // namespace hamk

// The one kernel of the companion module.  Plain __launch_bounds__(256), as hamk_symp.hpp's and hamk_lyap.hpp's.
#define HAMK_INSTANTIATE_PSEC(S)                                                                                      \
  extern "C" __global__ void __launch_bounds__(256) hamk_psec_steps_k(double* q, double* p, long long B, double dt,   \
                                                                       int nsteps, int coord, double level,           \
                                                                       double period, int direction, int max_hits,    \
                                                                       double* qhit, double* phit, double* thit,      \
                                                                       int* nhit, long long step0, int* status) {     \
    hamk::psec_body<S>(q, p, B, dt, nsteps, coord, level, period, direction, max_hits, qhit, phit, thit, nhit, step0, \
                       status);                                                                                       \
  }
