// hamk_exit.hpp -- first-exit times fused with classic RK4 on the lane mapping (one trajectory per lane, n <= 16): when, and through
// which bound, each trajectory first leaves a box of up to four gates; a trajectory that has left stops, and a wavefront whose
// trajectories have all stopped leaves the step loop.  No reference counterpart.
//
// Per trajectory: the state y, a code (HAMK_EXIT_ALIVE = -1 running; 2 g + side >= 0 stopped by gate g through its lower (side 0) or
// upper (side 1) bound; HAMK_EXIT_NONFINITE = -2 stopped because the state stopped being finite) and an exit time.  A lane is ALIVE
// iff its code at entry is exactly -1.  One step of an alive lane:
//     1.  y1 = RK4(y0, dt), keeping k1 and k2 + k3 beside the accumulator (k4 is what the last stage leaves in k)
//     2.  any component of y1 not finite: code = -2, texit = step0 + step index + 1, ST_NONFINITE, the exit state untouched
//     3.  otherwise every gate g (a component c_g of y = [q; p] and a closed interval [lo_g, hi_g]) FIRES where y1[c_g] < lo_g or
//         y1[c_g] > hi_g; its target is the violated bound.  theta_g in [0, 1] with Y_c(theta) = target on RK4's own third-order
//         continuous extension, by hamk_fused_rk4.hpp's dense_root (that header states Y and the iteration); a component
//         already outside [lo_g, hi_g] at y0 (an alive lane's first step only) has theta_g = 0.  The firing gate with the smallest
//         theta wins, on a tie the lowest index: code = 2 g + side, texit = (double)(step0 + step index) + theta, in units of dt,
//         and qexit, pexit receive Y(theta) in all 2n components -- the gate component as computed, not snapped to the bound
//     4.  y = y1 either way: a stopped lane holds the END of its exit step and is never advanced again
// A lane stopped at entry is not read beyond its code and no memory of its is written, but status (0).  Inside a running wavefront
// a stopped lane commits nothing: every state update is a select on `alive`, ST_SINGULAR of a right-hand side is OR-ed in for alive
// lanes only.  After every step `if (__ballot(alive) == 0) break;` -- a wave-uniform scalar branch -- drops the wavefront's remaining
// steps; a wavefront with no alive lane at entry runs none.  Wavefronts of one block leave at different steps:
//     NO BLOCK-WIDE BARRIER AND NO LDS MAY APPEAR INSIDE THE STEP LOOP (a barrier there would hang the block).
// What the loop calls in hamk_fused_rk4.hpp (the step, the component select, the root finder) needs neither.
//
// texit's two summands are the same whichever way a run is cut and code / texit / the exit state are read, updated and written
// back: N steps in one call equal N1 + N2 in two calls with step0 = N1 and the arrays carried over, bit for bit.  While a lane is
// alive its state's arithmetic does not involve the gates, nor any other lane.
//
// The step loop and the gate loop stay rolled, as the stage loop does: one copy of the right-hand side, one of Newton.  A gate's
// bounds and component are picked by scalar selects on the wave-uniform gate index: no register array is indexed at run time.  The
// gates arrive BY VALUE (HamkGates, as HamkBoxes does for hamk_sample_k).  Every store uses the lane's own index only, (i64)j * B + i.
//
// This header rides beside hamk_device.hpp in a COMPANION module of the lane variant (hamk_build.cpp build_companion): the
// variant's generated source with its HAMK_INSTANTIATE(HamkSys) replaced by HAMK_INSTANTIATE_EXIT(HamkSys).
#pragma once
#include "hamk_fused_rk4.hpp"

struct HamkGates { double lo[4], hi[4]; int coord[4]; int ngates; int reserved; };   // HAMK_EXIT_MAX_GATES = 4 (hamk.h); by value

namespace hamk {

constexpr int kExitAlive = -1, kExitNonfinite = -2;

template <class S>
HAMK_DEV void exit_body(double* __restrict__ q, double* __restrict__ p, i64 B, double dt, int nsteps, const HamkGates& gates,
                        int* __restrict__ code, double* __restrict__ texit, double* __restrict__ qexit, double* __restrict__ pexit,
                        i64 step0, int* __restrict__ status) {
  constexpr int N = S::N;
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const bool entered = code[i] == kExitAlive;
  bool alive = entered;                                        // a lane mask: code and texit are stored where the lane stops
  double aq[N], ap[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { aq[j] = 0.0; ap[j] = 0.0; }
  if (entered) {
#pragma unroll
    for (int j = 0; j < N; ++j) { aq[j] = q[(i64)j * B + i]; ap[j] = p[(i64)j * B + i]; }
  }
  int st = 0;
  TrigCache<S::NTRIG_F> tc;
  const double h2 = 0.5 * dt, h6 = dt * (1.0 / 6.0), h3 = dt * (1.0 / 3.0);
#pragma unroll 1
  for (int s = 0; s < nsteps; ++s) {
    if (__ballot(alive) == 0) break;                           // wave-uniform: nothing left to do in this wavefront
    double kq[N], kp[N], cq[N], cp[N], k1q[N], k1p[N], k23q[N], k23p[N];
    int sst = 0;
    HAMK_RK4_STAGES(S, 1, aq, ap, dt, h2, h6, h3, kq, kp, cq, cp, k1q, k1p, k23q, k23p, sst, tc)
    bool stops = false;
    if (alive) {                                               // lane-divergent: arithmetic and stores only
      st |= sst;
      bool bad = false;
#pragma unroll
      for (int j = 0; j < N; ++j) bad = bad || is_nonfinite_bits(cq[j]) || is_nonfinite_bits(cp[j]);
      if (bad) {
        code[i] = kExitNonfinite;
        texit[i] = (double)(step0 + (i64)s + 1);
        st |= ST_NONFINITE;
        stops = true;
      } else {
        double best = 2.0;                                     // above every theta
        int won = -1;
#pragma unroll 1
        for (int g = 0; g < gates.ngates; ++g) {
          // the gate, by scalar selects on the wave-uniform g; its component before and after and the three slopes, on coord
          const int coord = g == 0 ? gates.coord[0] : (g == 1 ? gates.coord[1] : (g == 2 ? gates.coord[2] : gates.coord[3]));
          const double lo = g == 0 ? gates.lo[0] : (g == 1 ? gates.lo[1] : (g == 2 ? gates.lo[2] : gates.lo[3]));
          const double hi = g == 0 ? gates.hi[0] : (g == 1 ? gates.hi[1] : (g == 2 ? gates.hi[2] : gates.hi[3]));
          double y0c, y1c, k1c, k23c, k4c;
          dense_component<N>(coord, aq, ap, cq, cp, k1q, k1p, k23q, k23p, kq, kp, y0c, y1c, k1c, k23c, k4c);
          const bool below = y1c < lo, above = y1c > hi;
          if (below || above) {
            const double target = below ? lo : hi;
            double th = dense_root(y0c, y1c, k1c, k23c, k4c, target, dt);
            th = (y0c < lo || y0c > hi) ? 0.0 : th;            // outside already at y0: the step's start
            const bool wins = th < best;                       // strict: on a tie the lower index stays
            best = wins ? th : best;
            won = wins ? 2 * g + (above ? 1 : 0) : won;
          }
        }
        if (won >= 0) {
          stops = true;
          code[i] = won;
          texit[i] = (double)(step0 + (i64)s) + best;
          if (qexit) {
            const double t2 = best * best, t3 = t2 * best;         // dense_weights(best), in place: hamk_fused_rk4.hpp says why
            const double b1 = best - 1.5 * t2 + (2.0 / 3.0) * t3, b2 = t2 - (2.0 / 3.0) * t3, b4 = (2.0 / 3.0) * t3 - 0.5 * t2;
#pragma unroll
            for (int j = 0; j < N; ++j) {
              qexit[(i64)j * B + i] = aq[j] + dt * (b1 * k1q[j] + b2 * k23q[j] + b4 * kq[j]);
              pexit[(i64)j * B + i] = ap[j] + dt * (b1 * k1p[j] + b2 * k23p[j] + b4 * kp[j]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) { aq[j] = alive ? cq[j] : aq[j]; ap[j] = alive ? cp[j] : ap[j]; }
    alive = alive && !stops;
  }
  if (entered) {
#pragma unroll
    for (int j = 0; j < N; ++j) { q[(i64)j * B + i] = aq[j]; p[(i64)j * B + i] = ap[j]; }
  }
  if (status) status[i] = st;
}

}  // namespace hamk

// The one kernel of the companion module.  Plain __launch_bounds__(256), as hamk_symp.hpp's, hamk_lyap.hpp's and hamk_psec.hpp's.
#define HAMK_INSTANTIATE_EXIT(S)                                                                                      \
  extern "C" __global__ void __launch_bounds__(256) hamk_exit_steps_k(double* q, double* p, long long B, double dt,   \
                                                                       int nsteps, HamkGates gates, int* code,        \
                                                                       double* texit, double* qexit, double* pexit,   \
                                                                       long long step0, int* status) {                \
    hamk::exit_body<S>(q, p, B, dt, nsteps, gates, code, texit, qexit, pexit, step0, status);                         \
  }
