// hamk_rec.hpp -- trajectory recording fused with classic RK4 on the lane mapping (one trajectory per lane, n <= 16): the state
// and / or the Hamiltonian on a grid of steps, written to fixed-size row buffers from inside one launch.  The fixed-step counterpart
// of evolveHam's rows (Hamilton.hs:433-462), which here only the adaptive stepper records.
//
// Per trajectory: the state y = [q; p].  G counts the steps of the whole run: step0 at entry, step0 + s + 1 after the call's step s.
// Where G is a multiple of `every`, the state after G steps is ROW k = G / every:
//     at entry       row 0 = the state as given, bit for bit, and only where step0 == 0
//     after a step   row G / every, for every G in (step0, step0 + nsteps] that `every` divides
// A row k >= max_rows is dropped; rows outside this call's range are never written.  Row k of qout / pout is an [n][B] block at
// (k - row_base) n B -- row_base is the row the three pointers point at: 0 for the caller's whole buffers, the call's first row where
// the host staged only the rows this call fills -- and hout[k - row_base][B] receives energy<S> (hamk_device.hpp: velocities +
// potential_value) of the recorded state.  qout / pout (both or neither) and hout may be null; energy<S> is evaluated only where a
// row is recorded and hout is given.  The kernel never reads the row buffers.
//
// "Is this step recorded, and to which row" does not depend on the lane: a countdown to the next recorded step, the rows still to
// fill and the row's start -- one 64-bit offset into qout / pout advanced by n B per recorded row, one into hout advanced by B -- all
// wave-uniform scalars; the one 64-bit division is at entry.  The stores sit at the top of the step loop, one copy of them and of energy<S> serving row 0 and every later row, behind
// that wave-uniform branch; the step never looks at them, so the final q, p do not depend on every, max_rows or which outputs are
// given, and N steps in one call equal N1 + N2 in two calls with step0 = N1, bit for bit on q, p and every row.
//
// The step is hamk_fused_rk4.hpp's HAMK_RK4_STAGES without dense output, as hamk_lyap.hpp uses it: that header states the
// right-hand side and the rolled stage loop.  The step loop stays rolled: one copy of the right-hand side.  Every store uses the
// lane's own index only, (i64)j * B + i within the row; every row offset is 64-bit.  No LDS, no barrier.
//
// status: the OR of HAMK_ST_SINGULAR of every right-hand side and of energy<S>'s solve, HAMK_ST_NONFINITE where the final state is
// not finite.  A non-finite lane's rows hold what the arithmetic gives.
//
// This header rides beside hamk_device.hpp in a COMPANION module of the lane variant (hamk_build.cpp build_companion): the
// variant's generated source with its HAMK_INSTANTIATE(HamkSys) replaced by HAMK_INSTANTIATE_REC(HamkSys).
#pragma once
#include "hamk_fused_rk4.hpp"

namespace hamk {

// A value that is the same in every lane, moved to scalar registers.  The row rule's one 64-bit division has no scalar form: the
// compiler expands it on the vector unit, and without this the countdown and the branch on it stay there for every step.
HAMK_DEV int wave_uniform(int x) {
#ifdef HAMK_HOST_EMULATION                                 // tests/host_emulation: a wavefront is one thread
  return x;
#else
  return __builtin_amdgcn_readfirstlane(x);
#endif
}
HAMK_DEV i64 wave_uniform(i64 x) {
  const unsigned lo = (unsigned)wave_uniform((int)(unsigned)((unsigned long long)x & 0xffffffffull));
  const unsigned hi = (unsigned)wave_uniform((int)(unsigned)((unsigned long long)x >> 32));
  return (i64)(((unsigned long long)hi << 32) | lo);
}

template <class S>
HAMK_DEV void rec_body(double* __restrict__ q, double* __restrict__ p, i64 B, double dt, int nsteps, int every, int max_rows,
                       double* __restrict__ qout, double* __restrict__ pout, double* __restrict__ hout, i64 step0, i64 row_base,
                       int* __restrict__ status) {
  constexpr int N = S::N;
  const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double aq[N], ap[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { aq[j] = q[(i64)j * B + i]; ap[j] = p[(i64)j * B + i]; }
  int st = 0;
  TrigCache<S::NTRIG_F> tc;
  const double h2 = 0.5 * dt, h6 = dt * (1.0 / 6.0), h3 = dt * (1.0 / 3.0);
  // the row rule, once per launch and the same in every lane: the next row to fill, how many rows are left for it, the steps until
  // it is due
  bool due = step0 == 0;                                       // row 0: the state as given
  const i64 next = due ? 0 : wave_uniform(step0 / every) + 1;
  int cd = every - wave_uniform((int)(step0 % every));
  const i64 room = (i64)max_rows - next;
  int left = room <= 0 ? 0 : (int)room;                        // at most max_rows: fits
  const i64 nb = (i64)N * B;
  // the row to fill as two 64-bit offsets from the kernel's own pointer arguments (so the stores are global ones, not flat): with
  // left > 0, next < max_rows and the offsets stay inside the buffers' 2^48 elements; with no room left nothing is stored
  const i64 at = left > 0 ? next - row_base : 0;
  i64 rs = at * nb, rh = at * B;                               // the row's start in qout / pout, and in hout
#pragma unroll 1
  for (int s = 0;; ++s) {
    if (due && left > 0) {                                     // wave-uniform: a scalar branch round the stores and the energy
      if (qout) {
#pragma unroll
        for (int j = 0; j < N; ++j) { qout[rs + (i64)j * B + i] = aq[j]; pout[rs + (i64)j * B + i] = ap[j]; }
        rs += nb;
      }
      if (hout) {
        double y[2 * N];
#pragma unroll
        for (int j = 0; j < N; ++j) { y[j] = aq[j]; y[N + j] = ap[j]; }
        hout[rh + i] = energy<S>(y, st);
        rh += B;
      }
      --left;
    }
    due = false;
    if (s == nsteps) break;
    double kq[N], kp[N], cq[N], cp[N];
    HAMK_RK4_STAGES(S, 0, aq, ap, dt, h2, h6, h3, kq, kp, cq, cp, kq, kp, kq, kp, st, tc)   // not dense: the four placeholders
#pragma unroll
    for (int j = 0; j < N; ++j) { aq[j] = cq[j]; ap[j] = cp[j]; }
    if (--cd == 0) { due = true; cd = every; }
  }
  bool bad = false;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    q[(i64)j * B + i] = aq[j];
    p[(i64)j * B + i] = ap[j];
    bad = bad || is_nonfinite_bits(aq[j]) || is_nonfinite_bits(ap[j]);
  }
  if (bad) st |= ST_NONFINITE;
  if (status) status[i] = st;
}

}  // namespace hamk

// The one kernel of the companion module.  Plain __launch_bounds__(256), as the other companions'.
#define HAMK_INSTANTIATE_REC(S)                                                                                       \
  extern "C" __global__ void __launch_bounds__(256) hamk_rec_steps_k(double* q, double* p, long long B, double dt,    \
                                                                      int nsteps, int every, int max_rows,            \
                                                                      double* qout, double* pout, double* hout,       \
                                                                      long long step0, long long row_base,            \
                                                                      int* status) {                                  \
    hamk::rec_body<S>(q, p, B, dt, nsteps, every, max_rows, qout, pout, hout, step0, row_base, status);               \
  }
