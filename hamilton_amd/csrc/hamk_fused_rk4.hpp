// hamk_fused_rk4.hpp -- what the kernels fused with classic RK4 on the lane mapping share (hamk_lyap.hpp, hamk_psec.hpp,
// hamk_exit.hpp): the rolled four-stage step (HAMK_RK4_STAGES, at the end), and RK4's continuous extension with the root finder
// on it.  Everything works on arrays that the CALLER declares -- nothing here owns state, so each body keeps its own register
// layout -- and is arithmetic only:
//     NO BARRIER AND NO LDS MAY APPEAR IN THIS HEADER
// (hamk_exit.hpp calls it from inside a step loop that the wavefronts of one block leave at different steps).
//
// The step.  The right-hand side is ham_eqs<S, S::MODE_H> with its default TRIG_FULL, the instantiation of hamk_hameqs_k and
// hamk_symp_steps_k: no LDS table.  The stage loop stays rolled -- one copy of the right-hand side, the stage's coefficients by
// scalar selects on the wave-uniform stage index -- and so do the caller's loops around it.  Where the caller wants dense output,
// k1 and k2 + k3 are kept beside the accumulator by selects on the same index (k4 is what the last stage leaves in k): no register
// array is indexed at run time.
//
// The continuous extension.  RK4's own third-order one,
//     Y(theta) = y0 + dt [b1 k1 + b2 (k2 + k3) + b4 k4],   b1 = theta - 3 theta^2 / 2 + 2 theta^3 / 3,
//                                                          b2 = theta^2 - 2 theta^3 / 3,  b4 = -theta^2 / 2 + 2 theta^3 / 3
// needs no extra right-hand side and no state carried between steps; Y(1) is the RK4 step.  theta in [0, 1] with Yc(theta) =
// target for ONE component c comes from the secant value (target - y0c) / (y1c - y0c) by a FIXED number of Newton iterations
// (kDenseNewton = 4), theta clamped to [0, 1] after each, a non-finite update leaving theta as it was: known cost, no lane can
// spin.  The component is picked by scalar selects on the wave-uniform coord (coord < n: q[coord], otherwise p[coord - n]).
#pragma once
#include "hamk_device.hpp"

namespace hamk {

constexpr int kDenseNewton = 4;

// component coord of y = [q; p] before (a) and after (c) a dense step, and its three slopes: coord is wave-uniform
template <int N>
HAMK_DEV void dense_component(int coord, const double (&aq)[N], const double (&ap)[N], const double (&cq)[N], const double (&cp)[N],
                              const double (&k1q)[N], const double (&k1p)[N], const double (&k23q)[N], const double (&k23p)[N],
                              const double (&kq)[N], const double (&kp)[N], double& y0c, double& y1c, double& k1c, double& k23c,
                              double& k4c) {
  y0c = 0.0; y1c = 0.0; k1c = 0.0; k23c = 0.0; k4c = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool isq = coord == j, isp = coord == j + N;
    y0c = isq ? aq[j] : (isp ? ap[j] : y0c);
    y1c = isq ? cq[j] : (isp ? cp[j] : y1c);
    k1c = isq ? k1q[j] : (isp ? k1p[j] : k1c);
    k23c = isq ? k23q[j] : (isp ? k23p[j] : k23c);
    k4c = isq ? kq[j] : (isp ? kp[j] : k4c);
  }
}

// the weights of Y(theta): Y = y0 + dt (b1 k1 + b2 k23 + b4 k4).  dense_root's; the hit store of hamk_psec.hpp and the exit store of
// hamk_exit.hpp spell the same three lines out in place, for HAMK_RK4_STAGES' reason: with this call there, chain8's state left an
// MI355X with other last bits.
HAMK_DEV void dense_weights(double th, double& b1, double& b2, double& b4) {
  const double t2 = th * th, t3 = t2 * th;
  b1 = th - 1.5 * t2 + (2.0 / 3.0) * t3; b2 = t2 - (2.0 / 3.0) * t3; b4 = (2.0 / 3.0) * t3 - 0.5 * t2;
}

// theta in [0, 1] with Yc(theta) = target
HAMK_DEV double dense_root(double y0c, double y1c, double k1c, double k23c, double k4c, double target, double dt) {
  double th = ::fmin(1.0, ::fmax(0.0, (target - y0c) / (y1c - y0c)));      // the secant value, in [0, 1] but for rounding
#pragma unroll
  for (int it = 0; it < kDenseNewton; ++it) {
    const double t2 = th * th;
    double b1, b2, b4;
    dense_weights(th, b1, b2, b4);
    const double d1 = 1.0 - 3.0 * th + 2.0 * t2, d2 = 2.0 * th - 2.0 * t2, d4 = 2.0 * t2 - th;
    const double g = (y0c - target) + dt * (b1 * k1c + b2 * k23c + b4 * k4c);
    const double dg = dt * (d1 * k1c + d2 * k23c + d4 * k4c);
    const double tn = th - g / dg;
    th = is_nonfinite_bits(tn) ? th : ::fmin(1.0, ::fmax(0.0, tn));
  }
  return th;
}

}  // namespace hamk

// c = RK4(a, dt), with h2 = dt / 2, h6 = dt / 6, h3 = dt / 3 as the caller computed them once; k is left holding k4.  DENSE (0 or 1): k1
// and k23 = k2 + k3 are kept as well; with DENSE 0 the four arrays are not touched and any array serves as a placeholder.  st collects
// the right-hand sides' status bits.
//
// A MACRO, the one thing here that is not a function.  As a function -- in every form tried: template, plain, lambda, with the
// k = 0 / c = a loop inside or outside -- the right-hand side is inlined and simplified inside that function first, with the arrays
// as memory, and only then inside the kernel body; ham_eqs' values then reach the re-association of its `reassociate(on)` sums and
// the contraction into fmas in another order.  Registers and spills stayed where they were, but chain8's state came out of an MI355X
// with other last bits (up to 64 ulp on thit / texit after 300 steps).  Expanded in place the body is token for token what each
// kernel had, and so are the bits.
#define HAMK_RK4_STAGES(S, DENSE, aq, ap, dt, h2, h6, h3, kq, kp, cq, cp, k1q, k1p, k23q, k23p, st, tc)                      \
  {                                                                                                                        \
    _Pragma("unroll") for (int j = 0; j < S::N; ++j) {                                                                     \
      kq[j] = 0.0; kp[j] = 0.0; cq[j] = aq[j]; cp[j] = ap[j];                                                              \
      if constexpr (DENSE) { k1q[j] = 0.0; k1p[j] = 0.0; k23q[j] = 0.0; k23p[j] = 0.0; }                                   \
    }                                                                                                                      \
    _Pragma("unroll 1") for (int sg = 0; sg < 4; ++sg) {                                                                   \
      const double a = (sg == 0) ? 0.0 : ((sg == 3) ? dt : h2);   /* wave-uniform: scalar selects */                       \
      const double b = (sg == 0 || sg == 3) ? h6 : h3;                                                                     \
      double yq[S::N], yp[S::N];                                                                                           \
      _Pragma("unroll") for (int j = 0; j < S::N; ++j) { yq[j] = fma(a, kq[j], aq[j]); yp[j] = fma(a, kp[j], ap[j]); }     \
      hamk::ham_eqs<S, S::MODE_H>(yq, yp, kq, kp, st, tc);                                                                 \
      _Pragma("unroll") for (int j = 0; j < S::N; ++j) {                                                                   \
        cq[j] = fma(b, kq[j], cq[j]); cp[j] = fma(b, kp[j], cp[j]);                                                        \
        if constexpr (DENSE) {                                                                                             \
          k1q[j] = (sg == 0) ? kq[j] : k1q[j]; k1p[j] = (sg == 0) ? kp[j] : k1p[j];                     /* k1 */           \
          const double sq = k23q[j] + kq[j], sp = k23p[j] + kp[j];                                                         \
          k23q[j] = (sg == 1) ? kq[j] : ((sg == 2) ? sq : k23q[j]);                          /* k2, then k2 + k3 */        \
          k23p[j] = (sg == 1) ? kp[j] : ((sg == 2) ? sp : k23p[j]);                                                        \
        }                                                                                                                  \
      }                                                                                                                    \
    }                                                                                                                      \
  }
