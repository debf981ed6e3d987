"""CPU: Poincare sections fused with RK4 (hamk_poincare_steps; hamilton_amd/csrc/hamk_psec.hpp) -- its three entry points and their
argument checks, the host's statement of the kernel's signature, the companion module that carries the kernel (compiled for gfx950
here: hiprtc needs no GPU), and the kernel itself run thread by thread on the host (tests/host_emulation/psec_driver.inc appended
to System.poincare_source, the g++ flags of test_lyapunov.py's `emulate`) against a literal numpy restatement of the scheme over the
oracle's hamEqs (below), against two analytic anchors, and for the bit-level properties the scheme promises.  What this cannot see
is the GPU compiler (tests/test_gpu_poincare.py, which imports the restatement, the anchors, the inputs and the bounds from here)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import test_kernel_signatures as KS
from conftest import ROOT
from hamilton_amd import examples as E
from test_gpu_symplectic import STATE_BOUND
from test_lyapunov import relstate, sample_phase

EMU = os.path.join(ROOT, "tests", "host_emulation")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
P = lambda a: None if a is None else a.ctypes.data_as(_dp)
I = lambda a: None if a is None else a.ctypes.data_as(_ip)
LL = ctypes.c_longlong
F = ctypes.c_double
NAMES = ("hamk_poincare_steps", "hamk_poincare_source", "hamk_poincare_build_info")
EPS = 2.2e-16
TWO_PI = 2.0 * np.pi
NEWTON = 4


# ---------------------------------------------------------------------------------------------------------------------- reference
# A LITERAL numpy restatement of the scheme of hamilton_amd/csrc/hamk_psec.hpp over the oracle's hamEqs (the oracle itself is not
# changed).  Per trajectory and step: y1 = RK4(y0); the cell index of the section component before and after
# (c = floor((yc - level) / period), or yc >= level ? 0 : -1 for period == 0); upward where c1 > c0 (target level + c1 period),
# downward where c1 < c0 (target level + c0 period); theta from the secant value by four Newton iterations on the cubic
# Y(theta) = y0 + dt [b1 k1 + b2 (k2 + k3) + b4 k4], clamped to [0, 1] after each, a non-finite update ignored; the hit Y(theta)
# goes to row nhit if 0 <= nhit < max_hits, nhit counts either way; thit = (step0 + step) + theta.
def cell(yc, level, period):
    return np.floor((yc - level) / period) if period > 0 else np.where(yc >= level, 0.0, -1.0)


def surface_distance(yc, level, period):
    """|yc - nearest surface value|."""
    d = yc - level
    return np.abs(d - period * np.round(d / period)) if period > 0 else np.abs(d)


def cubic_weights(th):
    t2, t3 = th * th, th * th * th
    return th - 1.5 * t2 + (2.0 / 3.0) * t3, t2 - (2.0 / 3.0) * t3, (2.0 / 3.0) * t3 - 0.5 * t2


def new_hits(n, nb, max_hits, sentinel=0.0):
    return dict(q=np.full((max_hits, n, nb), sentinel), p=np.full((max_hits, n, nb), sentinel), t=np.full((max_hits, nb), sentinel),
                n=np.zeros(nb, np.int32))


def restate(o, q, p, dt, nsteps, coord, level=0.0, period=0.0, direction=1, max_hits=16, hits=None, step0=0, perturb=None):
    """-> dict(q, p [n, B]; hq, hp [max_hits, n, B]; ht [max_hits, B]; n [B] int32; status [B]; margin [B]: the smallest distance
    of a step end from the surface relative to max(1, |yc|); target [max_hits, B]: the surface value of every stored hit).
    perturb: a numpy Generator -- every hamEqs output is multiplied by 1 +- 1e-12, the signs drawn from it."""
    q, p = np.array(q, dtype=np.float64), np.array(p, dtype=np.float64)
    n, nb = q.shape
    h = new_hits(n, nb, max_hits) if hits is None else {k: np.array(v) for k, v in hits.items()}
    hq, hp, ht, cnt = h["q"], h["p"], h["t"], h["n"].astype(np.int64)
    tgt = np.full((max_hits, nb), np.nan)
    st = np.zeros(nb, np.int32)
    lanes = np.arange(nb)

    def f(a, b):
        dq, dp, s1 = o.hameqs_batch(a, b, threads=1)
        st[:] |= s1
        if perturb is not None:
            dq = dq * (1.0 + 1e-12 * perturb.choice([-1.0, 1.0], size=dq.shape))
            dp = dp * (1.0 + 1e-12 * perturb.choice([-1.0, 1.0], size=dp.shape))
        return np.concatenate([dq, dp])

    y = np.concatenate([q, p])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        margin = surface_distance(y[coord], level, period) / np.maximum(1.0, np.abs(y[coord]))
        for s in range(nsteps):
            k1 = f(y[:n], y[n:])
            y2 = y + 0.5 * dt * k1; k2 = f(y2[:n], y2[n:])
            y3 = y + 0.5 * dt * k2; k3 = f(y3[:n], y3[n:])
            y4 = y + dt * k3; k4 = f(y4[:n], y4[n:])
            y1 = y + dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            k23 = k2 + k3
            y0c, y1c = y[coord], y1[coord]
            fin = np.isfinite(y0c) & np.isfinite(y1c)
            c0, c1 = cell(y0c, level, period), cell(y1c, level, period)
            up, down = fin & (c1 > c0) & (direction >= 0), fin & (c1 < c0) & (direction <= 0)
            hit = up | down
            if hit.any():
                target = level + np.where(up, c1, c0) * period
                th = np.clip((target - y0c) / (y1c - y0c), 0.0, 1.0)
                for _ in range(NEWTON):
                    b1, b2, b4 = cubic_weights(th)
                    g = (y0c - target) + dt * (b1 * k1[coord] + b2 * k23[coord] + b4 * k4[coord])
                    dg = dt * ((1.0 - 3.0 * th + 2.0 * th * th) * k1[coord] + (2.0 * th - 2.0 * th * th) * k23[coord] + (2.0 * th * th - th) * k4[coord])
                    tn = th - g / dg
                    th = np.where(np.isfinite(tn), np.clip(tn, 0.0, 1.0), th)
                b1, b2, b4 = cubic_weights(th)
                yh = y + dt * (b1 * k1 + b2 * k23 + b4 * k4)
                w = lanes[hit & (cnt >= 0) & (cnt < max_hits)]
                hq[cnt[w], :, w] = yh[:n, w].T
                hp[cnt[w], :, w] = yh[n:, w].T
                ht[cnt[w], w] = float(step0 + s) + th[w]
                tgt[cnt[w], w] = target[w]
                cnt[hit] += 1
            y = y1
            margin = np.fmin(margin, surface_distance(y[coord], level, period) / np.maximum(1.0, np.abs(y[coord])))
    st[~np.isfinite(y).all(0)] |= 2
    return dict(q=y[:n].copy(), p=y[n:].copy(), hq=hq, hp=hp, ht=ht, n=cnt.astype(np.int32), status=st, margin=margin, target=tgt)


def stored(r):
    """[max_hits, B] mask of the rows that hold a hit."""
    return np.arange(r["hq"].shape[0])[:, None] < np.minimum(r["n"], r["hq"].shape[0])[None, :]


OUT = ("q", "p", "hq", "hp", "ht", "n")


def same(a, b, keys=OUT):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


# The comparison of the kernel with the restatement: four systems, B = 257 (two blocks, the second holding one lane), dt = 0.02.
#   pendulum:        q[0] through the plane q = 0, both directions
#   doublePendulum:  theta1 = 0 (mod 2 pi), upward: the classical (theta2, p2) section
#   opcodeZoo:       q[0] = 0.0125 (mod 0.05), both directions (a family, crossed in both directions)
#   chain8:          q[3] through the plane q = 0, both directions
# A few hundred steps where the system allows them, and enough that the median lane has two hits in the restatement (asserted):
#   doublePendulum   250: the sample is chaotic -- at 300 steps the restatement's own 1e-12 sensitivity run is 4.4e-8 away from the
#                    oracle's state, beyond the 1e-8 of STATE_BOUND that the state is held to; at 250 it is 7.6e-9
#   opcodeZoo        20: not a physical system -- its potential is unbounded below and every lane of the sampling box has left
#                    the domain of its sqrt / log (NaN) within 100 steps of 0.02, the first six within 25
#   chain8           300, from a SMOOTH SMALL-AMPLITUDE sample (every link at 0.1 sin(..) (1 + 0.15 j), velocities 0.3 cos(..) (1 +
#                    0.15 j)): from test_lyapunov's sample the chain is so sensitive that a 1e-12 perturbation of hamEqs moves the
#                    state by 1e-6 within 100 steps, against STATE_BOUND's 1e-11; near the hanging equilibrium the same
#                    perturbation moves it by 9e-13 in 300 steps.  Smooth, because a random shape excites the chain's fastest
#                    modes, which steps of 0.02 do not resolve: the step's cubic is then not monotone and four Newton iterations
#                    leave a hit 3e-4 off the surface, in the restatement and the kernel alike
SYSTEMS = ["pendulum", "doublePendulum", "opcodeZoo", "chain8"]
B = 257
DT = 0.02
MAX_HITS = 4                 # fewer rows than opcodeZoo's and chain8's lanes have crossings: the overflow is compared too
MARGIN = 1e-9
CASES = {                    # name -> (nsteps, coord, level, period, direction, seed of the sample)
    "pendulum": (400, 0, 0.0, 0.0, 0, 17),
    "doublePendulum": (250, 0, 0.0, TWO_PI, 1, 17),
    "opcodeZoo": (20, 0, 0.0125, 0.05, 0, 17),
    "chain8": (300, 3, 0.0, 0.0, 0, 17),
}
_reference = {}


def inputs(name, spec, o, seed):
    if name == "chain8":
        lane, shape = np.arange(B, dtype=np.float64)[None, :], (1.0 + 0.15 * np.arange(float(spec.n)))[:, None]
        q = 0.1 * np.sin(1.0 + 0.37 * lane) * shape
        return q, o.to_phase_batch(q, 0.3 * np.cos(2.0 + 0.61 * lane) * shape)
    return sample_phase(spec, o, seed, B)


def surface_args(name):
    nsteps, coord, level, period, direction, _ = CASES[name]
    return dict(coord=coord, level=level, period=period, direction=direction)


def reference(oracle_lib, name):
    """Inputs, the restatement's result and the bounds for a system, computed once and shared by every test of both modules.
    State: the oracle's own rk4_steps_batch.  thit and the hit states: the restatement a second time with every hamEqs output
    multiplied by 1 +- 1e-12 (fixed-seed signs; 1e-12 is the tolerance ladder's own hamEqs figure) -- the
    bound is 4 x the largest |difference| between the two runs, DESIGN.md section 12's method and margin.  A lane is left out of
    the hit comparison only where some step end of the restatement lies within 1e-9 max(1, |yc|) of a surface value: the seeds
    are chosen so that there is none, and that is asserted here."""
    if name not in _reference:
        nsteps, coord, level, period, direction, seed = CASES[name]
        spec = E.get(name)
        o = oracle_lib.OracleSystem(spec)
        q, p = inputs(name, spec, o, seed)
        kw = dict(coord=coord, level=level, period=period, direction=direction, max_hits=MAX_HITS)
        want = restate(o, q, p, DT, nsteps, **kw)
        other = restate(o, q, p, DT, nsteps, perturb=np.random.default_rng(7), **kw)
        assert np.isfinite(want["q"]).all() and np.isfinite(want["p"]).all() and not want["status"].any(), name
        left_out = want["margin"] < MARGIN
        print(name, "lanes left out", int(left_out.sum()), "smallest margin", float(want["margin"].min()), "median hits", float(np.median(want["n"])),
              "most", int(want["n"].max()))
        assert left_out.sum() == 0, (name, np.nonzero(left_out)[0])                 # at most 2 of 257 may be; the seed leaves none
        assert np.median(want["n"]) >= 2, (name, np.median(want["n"]))
        assert np.array_equal(want["n"], other["n"])
        m = stored(want)
        _reference[name] = dict(
            o=o, q=q, p=p, want=want, nsteps=nsteps, kw=kw, left_out=left_out, state=o.rk4_steps_batch(q, p, DT, nsteps),
            t_bound=4.0 * float(np.abs(want["ht"] - other["ht"])[m].max()),
            y_bound=4.0 * float(max(np.abs(want["hq"] - other["hq"])[m[:, None, :].repeat(spec.n, 1)].max(),
                                    np.abs(want["hp"] - other["hp"])[m[:, None, :].repeat(spec.n, 1)].max())))
    return _reference[name]


def residuals(ref, r):
    """(largest |hit_c - target| / max(1, |target|), largest |H(hit) - H0| / max(1, |H0|)) over the stored hits of a result on
    ref's inputs; the targets are the restatement's (the counts agree wherever this is called)."""
    o, want = ref["o"], ref["want"]
    n = ref["q"].shape[0]
    coord = ref["kw"]["coord"]
    m = stored(want)
    h0 = o.observe_batch(ref["q"], ref["p"])[2]
    surf = energy = 0.0
    for row in range(m.shape[0]):
        w = np.nonzero(m[row])[0]
        if not w.size:
            continue
        yc = (r["hq"][row, coord, w] if coord < n else r["hp"][row, coord - n, w])
        t = want["target"][row, w]
        surf = max(surf, float((np.abs(yc - t) / np.maximum(1.0, np.abs(t))).max()))
        h = o.observe_batch(np.ascontiguousarray(r["hq"][row][:, w]), np.ascontiguousarray(r["hp"][row][:, w]))[2]
        energy = max(energy, float((np.abs(h - h0[w]) / np.maximum(1.0, np.abs(h0[w]))).max()))
    return surf, energy


# On the surface: the restatement's own residual is a few ulp of the target (Newton has converged to rounding, DESIGN.md section
# 13), so the bound is 8 x the larger of that residual and one eps.  Energy: the cubic is a third-order interpolant, its energy
# error is the restatement's own figure; the kernel solves the same cubic, so 2 x that.
SURFACE_MARGIN, ENERGY_MARGIN = 8.0, 2.0


def check_against_reference(ref, name, got, what):
    """got: a kernel run on ref's inputs (a dict like restate's): every lane that is not left out, every output.
    Measured (largest over the four systems, all on doublePendulum; the bounds are 4 x the first line's figures; per system in
    DESIGN.md section 13):
        between the two restatement runs      |dthit| 3.4e-8,  |dhit| 5.7e-9
        kernel on the host - restatement      |dthit| 5.3e-11, |dhit| 8.7e-12
        kernel on an MI355X - restatement     |dthit| 5.6e-11, |dhit| 9.2e-12
    """
    want, keep = ref["want"], ~ref["left_out"]
    n = ref["q"].shape[0]
    assert keep.sum() >= B - 2
    state = relstate(got["q"], got["p"], *ref["state"])
    m = stored(want) & keep[None, :]
    mm = m[:, None, :].repeat(n, 1)
    dt_ = float(np.abs(got["ht"] - want["ht"])[m].max())
    dy = float(max(np.abs(got["hq"] - want["hq"])[mm].max(), np.abs(got["hp"] - want["hp"])[mm].max()))
    surf, energy = residuals(ref, got)
    rsurf, renergy = residuals(ref, want)
    print(what, name, "state err", state, "|dthit|", dt_, "bound", ref["t_bound"], "|dhit|", dy, "bound", ref["y_bound"],
          "surface", surf, "restatement's", rsurf, "energy", energy, "restatement's", renergy)
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["n"][keep], want["n"][keep]), np.nonzero(got["n"] != want["n"])[0]
    assert state < STATE_BOUND[name], (name, state)
    assert relstate(want["q"], want["p"], *ref["state"]) < STATE_BOUND[name]
    assert dt_ <= ref["t_bound"], (name, dt_, ref["t_bound"])
    assert dy <= ref["y_bound"], (name, dy, ref["y_bound"])
    assert surf <= SURFACE_MARGIN * max(rsurf, EPS), (name, surf, rsurf)
    assert energy <= ENERGY_MARGIN * renergy, (name, energy, renergy)


# ---- analytic anchors ------------------------------------------------------------------------------------------------
# rotor:      mkSystem([1, 1], f(q) = (cos q, sin q), U = 0, n = 1): K = 1, hamEqs = (p, 0); RK4 and the cubic are exact to
#             rounding: Y(theta) = y0 + theta dt (p, 0).  Section q = 0 (mod 2 pi).  With qN = q0 + N dt p the number of upward
#             crossings is floor(qN / 2 pi) - floor(q0 / 2 pi) where positive, of downward ones its negative; the r-th crossing
#             happens at time (target_r - q0) / p; the stored momentum is p, bit for bit.
#             Bound on |thit dt - t|: every step commits at most 8 roundings relative to |q| (K = cos^2 + sin^2 and its inverse:
#             3; the four stage evaluations' fma and the accumulation: 5 at the most, most of them exact here), so after k steps q
#             is off by at most 8 k eps qmax, which the division by |p| turns into time; Newton's root has the conditioning
#             eps qmax / |p|; thit = step + theta is rounded at eps N.  In all: (8 N + 2) eps qmax / |p| + eps N dt.
# oscillator: mkSystem([1], f(q) = q, U = x^2 / 2): hamEqs = (p, -q) = A y.  The RK4 map is linear, M = [[a, b], [-b, a]],
#             a = 1 - dt^2 / 2 + dt^4 / 24, b = dt - dt^3 / 6, and k1 = A y0, k2 = A (y0 + dt / 2 k1), k3 = A (y0 + dt / 2 k2),
#             k4 = A (y0 + dt k3) are known in closed form, so the cubic's coefficients are; theta is taken from numpy.roots on
#             them (NOT from Newton).  Bound on |theta - root|: the root's conditioning eps ymax / |Y'_c(theta)| times
#             8 (k + 2) at step k -- both the kernel's state and the expected M^k y0 carry at most 8 roundings of size eps ymax
#             per step (as above), and a state error of delta moves the root by delta / |Y'_c|.  The hit state: twice that in y.
ANCHOR_B = 64
ROTOR_DT, ROTOR_N, ROTOR_MAX_HITS = 0.02, 300, 2
OSC_CASES = [(0.1, 100), (0.5, 40)]            # (dt, nsteps)


def anchor_spec(kind):
    if kind == "rotor":
        return E.SystemSpec(name="rotor", m=2, n=1, inertia=(1.0, 1.0), f=lambda q, ops: [ops.cos(q[0]), ops.sin(q[0])],
                            u=lambda z, ops: 0.0 * z[0], u_space=0, q0=(0.0,), qd0=(1.0,))
    return E.SystemSpec(name="oscillator", m=1, n=1, inertia=(1.0,), f=lambda q, ops: [q[0]], u=lambda z, ops: 0.5 * z[0] * z[0],
                        u_space=0, q0=(0.0,), qd0=(0.0,))


_anchor_systems = {}


def anchor_system(kind):
    """The library's handle, by mkSystem (one per kind and process)."""
    from hamilton_amd import api, tracer as T
    if kind not in _anchor_systems:
        if kind == "rotor":
            _anchor_systems[kind] = api.mkSystem([1.0, 1.0], lambda q: [T.cos(q[0]), T.sin(q[0])], lambda q: 0.0 * q[0], 1)
        else:
            _anchor_systems[kind] = api.mkSystem([1.0], lambda q: [q[0]], lambda q: 0.5 * q[0] * q[0], 1)
    return _anchor_systems[kind]


def rotor_inputs():
    """p of both signs, magnitudes 0.25 .. 4 (the fastest lanes cross three to four times in N dt = 6), q0 in (-3, 3)."""
    lane = np.arange(ANCHOR_B)
    p = np.where(lane % 2 == 0, 1.0, -1.0) * (0.25 + 3.75 * (lane // 2) / (ANCHOR_B // 2 - 1))
    q = 2.9 * np.sin(1.0 + 0.7 * lane)
    return q.reshape(1, -1).copy(), p.reshape(1, -1).copy()


def check_rotor(got, direction, what):
    """got: ROTOR_N steps of ROTOR_DT from rotor_inputs(), section q = 0 (mod 2 pi), ROTOR_MAX_HITS rows, sentinel -7 in the hit
    buffers.  -> worst error / bound."""
    q0, p0 = rotor_inputs()
    q0, p0 = q0[0], p0[0]
    qn = q0 + ROTOR_N * ROTOR_DT * p0
    assert (surface_distance(qn, 0.0, TWO_PI) > 1e-6).all() and (surface_distance(q0, 0.0, TWO_PI) > 1e-6).all()
    net = np.floor(qn / TWO_PI) - np.floor(q0 / TWO_PI)
    count = np.where(net * direction >= 0, np.abs(net), 0.0) if direction else np.abs(net)
    assert count.max() > ROTOR_MAX_HITS and (count == 0).any()                # an overflow and a lane with no hit are both there
    assert not got["status"].any()
    assert np.array_equal(got["n"], count.astype(np.int32)), (got["n"], count)
    qmax = max(1.0, float(np.abs(q0).max()), float(np.abs(qn).max()))
    worst = 0.0
    for row in range(ROTOR_MAX_HITS):
        w = count > row
        first = np.where(p0 > 0, np.floor(q0 / TWO_PI) + 1.0, np.floor(q0 / TWO_PI))        # the first surface value on the way
        target = TWO_PI * (first + np.sign(p0) * row)
        t = (target - q0) / p0
        bound = (8 * ROTOR_N + 2) * EPS * qmax / np.abs(p0) + EPS * ROTOR_N * ROTOR_DT
        err = np.abs(got["ht"][row] * ROTOR_DT - t)
        worst = max(worst, float((err / bound)[w].max()))
        assert (err <= bound)[w].all(), (what, row, float((err / bound)[w].max()))
        assert np.array_equal(got["hp"][row, 0][w], p0[w])                                   # the momentum, bit for bit
        assert (np.abs(got["hq"][row, 0] - target)[w] <= 8 * EPS * np.maximum(1.0, np.abs(target))[w]).all()
        for k in ("hq", "hp"):
            assert (got[k][row, 0][~w] == -7.0).all()                                        # rows at or beyond the count: untouched
        assert (got["ht"][row][~w] == -7.0).all()
    print(what, "rotor direction", direction, "worst |thit dt - t| / bound", worst, "largest count", int(count.max()))
    return worst


def osc_inputs():
    rng = np.random.default_rng(23)
    return rng.uniform(-2, 2, (1, ANCHOR_B)), rng.uniform(-2, 2, (1, ANCHOR_B))


def osc_expected(dt, nsteps, direction, max_hits):
    """The oscillator's crossings of q = 0 in closed form: per lane the list of (step, theta, Y(theta), |Y'_c(theta)|), theta by
    numpy.roots on the step's cubic; and the smallest |q| at a step end."""
    a, b = 1.0 - dt ** 2 / 2 + dt ** 4 / 24, dt - dt ** 3 / 6
    M, A, I2 = np.array([[a, b], [-b, a]]), np.array([[0.0, 1.0], [-1.0, 0.0]]), np.eye(2)
    K1 = A
    K2 = A @ (I2 + dt / 2 * K1)
    K3 = A @ (I2 + dt / 2 * K2)
    K4 = A @ (I2 + dt * K3)
    C1, C2, C3 = K1, -1.5 * K1 + (K2 + K3) - 0.5 * K4, (2.0 / 3.0) * (K1 - (K2 + K3) + K4)            # Y = y0 + dt (th C1 + th^2 C2 + th^3 C3) y0
    q0, p0 = osc_inputs()
    out, closest = [], np.inf
    for i in range(ANCHOR_B):
        y = np.array([q0[0, i], p0[0, i]])
        hits = []
        for s in range(nsteps):
            y1 = M @ y
            closest = min(closest, abs(y1[0]))
            up, down = y[0] < 0 <= y1[0], y1[0] < 0 <= y[0]
            if (up and direction >= 0) or (down and direction <= 0):
                c = [dt * (C3 @ y)[0], dt * (C2 @ y)[0], dt * (C1 @ y)[0], y[0]]
                r = np.roots(c)
                r = r[np.abs(r.imag) < 1e-12].real
                th = float(r[np.argmin(np.abs(r - y[0] / (y[0] - y1[0])))])
                assert 0.0 <= th <= 1.0
                yh = y + dt * ((th * C1 + th * th * C2 + th ** 3 * C3) @ y)
                slope = abs(dt * ((C1 + 2 * th * C2 + 3 * th * th * C3) @ y)[0])
                hits.append((s, th, yh, slope))
            y = y1
        out.append(hits)
    return out, closest


def check_oscillator(got, dt, nsteps, direction, max_hits, what):
    """-> the worst |theta - root| / (eps ymax / |Y'_c|), the ratio DESIGN.md section 13 records; the bound is 8 (k + 2) at step k."""
    exp, closest = osc_expected(dt, nsteps, direction, max_hits)
    assert closest > 1e-6                                     # no step end near the plane: the counts are unambiguous
    q0, p0 = osc_inputs()
    ymax = max(1.0, float(np.hypot(q0, p0).max()))
    assert not got["status"].any()
    worst = 0.0
    assert max(len(h) for h in exp) >= 2
    for i, hits in enumerate(exp):
        assert got["n"][i] == len(hits), (i, got["n"][i], len(hits))
        for row, (s, th, yh, slope) in enumerate(hits[:max_hits]):
            cond = EPS * ymax / slope
            err = abs((got["ht"][row, i] - s) - th)
            worst = max(worst, err / cond)
            assert err <= 8 * (s + 2) * cond + EPS * nsteps, (what, i, row, err / cond)          # (+ the rounding of step + theta)
            dy = max(abs(got["hq"][row, 0, i] - yh[0]), abs(got["hp"][row, 0, i] - yh[1]))
            assert dy <= 2 * 8 * (s + 2) * EPS * ymax * max(1.0, 2.0 * ymax * dt / slope), (what, i, row, dy)
    print(what, "oscillator dt", dt, "direction", direction, "worst |theta - root| / (eps ymax / |Y'|)", worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------- emulation
@pytest.fixture(scope="module")
def emulate(hamk_lib, tmp_path_factory):
    """System -> hamk_psec_steps_k of its companion module on the host."""
    cache = {}
    tmp = tmp_path_factory.mktemp("psec_emu")

    def make(s):
        src = s.poincare_source
        key = hashlib.sha1(src.encode()).hexdigest()[:16]
        if key not in cache:
            cpp, so = str(tmp / f"{key}.cpp"), str(tmp / f"{key}.so")
            with open(cpp, "w") as fh:
                fh.write(src + open(os.path.join(EMU, "psec_driver.inc")).read())
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-gnu-unique", "-Wno-unknown-pragmas", "-Wno-attributes",
                                   "-include", os.path.join(EMU, "hip_shim.hpp"), "-I" + os.path.join(ROOT, "hamilton_amd", "csrc"),
                                   "-o", so, cpp])
            cache[key] = ctypes.CDLL(so)
        return cache[key]
    return make


def emu_steps(L, q, p, dt, nsteps, coord, level=0.0, period=0.0, direction=1, max_hits=16, hits=None, step0=0, sentinel=0.0, thit=True,
              status=True):
    """hamk_psec_steps_k on the host, on copies -> a dict like restate's (hits: a dict q, p, t, n to continue from)."""
    q, p = (np.ascontiguousarray(a, dtype=np.float64).copy() for a in (q, p))
    n, nb = q.shape
    h = new_hits(n, nb, max_hits, sentinel) if hits is None else {k: np.array(v) for k, v in hits.items()}
    st = np.full(nb, -1, np.int32) if status else None
    L.emu_psec(P(q), P(p), LL(nb), F(dt), int(nsteps), int(coord), F(level), F(period), int(direction), int(max_hits), P(h["q"]), P(h["p"]),
               P(h["t"] if thit else None), I(h["n"]), LL(step0), I(st))
    return dict(q=q, p=p, hq=h["q"], hp=h["p"], ht=h["t"], n=h["n"], status=st)


def carry(r):
    return dict(q=r["hq"], p=r["hp"], t=r["ht"], n=r["n"])


def run_properties(run, ref, name):
    """What the scheme promises bit for bit, for any way `run(q, p, nsteps, **kw) -> dict` of running the kernel (the host emulation
    here, hamk_poincare_steps on the GPU in tests/test_gpu_poincare.py)."""
    q, p, kw, N = ref["q"], ref["p"], dict(ref["kw"]), ref["nsteps"]
    n = q.shape[0]
    one = run(q, p, N, sentinel=-7.0, **kw)
    # cut invariance: N = N1 + N2 with step0 and the buffers carried
    n1 = N // 3
    h1 = run(q, p, n1, sentinel=-7.0, **kw)
    h2 = run(h1["q"], h1["p"], N - n1, hits=carry(h1), step0=n1, **kw)
    assert same(one, h2) and np.array_equal(one["status"], h1["status"] | h2["status"])
    assert one["n"].max() > 0 and h1["n"].max() > 0 and not np.array_equal(h1["n"], one["n"])
    # rows at or beyond the count keep the sentinel; the stored ones do not
    m = stored(one)
    for k in ("hq", "hp"):
        a = one[k].transpose(0, 2, 1)
        assert (a[~m] == -7.0).all() and (a[m] != -7.0).any()
    assert (one["ht"][~m] == -7.0).all() and (one["ht"][m] >= 0.0).all() and (one["ht"][m] <= N).all()
    assert (np.diff(np.where(m, one["ht"], 2.0 * N), axis=0)[m[1:]] > 0).all()         # a lane's hits are in stepping order
    # q, p do not depend on the surface
    for other in (dict(kw, coord=(kw["coord"] + 1) % (2 * n)), dict(kw, level=kw["level"] + 0.37), dict(kw, period=0.0 if kw["period"] else 0.5),
                  dict(kw, direction=-1 if kw["direction"] >= 0 else 1), dict(kw, max_hits=1)):
        r = run(q, p, N, **other)
        assert np.array_equal(r["q"], one["q"]) and np.array_equal(r["p"], one["p"]), other
    # one row only: the count is the same, the row is the first row
    r = run(q, p, N, sentinel=-7.0, **dict(kw, max_hits=1))
    assert np.array_equal(r["n"], one["n"]) and np.array_equal(r["hq"][0], one["hq"][0]) and np.array_equal(r["ht"][0], one["ht"][0])
    # thit = NULL: everything else the same, thit untouched
    r = run(q, p, N, sentinel=-7.0, thit=False, **kw)
    assert same(one, r, ("q", "p", "hq", "hp", "n")) and (r["ht"] == -7.0).all()
    # a count that is not zero at entry: rows below it are left alone, rows from it on are filled
    hits = new_hits(n, B, kw["max_hits"], -7.0)
    hits["n"][:] = 2
    r = run(q, p, N, hits=hits, **kw)
    assert np.array_equal(r["n"], one["n"] + 2) and (r["hq"][:2] == -7.0).all() and np.array_equal(r["hq"][2:], one["hq"][:-2])
    # a count outside [0, max_hits) at entry stores nothing, whatever it is
    hits["n"][:] = np.where(np.arange(B) % 2 == 0, -1000, kw["max_hits"]).astype(np.int32)
    r = run(q, p, n1, hits=hits, **kw)
    assert (r["hq"] == -7.0).all() and (r["hp"] == -7.0).all() and (r["ht"] == -7.0).all() and np.array_equal(r["n"], hits["n"] + h1["n"])
    return one


def run_nan_lane(run, ref, lane):
    """A NaN lane among healthy ones: no hits, flagged, the neighbours keep their bits, and the launch ends."""
    q, p, kw = ref["q"], ref["p"], ref["kw"]
    nsteps = 60
    want = run(q, p, nsteps, sentinel=-7.0, **kw)
    bad = q.copy()
    bad[kw["coord"] if kw["coord"] < q.shape[0] else 0, lane] = np.nan
    got = run(bad, p, nsteps, sentinel=-7.0, **kw)
    keep = np.arange(q.shape[1]) != lane
    assert got["status"][lane] & 2 and not got["status"][keep].any() and not want["status"].any()
    assert got["n"][lane] == 0 and (got["hq"][:, :, lane] == -7.0).all() and (got["ht"][:, lane] == -7.0).all()
    assert same({k: v[..., keep] for k, v in got.items()}, {k: v[..., keep] for k, v in want.items()})


# ---------------------------------------------------------------------------------------------------------------------- 1. ABI
def test_entry_points_are_declared_exported_and_bound(hamk_lib):
    from hamilton_amd import _abi, api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hamk.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "hamilton_amd", "libhamk.so")], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in exported and name in _abi.SIGNATURES and hasattr(hamk_lib, name), name
    assert len(_abi.SIGNATURES["hamk_poincare_steps"][1]) == 18
    assert callable(api.poincareSteps) and isinstance(api.System.poincare_source, property) and isinstance(api.System.poincare_build_info, property)
    hpp = open(os.path.join(ROOT, "include", "hamilton.hpp")).read()
    hs = open(os.path.join(ROOT, "bindings", "haskell", "Numeric", "Hamilton", "HIP.hs")).read()
    assert "hamk_poincare_steps" in hpp and "poincareSteps" in hpp
    assert 'foreign import ccall safe "hamk_poincare_steps"' in hs and "poincareStepsBatch" in hs


def test_host_signature_equals_the_kernel(hamk_lib):
    """The host states the kernel's parameter list once, in namespace sig_psec of hamk_host.h (namespace sig keeps its eleven
    entries, sig_lyap its one); launch_psec builds the argument array from it.  Text only, as tests/test_kernel_signatures.py."""
    device = KS.device_kernels("hamk_psec.hpp")
    assert list(device) == ["hamk_psec_steps_k"]
    host_h = KS._text("hamk_host.h")
    body = re.search(r"namespace sig_psec \{(.*?)\}  // namespace sig_psec", host_h, re.S).group(1)
    host = {m.group(1): KS._types(m.group(2), named=False) for m in re.finditer(r"using (hamk_\w+_k) = void\(([^)]*)\);", body)}
    assert host == device
    assert device["hamk_psec_steps_k"] == ["double*", "double*", "long long", "double", "int", "int", "double", "double", "int", "int",
                                           "double*", "double*", "double*", "int*", "long long", "int*"]
    assert len(re.findall(r"using hamk_psec_steps_k\b", host_h)) == 1 and "hamk_psec_steps_k" not in KS.host_table()
    assert len(KS.host_table()) == 11
    assert "launch_kernel<sig_psec::hamk_psec_steps_k>::on(" in KS._text("hamk_dispatch.cpp")
    for cpp in ("hamk_api.cpp", "hamk_build.cpp", "hamk_dispatch.cpp", "hamk_comm.cpp", "hamk_codegen.cpp"):
        assert "hipModuleLaunchKernel" not in KS._text(cpp), cpp              # launch_kernel (hamk_host.h) stays the only caller


def test_argument_checks(hamk_lib):
    """Every refusal of include/hamk.h, each with its code and a message naming the argument, before any device is looked at;
    nothing to do is HAMK_OK and leaves every array as it was."""
    from hamilton_amd import _abi, api
    L = hamk_lib
    s = api.system_from_spec(E.get("pendulum"))
    q, p = np.array([[0.1, 0.2]]), np.array([[0.3, 0.4]])
    h = new_hits(1, 2, 3, -7.0)
    st = np.full(2, -5, np.int32)
    base = dict(s=s._h, B=2, q=q.ctypes.data, p=p.ctypes.data, dt=0.01, nsteps=5, coord=0, level=0.0, period=0.0, direction=1, max_hits=3,
                qhit=h["q"].ctypes.data, phit=h["p"].ctypes.data, thit=h["t"].ctypes.data, nhit=h["n"].ctypes.data, step0=0, status=st.ctypes.data, mem=0)

    def call(**kw):
        return L.hamk_poincare_steps(*dict(base, **kw).values())

    INV = _abi.HAMK_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    assert call(s=None) == INV and b"handle" in L.hamk_last_error()
    for k in ("q", "p", "qhit", "phit", "nhit"):
        assert call(**{k: None}) == INV and b"null" in L.hamk_last_error(), k
    assert call(B=-1) == INV
    assert call(nsteps=-1) == INV and b"nsteps" in L.hamk_last_error()
    for coord in (-1, 2, 7):
        assert call(coord=coord) == INV and b"coord" in L.hamk_last_error(), coord
    for dt in (nan, inf, -inf):
        assert call(dt=dt) == INV and b"dt" in L.hamk_last_error()
        assert call(level=dt) == INV and b"level" in L.hamk_last_error()
    for period in (nan, inf, -1.0, -1e-300):
        assert call(period=period) == INV and b"period" in L.hamk_last_error(), period
    for direction in (-2, 2, 7):
        assert call(direction=direction) == INV and b"direction" in L.hamk_last_error()
    for max_hits in (0, -4):
        assert call(max_hits=max_hits) == INV and b"max_hits" in L.hamk_last_error()
    assert call(B=1 << 40, max_hits=1 << 20) == INV and b"max_hits" in L.hamk_last_error() and b"2^48" in L.hamk_last_error()
    assert call(B=1 << 62, max_hits=0x7fffffff) == INV and b"max_hits" in L.hamk_last_error()
    assert call(step0=-1) == INV and b"step0" in L.hamk_last_error()
    assert call(mem=7) == INV
    # nothing to do: HAMK_OK with nothing launched (no GPU is needed for that) and nothing written
    before = [x.copy() for x in (q, p, h["q"], h["p"], h["t"], h["n"], st)]
    assert call(B=0) == _abi.HAMK_OK
    assert call(nsteps=0) == _abi.HAMK_OK
    assert call(nsteps=0, dt=-0.01, coord=1, period=TWO_PI, direction=0, thit=None, status=None, step0=1 << 40, mem=1) == _abi.HAMK_OK
    assert all(np.array_equal(a, b) for a, b in zip(before, (q, p, h["q"], h["p"], h["t"], h["n"], st)))
    # ... and through the binding: the state back unchanged, zeroed buffers of max_hits rows, status 0; given buffers come back
    ph, hits = api.poincareSteps(0.01, 0, s, api.Phase(q, p), 0, max_hits=4)
    assert np.array_equal(ph.positions, q) and np.array_equal(ph.momenta, p)
    assert hits.positions.shape == (4, 1, 2) and hits.momenta.shape == (4, 1, 2) and hits.times.shape == (4, 2) and hits.count.shape == (2,)
    assert hits.count.dtype == np.int32 and not hits.positions.any() and not hits.momenta.any() and not hits.times.any() and not hits.count.any()
    assert not np.asarray(s.last_status).any()
    given = api.Hits(h["q"], h["p"], h["t"], np.array([1, 5], np.int32))
    ph, hits = api.poincareSteps(0.01, 0, s, api.Phase(q, p), 0, hits=given, step0=9)
    assert np.array_equal(hits.positions, h["q"]) and np.array_equal(hits.times, h["t"]) and np.array_equal(hits.count, [1, 5])
    assert hits.positions is not h["q"]                                                     # out of place
    with pytest.raises(api.HamkError):
        api.poincareSteps(0.01, 0, s, api.Phase(q, p), 2)                                   # coord is refused through the binding too
    if L.hamk_device_count() == 0:                                                          # no CPU fall-back: a real call needs the GPU
        with pytest.raises(api.HamkError):
            api.poincareSteps(0.01, 1, s, api.Phase(q, p), 0)


def test_unsupported_handles_name_the_limit(hamk_lib):
    """One trajectory per lane: n <= 16, and no handle whose options state another mapping."""
    from hamilton_amd import _abi, api
    z = np.zeros((4, 20, 2))
    cnt = np.zeros(2, np.int32)
    big = api.system_from_spec(E.get("chain20"))
    wave = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_WAVE})
    quad = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_QUAD})
    for s, word in ((big, "n <= 16"), (wave, "HAMK_MAP_WAVE"), (quad, "HAMK_MAP_QUAD")):
        rc = hamk_lib.hamk_poincare_steps(s._h, 2, z.ctypes.data, z.ctypes.data, 0.01, 1, 0, 0.0, 0.0, 1, 4, z.ctypes.data, z.ctypes.data, None,
                                          cnt.ctypes.data, 0, None, 0)
        msg = hamk_lib.hamk_last_error().decode()
        assert rc == _abi.HAMK_ERR_UNSUPPORTED and word in msg and "n <= 16" in msg and "Poincare" in msg, (rc, msg)
        assert hamk_lib.hamk_poincare_source(s._h) is None and hamk_lib.hamk_poincare_build_info(s._h) is None
        with pytest.raises(api.HamkError, match="n <= 16") as e:
            s.poincare_source
        assert e.value.code == _abi.HAMK_ERR_UNSUPPORTED
    assert hamk_lib.hamk_poincare_source(None) is None and hamk_lib.hamk_poincare_build_info(None) is None
    lane = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_LANE})          # the lane mapping stated: fine
    assert "HAMK_INSTANTIATE_PSEC(HamkSys)" in lane.poincare_source


# ---------------------------------------------------------------------------------------------------------------------- 1. build
@pytest.mark.parametrize("name", SYSTEMS + ["chain16"])
def test_companion_module_compiles_for_gfx950(hamk_lib, name):
    """The kernel lives in a module of its own: the per-system module keeps its nine function symbols, its nine build_info rows and
    its source; the two other companions are what they were; the new one is the source with the final instantiation replaced."""
    from hamilton_amd import api
    s = api.system_from_spec(E.get(name))
    src, info, symp, lyap = s.source, s.build_info, s.symplectic_source, s.lyapunov_source
    head = src[:src.rindex("HAMK_INSTANTIATE(HamkSys)")]
    line = s.poincare_build_info
    assert line.count("\n") == 1 and line.endswith("\n")
    m = re.fullmatch(r"hamk_psec_steps_k build=default bytes=(\d+) sgpr_spills=(-?\d+) vgpr_spills=(-?\d+) vgprs=(\d+) functions=(\d+)\n", line)
    assert m, line
    nbytes, _, vspill, vgprs, nfunc = (int(x) for x in m.groups())
    assert nfunc == 1, (name, nfunc)                          # every device function inlined into the one kernel
    assert 0 < nbytes < 100 * 1024, (name, nbytes)
    assert 0 < vgprs <= 512 and vspill >= 0
    if name != "chain16":
        assert vspill == 0, (name, vspill)                    # chain8 fits; chain16 spills as both other companions do
    assert s.num_device_functions == 9 and s.build_info == info and len(info.splitlines()) == 9 and s.source == src
    assert s.symplectic_source == symp and symp == head + '#include "hamk_symp.hpp"\nHAMK_INSTANTIATE_SYMP(HamkSys)\n'
    assert s.lyapunov_source == lyap and lyap == head + '#include "hamk_lyap.hpp"\nHAMK_INSTANTIATE_LYAP(HamkSys)\n'
    fresh = api.system_from_spec(E.get(name))                                               # ... and without the new companion built
    assert fresh.symplectic_source == symp and fresh.lyapunov_source == lyap
    assert s.poincare_source == head + '#include "hamk_psec.hpp"\nHAMK_INSTANTIATE_PSEC(HamkSys)\n'
    assert s.kernel_bytes("hamk_psec_steps_k") == 0                                         # not a kernel of the per-system module
    assert s.poincare_build_info == line                                                    # built once


def test_auto_mapping_keeps_the_stepper_on_the_lane_module(hamk_lib):
    """chain12: AUTO serves small RK4 ensembles on the four-lane kernels; the section module is the lane module's companion."""
    from hamilton_amd import _abi, api
    s = api.system_from_spec(E.get("chain12"))
    assert s.options(8192)["mapping"] == _abi.MAP_QUAD
    s.describe_batch(8192)
    comp = s.poincare_source
    assert '#include "hamk_device.hpp"' in comp and "hamk_quad.hpp" not in comp and comp.endswith("HAMK_INSTANTIATE_PSEC(HamkSys)\n")


# ---------------------------------------------------------------------------------------------------------------------- 2. rotor
@pytest.mark.parametrize("direction", [1, -1, 0])
def test_rotor_anchor(emulate, oracle_lib, direction):
    """Counts from floor arithmetic, crossing times from (target - q0) / p, the momentum bit for bit, a max_hits below the fastest
    lanes' counts: the restatement first, then the kernel."""
    o = oracle_lib.OracleSystem(anchor_spec("rotor"))
    q, p = rotor_inputs()
    kw = dict(coord=0, level=0.0, period=TWO_PI, direction=direction, max_hits=ROTOR_MAX_HITS)
    r = restate(o, q, p, ROTOR_DT, ROTOR_N, hits=new_hits(1, ANCHOR_B, ROTOR_MAX_HITS, -7.0), **kw)
    check_rotor(r, direction, "restatement")
    check_rotor(emu_steps(emulate(anchor_system("rotor")), q, p, ROTOR_DT, ROTOR_N, sentinel=-7.0, **kw), direction, "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 3. oscillator
@pytest.mark.parametrize("direction", [1, -1, 0])
@pytest.mark.parametrize("case", OSC_CASES, ids=lambda c: "dt%g-n%d" % c)
def test_oscillator_anchor(emulate, oracle_lib, case, direction):
    """Count, theta and the hit state against numpy.roots on the closed-form cubic of every crossing step."""
    dt, nsteps = case
    o = oracle_lib.OracleSystem(anchor_spec("oscillator"))
    q, p = osc_inputs()
    kw = dict(coord=0, level=0.0, period=0.0, direction=direction, max_hits=8)
    check_oscillator(restate(o, q, p, dt, nsteps, **kw), dt, nsteps, direction, 8, "restatement")
    check_oscillator(emu_steps(emulate(anchor_system("oscillator")), q, p, dt, nsteps, **kw), dt, nsteps, direction, 8, "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 4. values
@pytest.mark.parametrize("name", SYSTEMS)
def test_kernel_on_host_matches_the_restatement(emulate, oracle_lib, name):
    from hamilton_amd import api
    ref = reference(oracle_lib, name)
    got = emu_steps(emulate(api.system_from_spec(E.get(name))), ref["q"], ref["p"], DT, ref["nsteps"], **ref["kw"])
    check_against_reference(ref, name, got, "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 5. bits
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_properties_on_host(emulate, oracle_lib, name):
    """Cut invariance, q and p independent of the surface, the sentinel beyond the count, thit = NULL, counts at entry."""
    from hamilton_amd import api
    ref = reference(oracle_lib, name)
    L = emulate(api.system_from_spec(E.get(name)))
    run_properties(lambda q, p, nsteps, **kw: emu_steps(L, q, p, DT, nsteps, **kw), ref, name)


def test_a_nan_lane_among_healthy_ones_on_host(emulate, oracle_lib):
    from hamilton_amd import api
    ref = reference(oracle_lib, "doublePendulum")
    L = emulate(api.system_from_spec(E.get("doublePendulum")))
    run_nan_lane(lambda q, p, nsteps, **kw: emu_steps(L, q, p, DT, nsteps, **kw), ref, 37)
    # status may be null
    a = emu_steps(L, ref["q"], ref["p"], DT, 20, **ref["kw"])
    assert same(a, emu_steps(L, ref["q"], ref["p"], DT, 20, status=False, **ref["kw"]))


# ---- the order of the first crossing time ----------------------------------------------------------------------------
# pendulum, 16 lanes, first upward crossing of q = 0 from q0 in [-2, -0.5] at rest: dt = 0.08 and 0.04 against dt / 8 = 0.01 (time
# = thit dt).  The continuous extension is third order locally, the step fourth: fourth order in time is expected.  The
# restatement's own observed order is measured first and must be fourth (3.5 .. 4.5); the kernel's must be the restatement's
# within 0.1.  Measured: restatement 3.9991, kernel on the host 3.9991, on an MI355X 3.9991.
ORDER_DTS, ORDER_T = (0.08, 0.04, 0.01), 8.0


def order_inputs(oracle_lib):
    o = oracle_lib.OracleSystem(E.get("pendulum"))
    q = np.linspace(-2.0, -0.5, 16).reshape(1, -1)
    return o, q, o.to_phase_batch(q, np.zeros_like(q))


def observed_order(run):
    """run(dt, nsteps) -> dict with ht, n: log2 of the ratio of the largest first-crossing-time errors at dt and dt / 2."""
    t = []
    for dt in ORDER_DTS:
        r = run(dt, int(round(ORDER_T / dt)))
        assert (r["n"] >= 1).all()
        t.append(r["ht"][0] * dt)
    e1, e2 = float(np.abs(t[0] - t[2]).max()), float(np.abs(t[1] - t[2]).max())
    return float(np.log2(e1 / e2)), e1, e2


def check_order(oracle_lib, run, what):
    o, q, p = order_inputs(oracle_lib)
    kw = dict(coord=0, level=0.0, period=0.0, direction=1, max_hits=2)
    own = observed_order(lambda dt, nsteps: restate(o, q, p, dt, nsteps, **kw))
    got = observed_order(lambda dt, nsteps: run(q, p, dt, nsteps, **kw))
    print(what, "observed order of the first crossing time: restatement", own, "kernel", got)
    assert 3.5 < own[0] < 4.5, own
    assert abs(got[0] - own[0]) < 0.1, (got, own)


def test_order_of_the_first_crossing_time_on_host(emulate, oracle_lib):
    from hamilton_amd import api
    L = emulate(api.system_from_spec(E.get("pendulum")))
    check_order(oracle_lib, lambda q, p, dt, nsteps, **kw: emu_steps(L, q, p, dt, nsteps, **kw), "kernel on host")
