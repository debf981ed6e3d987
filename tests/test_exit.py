"""CPU: first-exit times fused with RK4 (hamk_exit_steps; hamilton_amd/csrc/hamk_exit.hpp) -- its three entry points and their
argument checks, the host's statement of the kernel's signature, the companion module that carries the kernel (compiled for gfx950
here: hiprtc needs no GPU), and the kernel itself run thread by thread on the host (tests/host_emulation/exit_driver.inc, the g++
flags of test_lyapunov.py's `emulate`; __ballot is the thread's own predicate there) against a literal numpy restatement of the
scheme over the oracle's hamEqs (below), against three analytic anchors, and for the bit-level properties the scheme promises.
What this cannot see is the GPU compiler and the wave-wide break (tests/test_gpu_exit.py, which imports the restatement, the
anchors, the inputs and the bounds from here)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import test_kernel_signatures as KS
import test_poincare as PS
from conftest import ROOT
from hamilton_amd import examples as E
from test_lyapunov import sample_phase

EMU = os.path.join(ROOT, "tests", "host_emulation")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
P = lambda a: None if a is None else a.ctypes.data_as(_dp)
I = lambda a: None if a is None else a.ctypes.data_as(_ip)
LL = ctypes.c_longlong
F = ctypes.c_double
NAMES = ("hamk_exit_steps", "hamk_exit_source", "hamk_exit_build_info")
EPS = 2.2e-16
PI = float(np.pi)
INF = float("inf")
NEWTON = 4
ALIVE, NONFINITE = -1, -2
ST_NONFINITE = 2


# ---------------------------------------------------------------------------------------------------------------------- reference
# A LITERAL numpy restatement of the scheme of hamilton_amd/csrc/hamk_exit.hpp over the oracle's hamEqs (the oracle itself is not
# changed).  A lane is alive iff its code is -1.  Per alive lane and step: y1 = RK4(y0); any component of y1 not finite: code -2,
# texit = step0 + step + 1; otherwise gate g = (coord, lo, hi) fires where y1[coord] < lo or > hi, the target is the violated
# bound, theta from the secant value by four Newton iterations on the cubic Y(theta) = y0 + dt [b1 k1 + b2 (k2 + k3) + b4 k4],
# clamped to [0, 1] after each, a non-finite update ignored, theta = 0 where y0[coord] is outside already; the smallest theta wins,
# on a tie the lowest index: code = 2 g + side, texit = (step0 + step) + theta, the exit state Y(theta); y = y1 either way, and a
# stopped lane is never touched again.
def new_exits(n, nb, sentinel=0.0):
    return dict(code=np.full(nb, ALIVE, np.int32), t=np.full(nb, sentinel), q=np.full((n, nb), sentinel), p=np.full((n, nb), sentinel))


def restate(o, q, p, dt, nsteps, gates, exits=None, step0=0, perturb=None):
    """-> dict(q, p [n, B]; code [B] int32; t [B]; eq, ep [n, B]; status [B]; margin [B]: the smallest distance of a step end of
    an alive lane from a finite bound relative to max(1, |yc|); target [B]: the bound of every exit; steps [B]: the steps each lane
    ran).  perturb: a numpy Generator -- every hamEqs output is multiplied by 1 +- 1e-12, the signs drawn from it."""
    q, p = np.array(q, dtype=np.float64), np.array(p, dtype=np.float64)
    n, nb = q.shape
    e = new_exits(n, nb) if exits is None else {k: np.array(v) for k, v in exits.items()}
    code, te, eq, ep = e["code"].astype(np.int64), e["t"], e["q"], e["p"]
    st = np.zeros(nb, np.int32)
    margin = np.full(nb, np.inf)
    target = np.full(nb, np.nan)
    steps = np.zeros(nb, np.int64)
    yall = np.concatenate([q, p])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for s in range(nsteps):
            w = np.nonzero(code == ALIVE)[0]
            if not w.size:
                break
            steps[w] += 1
            y = np.ascontiguousarray(yall[:, w])
            sw = np.zeros(w.size, np.int32)

            def f(v):
                dq, dp, s1 = o.hameqs_batch(np.ascontiguousarray(v[:n]), np.ascontiguousarray(v[n:]), threads=1)
                sw[:] |= s1
                if perturb is not None:
                    dq = dq * (1.0 + 1e-12 * perturb.choice([-1.0, 1.0], size=dq.shape))
                    dp = dp * (1.0 + 1e-12 * perturb.choice([-1.0, 1.0], size=dp.shape))
                return np.concatenate([dq, dp])

            k1 = f(y)
            k2 = f(y + 0.5 * dt * k1)
            k3 = f(y + 0.5 * dt * k2)
            k4 = f(y + dt * k3)
            y1 = y + dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
            k23 = k2 + k3
            st[w] |= sw
            bad = ~np.isfinite(y1).all(0)
            best, won, tgt = np.full(w.size, 2.0), np.full(w.size, -1), np.full(w.size, np.nan)
            for g, (c, lo, hi) in enumerate(gates):
                y0c, y1c = y[c], y1[c]
                below, above = y1c < lo, y1c > hi
                t = np.where(below, lo, hi)
                th = np.clip((t - y0c) / (y1c - y0c), 0.0, 1.0)
                for _ in range(NEWTON):
                    b1, b2, b4 = PS.cubic_weights(th)
                    gv = (y0c - t) + dt * (b1 * k1[c] + b2 * k23[c] + b4 * k4[c])
                    dg = dt * ((1.0 - 3.0 * th + 2.0 * th * th) * k1[c] + (2.0 * th - 2.0 * th * th) * k23[c] + (2.0 * th * th - th) * k4[c])
                    tn = th - gv / dg
                    th = np.where(np.isfinite(tn), np.clip(tn, 0.0, 1.0), th)
                th = np.where((y0c < lo) | (y0c > hi), 0.0, th)
                wins = (below | above) & ~bad & (th < best)
                best, won, tgt = np.where(wins, th, best), np.where(wins, 2 * g + above, won), np.where(wins, t, tgt)
                d = np.fmin(np.abs(y1c - lo), np.abs(y1c - hi)) / np.maximum(1.0, np.abs(y1c))
                margin[w] = np.fmin(margin[w], np.where(bad, np.inf, d))
            out = won >= 0
            b1, b2, b4 = PS.cubic_weights(best)
            yh = y + dt * (b1 * k1 + b2 * k23 + b4 * k4)
            code[w[out]] = won[out]
            te[w[out]] = float(step0 + s) + best[out]
            eq[:, w[out]] = yh[:n, out]
            ep[:, w[out]] = yh[n:, out]
            target[w[out]] = tgt[out]
            code[w[bad]] = NONFINITE
            te[w[bad]] = float(step0 + s + 1)
            st[w[bad]] |= ST_NONFINITE
            yall[:, w] = y1
    return dict(q=yall[:n].copy(), p=yall[n:].copy(), code=code.astype(np.int32), t=te, eq=eq, ep=ep, status=st, margin=margin, target=target,
                steps=steps)


OUT = ("q", "p", "code", "t", "eq", "ep")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b, keys=OUT):
    """Bit for bit, NaN payloads included."""
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def lanes(r, w, keys=OUT + ("status",)):
    return {k: r[k][..., w] for k in keys if r.get(k) is not None}


def carry(r):
    return dict(code=r["code"], t=r["t"], q=r["eq"], p=r["ep"])


# The comparison of the kernel with the restatement: four systems, B = 257 (four wavefronts and one lane), dt = 0.02.
#   pendulum:        one gate on q, [-pi, pi]: the lanes that swing over
#   doublePendulum:  theta1, theta2 in [-pi, pi]: the flip map
#   chain8:          q[3] in [-c, c], from test_poincare's smooth small-amplitude sample (DESIGN.md sections 12 / 13 say why)
#   opcodeZoo:       two gates on q[0] and p[0]; 20 steps, its lanes leave the domain of its sqrt / log soon after (section 13)
# The gates are placed on the oracle's trajectories so that a good part of the lanes exits, a good part survives and no lane starts
# outside a gate (asserted in reference(); a start outside is the free particle's case: its exit state is y0, not a point of the bound).
SYSTEMS = ["pendulum", "doublePendulum", "chain8", "opcodeZoo"]
B = 257
DT = 0.02
MARGIN = 1e-9
CASES = {                    # name -> (nsteps, gates, seed of the sample)
    "pendulum": (400, [(0, -PI, PI)], 17),
    "doublePendulum": (400, [(0, -PI, PI), (1, -PI, PI)], 17),
    "chain8": (300, [(3, -0.16, 0.16)], 17),
    "opcodeZoo": (20, [(0, -0.85, 0.85), (2, -2.0, INF)], 17),
}
_reference = {}


def inputs(name, spec, o, seed):
    return PS.inputs(name, spec, o, seed) if name == "chain8" else sample_phase(spec, o, seed, B)


def exited(r):
    return r["code"] >= 0


def reference(oracle_lib, name):
    """Inputs, the restatement's result and the bounds for a system, computed once and shared by every test of both modules.
    texit, the exit state and the final state: the restatement a second time with every hamEqs output multiplied by 1 +- 1e-12
    (fixed-seed signs; 1e-12 is the tolerance ladder's own hamEqs figure) -- the bound is 4 x the largest
    |difference| between the two runs, DESIGN.md section 12's method and margin.  A lane may be left out only where some step end
    of the restatement lies within 1e-9 max(1, |yc|) of a bound: the seeds are chosen so that there is none, asserted here."""
    if name not in _reference:
        nsteps, gates, seed = CASES[name]
        spec = E.get(name)
        o = oracle_lib.OracleSystem(spec)
        q, p = inputs(name, spec, o, seed)
        y0 = np.concatenate([q, p])
        assert all(((y0[c] >= lo) & (y0[c] <= hi)).all() for c, lo, hi in gates), name
        want = restate(o, q, p, DT, nsteps, gates)
        other = restate(o, q, p, DT, nsteps, gates, perturb=np.random.default_rng(7))
        assert np.isfinite(want["q"]).all() and np.isfinite(want["p"]).all() and not want["status"].any(), name
        left_out = want["margin"] < MARGIN
        m = exited(want)
        print(name, "lanes left out", int(left_out.sum()), "smallest margin", float(want["margin"].min()), "exited", int(m.sum()), "of", B,
              "codes", np.unique(want["code"]).tolist(), "median exit step", float(np.median(want["t"][m])) if m.any() else None)
        assert left_out.sum() == 0, (name, np.nonzero(left_out)[0])                 # at most 2 of 257 may be; the seed leaves none
        assert 20 <= m.sum() <= B - 20, (name, int(m.sum()))                        # exits and survivors are both there
        assert np.array_equal(want["code"], other["code"]) and np.array_equal(np.floor(want["t"]), np.floor(other["t"]))
        diff = lambda k, mask: float(np.abs(want[k] - other[k])[..., mask].max())
        _reference[name] = dict(o=o, q=q, p=p, want=want, nsteps=nsteps, gates=gates, left_out=left_out,
                                t_bound=4.0 * diff("t", m), e_bound=4.0 * max(diff("eq", m), diff("ep", m)),
                                y_bound=4.0 * max(diff("q", slice(None)), diff("p", slice(None))))
    return _reference[name]


def surface_residual(ref, r):
    """The largest |exit_state[coord] - bound| / max(1, |bound|) over the exited lanes of a result on ref's inputs (codes and
    bounds are the restatement's: the codes agree wherever this is called)."""
    want = ref["want"]
    n = ref["q"].shape[0]
    worst = 0.0
    for i in np.nonzero(exited(want))[0]:
        c = ref["gates"][want["code"][i] // 2][0]
        yc = r["eq"][c, i] if c < n else r["ep"][c - n, i]
        worst = max(worst, abs(yc - want["target"][i]) / max(1.0, abs(want["target"][i])))
    return worst


SURFACE_MARGIN = 8.0


def check_against_reference(ref, name, got, what):
    """got: a kernel run on ref's inputs (a dict like restate's): every lane that is not left out, every output."""
    want, keep = ref["want"], ~ref["left_out"]
    assert keep.sum() >= B - 2
    m = exited(want) & keep
    dt_ = float(np.abs(got["t"] - want["t"])[m].max())
    de = float(max(np.abs(got["eq"] - want["eq"])[:, m].max(), np.abs(got["ep"] - want["ep"])[:, m].max()))
    dy = float(max(np.abs(got["q"] - want["q"])[:, keep].max(), np.abs(got["p"] - want["p"])[:, keep].max()))
    surf, rsurf = surface_residual(ref, got), surface_residual(ref, want)
    print(what, name, "|dtexit|", dt_, "bound", ref["t_bound"], "|dexit state|", de, "bound", ref["e_bound"], "|dstate|", dy, "bound", ref["y_bound"],
          "on the bound", surf, "restatement's", rsurf)
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["code"][keep], want["code"][keep]), np.nonzero(got["code"] != want["code"])[0]
    assert dt_ <= ref["t_bound"], (name, dt_, ref["t_bound"])
    assert de <= ref["e_bound"], (name, de, ref["e_bound"])
    assert dy <= ref["y_bound"], (name, dy, ref["y_bound"])
    assert surf <= SURFACE_MARGIN * max(rsurf, EPS), (name, surf, rsurf)
    alive = want["code"] == ALIVE                                   # what a running lane never had written
    assert (got["t"][alive] == 0.0).all() and (got["eq"][:, alive] == 0.0).all() and (got["ep"][:, alive] == 0.0).all()


# ---- analytic anchors ------------------------------------------------------------------------------------------------
# rotor:         test_poincare's (K = 1, hamEqs = (p, 0); RK4 and the cubic are exact to rounding).  Gate q in [-pi, pi], p of both
#                signs and p = 0: a lane leaves through the upper bound for p > 0 (code 1) at time (pi - q0) / p, through the lower
#                for p < 0 (code 0) at (-pi - q0) / p, never for p = 0 (code -1).  Bound on |texit dt - t|: DESIGN.md section 13's
#                for its rotor with k = the exit step: (8 k + 2) eps qmax / |p| + eps k dt, here with k <= ROTOR_N.
# oscillator:    test_poincare's closed-form RK4 map and cubic; gate q in [-c, c]: the first exit's theta against numpy.roots on the
#                exit step's cubic, within section 13's conditioning bound 8 (k + 2) eps ymax / |Y'_c(theta)| at step k.
# free particle: mkSystem([1, 1], (q0, q1), U = 0), n = 2: hamEqs = (p, 0), everything exact to rounding; the three gate-order
#                cases of the scheme (test_free_particle_*).
ANCHOR_B = 64
ROTOR_DT, ROTOR_N = 0.02, 400
ROTOR_GATES = [(0, -PI, PI)]
OSC_CASES = [(0.1, 100), (0.5, 40)]            # (dt, nsteps)
OSC_C = 0.75

anchor_spec = PS.anchor_spec
_anchor_systems = {}


def free_spec():
    return E.SystemSpec(name="free2", m=2, n=2, inertia=(1.0, 1.0), f=lambda q, ops: [q[0], q[1]], u=lambda z, ops: 0.0 * z[0], u_space=0,
                        q0=(0.0, 0.0), qd0=(1.0, 1.0))


def anchor_system(kind):
    """The library's handle, by mkSystem (one per kind and process)."""
    from hamilton_amd import api
    if kind == "free":
        if kind not in _anchor_systems:
            _anchor_systems[kind] = api.mkSystem([1.0, 1.0], lambda q: [q[0], q[1]], lambda q: 0.0 * q[0], 2)
        return _anchor_systems[kind]
    return PS.anchor_system(kind)


def rotor_inputs(nb=ANCHOR_B):
    """p of both signs, magnitudes 1 .. 4, every eighth lane at rest; q0 in (-3, 3)."""
    lane = np.arange(nb)
    p = np.where(lane % 2 == 0, 1.0, -1.0) * (1.0 + 3.0 * (lane % 61) / 60.0)
    p[lane % 8 == 3] = 0.0
    q = 2.9 * np.sin(1.0 + 0.7 * lane)
    return q.reshape(1, -1).copy(), p.reshape(1, -1).copy()


def check_rotor(got, what, nb=ANCHOR_B):
    """got: ROTOR_N steps of ROTOR_DT from rotor_inputs(nb), ROTOR_GATES, sentinel -7.  -> worst error / bound."""
    q0, p0 = rotor_inputs(nb)
    q0, p0 = q0[0], p0[0]
    moving = p0 != 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p0 > 0, (PI - q0) / p0, (-PI - q0) / p0)
    assert (t[moving] < 0.9 * ROTOR_N * ROTOR_DT).all() and (~moving).any()            # every moving lane leaves well inside the run
    assert not got["status"].any()
    assert np.array_equal(got["code"], np.where(p0 > 0, 1, np.where(p0 < 0, 0, ALIVE)).astype(np.int32))
    k = np.floor(t / ROTOR_DT)
    bound = (8 * (k + 1) + 2) * EPS * PI / np.abs(np.where(moving, p0, 1.0)) + EPS * (k + 1) * ROTOR_DT
    err = np.abs(got["t"] * ROTOR_DT - t)
    assert (err[moving] <= bound[moving]).all(), (what, float((err[moving] / bound[moving]).max()))
    assert np.array_equal(got["ep"][0][moving], p0[moving]) and np.array_equal(got["p"][0], p0)      # the momentum, bit for bit
    tgt = np.where(p0 > 0, PI, -PI)
    assert (np.abs(got["eq"][0] - tgt)[moving] <= 8 * EPS * PI).all()
    # a stopped lane holds the end of its exit step; a lane at rest has not moved and nothing of its exit record was written
    k = np.where(moving, k, 0.0)
    assert (np.abs(got["q"][0] - (q0 + (k + 1) * ROTOR_DT * p0))[moving] <= (8 * (k[moving] + 1) + 2) * EPS * 2 * PI).all()
    assert np.array_equal(got["q"][0][~moving], q0[~moving])
    assert (got["t"][~moving] == -7.0).all() and (got["eq"][0][~moving] == -7.0).all() and (got["ep"][0][~moving] == -7.0).all()
    worst = float((err[moving] / bound[moving]).max())
    print(what, "rotor worst |texit dt - t| / bound", worst, "latest exit step", int(k[moving].max()))
    return worst


osc_inputs = PS.osc_inputs


def osc_expected(dt, nsteps):
    """The oscillator's first exit from |q| <= OSC_C in closed form: per lane None or (step, side, theta, Y(theta), |Y'_c(theta)|),
    theta by numpy.roots on the exit step's cubic; and the smallest distance of a step end from a bound."""
    a, b = 1.0 - dt ** 2 / 2 + dt ** 4 / 24, dt - dt ** 3 / 6
    M, A, I2 = np.array([[a, b], [-b, a]]), np.array([[0.0, 1.0], [-1.0, 0.0]]), np.eye(2)
    K1 = A
    K2 = A @ (I2 + dt / 2 * K1)
    K3 = A @ (I2 + dt / 2 * K2)
    K4 = A @ (I2 + dt * K3)
    C1, C2, C3 = K1, -1.5 * K1 + (K2 + K3) - 0.5 * K4, (2.0 / 3.0) * (K1 - (K2 + K3) + K4)
    q0, p0 = osc_inputs()
    out, closest = [], np.inf
    for i in range(ANCHOR_B):
        y = np.array([q0[0, i], p0[0, i]])
        hit = None
        for s in range(nsteps):
            y1 = M @ y
            closest = min(closest, abs(abs(y1[0]) - OSC_C))
            if abs(y1[0]) > OSC_C:
                side = int(y1[0] > 0)
                tgt = OSC_C if side else -OSC_C
                if abs(y[0]) > OSC_C:                                  # outside at the start (step 0 only): theta = 0
                    hit = (s, side, 0.0, y.copy(), abs(dt * (C1 @ y)[0]))
                else:
                    r = np.roots([dt * (C3 @ y)[0], dt * (C2 @ y)[0], dt * (C1 @ y)[0], y[0] - tgt])
                    r = r[np.abs(r.imag) < 1e-12].real
                    th = float(r[np.argmin(np.abs(r - (tgt - y[0]) / (y1[0] - y[0])))])
                    assert 0.0 <= th <= 1.0
                    hit = (s, side, th, y + dt * ((th * C1 + th * th * C2 + th ** 3 * C3) @ y), abs(dt * ((C1 + 2 * th * C2 + 3 * th * th * C3) @ y)[0]))
                break
            y = y1
        out.append(hit)
    return out, closest


def check_oscillator(got, dt, nsteps, what):
    """-> the worst |theta - root| / (eps ymax / |Y'_c|); the bound is 8 (k + 2) at step k."""
    exp, closest = osc_expected(dt, nsteps)
    assert closest > 1e-6                                     # no step end near a bound: the codes are unambiguous
    q0, p0 = osc_inputs()
    ymax = max(1.0, float(np.hypot(q0, p0).max()))
    assert not got["status"].any()
    worst = 0.0
    assert sum(h is None for h in exp) >= 2 and sum(h is not None and h[2] > 0 for h in exp) >= 8 and any(h is not None and h[2] == 0 for h in exp)
    for i, h in enumerate(exp):
        if h is None:
            assert got["code"][i] == ALIVE, i
            continue
        s, side, th, yh, slope = h
        assert got["code"][i] == side, (i, got["code"][i], side)
        cond = EPS * ymax / slope
        err = abs((got["t"][i] - s) - th)
        worst = max(worst, err / cond)
        assert err <= 8 * (s + 2) * cond + EPS * nsteps, (what, i, err / cond)
        dy = max(abs(got["eq"][0, i] - yh[0]), abs(got["ep"][0, i] - yh[1]))
        assert dy <= 2 * 8 * (s + 2) * EPS * ymax * max(1.0, 2.0 * ymax * dt / slope), (what, i, dy)
    print(what, "oscillator dt", dt, "worst |theta - root| / (eps ymax / |Y'|)", worst)
    return worst


# free particle, n = 2, dt = 0.5, one step decides: y0 = (q0, q1, p0, p1), y1 = (q0 + dt p0, q1 + dt p1, p0, p1), all exact in binary.
FREE_DT = 0.5
FREE_GATES = [(0, -1.0, 1.0), (1, -1.0, 1.0)]
FREE_LANES = [      # (q0, q1, p0, p1) -> (code, texit, exit q0, exit q1) after 4 steps with step0 = 10
    ((0.5, 0.75, 2.0, 2.0), (3, 10.25, 0.75, 1.0)),          # both gates violated in step 0: theta 0.5 against 0.25 -- the second gate wins
    ((0.75, 0.5, 2.0, 2.0), (1, 10.25, 1.0, 0.75)),          # ... and the other way round
    ((0.5, 0.5, 2.0, 2.0), (1, 10.5, 1.0, 1.0)),             # an exact tie: the lower index wins
    ((-0.5, -0.5, -2.0, -2.0), (0, 10.5, -1.0, -1.0)),       # ... through the lower bounds
    ((1.5, 0.0, 1.0, 0.0), (1, 10.0, 1.5, 0.0)),             # starts outside a gate: theta = 0, texit = step0, the exit state is y0
    ((-1.5, 0.0, 0.5, 0.0), (0, 10.0, -1.5, 0.0)),           # ... outside below, moving back in but not there after the step
    ((0.0, 0.0, 0.25, -0.625), (2, 13.2, 0.4, -1.0)),        # leaves through q1 = -1 in the last step, at t = 1.6 = (3 + 0.2) dt
    ((0.0, 0.0, 0.25, 0.125), (ALIVE, -7.0, -7.0, -7.0)),    # never leaves in 4 steps
]


def check_free(got, what):
    for i, (y0, (code, t, e0, e1)) in enumerate(FREE_LANES):
        assert got["code"][i] == code, (what, i, got["code"][i], code)
        if code == ALIVE:
            assert got["t"][i] == -7.0 and (got["eq"][:, i] == -7.0).all() and (got["ep"][:, i] == -7.0).all(), (what, i)
            continue
        # every quantity is below 2 (texit: below 16) and comes out of a handful of roundings: 8 eps of its magnitude
        assert abs(got["t"][i] - t) <= 8 * EPS * 16 and abs(got["eq"][0, i] - e0) <= 8 * EPS * 2 and abs(got["eq"][1, i] - e1) <= 8 * EPS * 2, (what, i, got["t"][i], got["eq"][:, i])
        assert got["ep"][0, i] == y0[2] and got["ep"][1, i] == y0[3]
        if t == 10.0:
            assert got["t"][i] == 10.0 and got["eq"][0, i] == e0 and got["eq"][1, i] == e1            # theta = 0: texit = step0 and Y(0) = y0, exactly
    assert not got["status"].any()


def free_inputs():
    y = np.array([l[0] for l in FREE_LANES]).T
    return np.ascontiguousarray(y[:2]), np.ascontiguousarray(y[2:])


# ---------------------------------------------------------------------------------------------------------------------- emulation
@pytest.fixture(scope="module")
def emulate(hamk_lib, tmp_path_factory):
    """System -> hamk_exit_steps_k of its companion module on the host."""
    cache = {}
    tmp = tmp_path_factory.mktemp("exit_emu")

    def make(s):
        src = s.exit_source
        key = hashlib.sha1(src.encode()).hexdigest()[:16]
        if key not in cache:
            d = tmp / key
            d.mkdir()
            cpp, so = str(d / "exit.cpp"), str(d / "exit.so")
            with open(str(d / "exit_module.inc"), "w") as fh:
                fh.write(src)
            with open(cpp, "w") as fh:
                fh.write(open(os.path.join(EMU, "exit_driver.inc")).read())
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-gnu-unique", "-Wno-unknown-pragmas", "-Wno-attributes",
                                   "-include", os.path.join(EMU, "hip_shim.hpp"), "-I" + os.path.join(ROOT, "hamilton_amd", "csrc"),
                                   "-o", so, cpp])
            cache[key] = ctypes.CDLL(so)
        return cache[key]
    return make


def gate_arrays(gates):
    return (np.array([g[0] for g in gates], np.int32), np.array([g[1] for g in gates], np.float64), np.array([g[2] for g in gates], np.float64))


def emu_steps(L, q, p, dt, nsteps, gates, exits=None, step0=0, sentinel=0.0, record=True, status=True):
    """hamk_exit_steps_k on the host, on copies -> a dict like restate's (exits: a dict code, t, q, p to continue from;
    record=False: qexit = pexit = NULL)."""
    q, p = (np.ascontiguousarray(a, dtype=np.float64).copy() for a in (q, p))
    n, nb = q.shape
    e = new_exits(n, nb, sentinel) if exits is None else {k: np.array(v) for k, v in exits.items()}
    st = np.full(nb, -1, np.int32) if status else None
    c, lo, hi = gate_arrays(gates)
    L.emu_exit(P(q), P(p), LL(nb), F(dt), int(nsteps), I(c), P(lo), P(hi), len(gates), I(e["code"]), P(e["t"]), P(e["q"] if record else None),
               P(e["p"] if record else None), LL(step0), I(st))
    return dict(q=q, p=p, code=e["code"], t=e["t"], eq=e["q"], ep=e["p"], status=st)


def run_properties(run, ref, name):
    """What the scheme promises bit for bit, for any way `run(q, p, nsteps, gates, **kw) -> dict` of running the kernel (the host
    emulation here, hamk_exit_steps on the GPU in tests/test_gpu_exit.py)."""
    q, p, gates, N = ref["q"], ref["p"], ref["gates"], ref["nsteps"]
    n, nb = q.shape
    one = run(q, p, N, gates, sentinel=-7.0)
    out = exited(one)
    assert 20 <= out.sum() <= nb - 20
    # cut invariance: N = N1 + N2 with step0 and the arrays carried, bit for bit on every output
    n1 = N // 3
    h1 = run(q, p, n1, gates, sentinel=-7.0)
    h2 = run(h1["q"], h1["p"], N - n1, gates, exits=carry(h1), step0=n1)
    assert same(one, h2) and np.array_equal(one["status"], h1["status"] | h2["status"])
    assert exited(h1).any() and (exited(h1) != out).any()                    # lanes stop in both parts
    # a running lane's exit record is never written
    assert (one["t"][~out] == -7.0).all() and (one["eq"][:, ~out] == -7.0).all() and (one["ep"][:, ~out] == -7.0).all()
    assert (one["t"][out] >= 0.0).all() and (one["t"][out] <= N).all()
    # freeze: a stopped lane's q, p are those of a call that ends with its exit step
    for k in np.unique(np.floor(one["t"][out]).astype(int))[[0, -1]]:
        w = out & (np.floor(one["t"]) == k)
        r = run(q, p, int(k) + 1, gates)
        assert same(lanes(r, w), lanes(one, w), ("q", "p", "code", "t", "eq", "ep"))
    # gate independence: lanes that survive both gate lists hold the same bits
    for other in ([(g[0], 1.5 * g[1], 1.5 * g[2]) for g in gates], [(gates[0][0], -INF, INF)], gates + [((gates[0][0] + 1) % (2 * n), -INF, 1e300)]):
        r = run(q, p, N, other)
        w = ~out & ~exited(r)
        assert w.sum() >= 20 and same(lanes(r, w), lanes(one, w), ("q", "p")), other
    # infinite bounds on both sides: nobody stops, and the state is the plain RK4 state of the survivors above
    r = run(q, p, N, [(gates[0][0], -INF, INF)], sentinel=-7.0)
    assert (r["code"] == ALIVE).all() and (r["t"] == -7.0).all() and same(lanes(r, ~out), lanes(one, ~out), ("q", "p"))
    # one bound infinite: the lanes that left through the finite bound of gate 0 FIRST still do, at the same time
    c0, lo0, hi0 = gates[0]
    r = run(q, p, N, [(c0, -INF, hi0)] + gates[1:], sentinel=-7.0)
    w = one["code"] == 1
    assert w.any() and same(lanes(r, w), lanes(one, w))
    assert not (r["code"] == 0).any()
    # qexit = pexit = NULL: everything else the same, the exit states untouched
    r = run(q, p, N, gates, sentinel=-7.0, record=False)
    assert same(one, r, ("q", "p", "code", "t")) and (r["eq"] == -7.0).all() and (r["ep"] == -7.0).all()
    # lanes stopped at entry keep their bits, NaN payloads and arbitrary codes included; status 0
    nan1 = np.array([0x7ff8dead0000beef], np.uint64).view(np.float64)[0]
    e = new_exits(n, nb, -7.0)
    stopped = np.arange(nb) % 3 == 1
    e["code"][stopped] = np.resize(np.array([0, 1, 7, -2, -3, 1 << 30, -(1 << 31)], np.int64), int(stopped.sum())).astype(np.int32)
    e["t"][stopped] = nan1
    e["q"][:, stopped] = nan1
    qs, ps = q.copy(), p.copy()
    qs[:, stopped & (np.arange(nb) % 2 == 0)] = nan1
    ps[:, stopped & (np.arange(nb) % 2 == 1)] = 1e308
    r = run(qs, ps, N, gates, exits=e)
    given = dict(q=qs, p=ps, code=e["code"], t=e["t"], eq=e["q"], ep=e["p"])
    assert same(lanes(r, stopped, OUT), lanes(given, stopped, OUT)) and not r["status"][stopped].any()
    assert same(lanes(r, ~stopped, OUT), lanes(one, ~stopped, OUT)) and np.array_equal(r["status"][~stopped], one["status"][~stopped])
    return one


def run_nan_lane(run, ref, lane):
    """A NaN lane among healthy ones: code -2 after its first step, flagged, its exit state untouched; the neighbours keep their
    bits, and the launch ends."""
    q, p, gates = ref["q"], ref["p"], ref["gates"]
    nsteps = 60
    want = run(q, p, nsteps, gates, sentinel=-7.0, step0=5)
    bad = q.copy()
    bad[0, lane] = np.nan
    got = run(bad, p, nsteps, gates, sentinel=-7.0, step0=5)
    keep = np.arange(q.shape[1]) != lane
    assert got["status"][lane] & ST_NONFINITE and not (got["status"][keep] & ST_NONFINITE).any()
    assert got["code"][lane] == NONFINITE and got["t"][lane] == 6.0
    assert (got["eq"][:, lane] == -7.0).all() and (got["ep"][:, lane] == -7.0).all()
    assert same(lanes(got, keep), lanes(want, keep))
    one = run(bad, p, 1, gates, sentinel=-7.0, step0=5)                    # freeze: floor(texit) - step0 steps for code -2
    assert same(lanes(one, ~keep), lanes(got, ~keep))


# ---------------------------------------------------------------------------------------------------------------------- 1. ABI
def test_entry_points_are_declared_exported_and_bound(hamk_lib):
    from hamilton_amd import _abi, api
    raw = open(os.path.join(ROOT, "include", "hamk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "hamilton_amd", "libhamk.so")], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in exported and name in _abi.SIGNATURES and hasattr(hamk_lib, name), name
    assert len(_abi.SIGNATURES["hamk_exit_steps"][1]) == 15
    for macro, value in (("HAMK_EXIT_MAX_GATES", "4"), ("HAMK_EXIT_ALIVE", "-1"), ("HAMK_EXIT_NONFINITE", "-2")):
        assert re.search(r"#define\s+" + macro + r"\s+" + value + r"\s", header), macro
    assert re.search(r"typedef struct hamk_gate \{\s*int32_t coord;\s*int32_t reserved;\s*double lo, hi;\s*\} hamk_gate;", header)
    assert ctypes.sizeof(_abi.hamk_gate) == 24
    assert "hamk_exit_steps" in raw[:raw.index("#define HAMK_H")]                         # the header comment's table of entry points
    assert callable(api.exitSteps) and isinstance(api.System.exit_source, property) and isinstance(api.System.exit_build_info, property)
    hpp = open(os.path.join(ROOT, "include", "hamilton.hpp")).read()
    hs = open(os.path.join(ROOT, "bindings", "haskell", "Numeric", "Hamilton", "HIP.hs")).read()
    assert "hamk_exit_steps" in hpp and "exitSteps" in hpp
    assert 'foreign import ccall safe "hamk_exit_steps"' in hs and "exitStepsBatch" in hs


def test_host_signature_equals_the_kernel(hamk_lib):
    """The host states the kernel's parameter list once, in namespace sig_exit of hamk_host.h (namespace sig keeps its eleven
    entries); launch_exit builds the argument array from it.  Text only, as tests/test_kernel_signatures.py."""
    device = KS.device_kernels("hamk_exit.hpp")
    assert list(device) == ["hamk_exit_steps_k"]
    host_h = KS._text("hamk_host.h")
    body = re.search(r"namespace sig_exit \{(.*?)\}  // namespace sig_exit", host_h, re.S).group(1)
    host = {m.group(1): KS._types(m.group(2), named=False) for m in re.finditer(r"using (hamk_\w+_k) = void\(([^)]*)\);", body)}
    assert host == device
    assert device["hamk_exit_steps_k"] == ["double*", "double*", "long long", "double", "int", "HamkGates", "int*", "double*", "double*", "double*",
                                           "long long", "int*"]
    assert len(re.findall(r"using hamk_exit_steps_k\b", host_h)) == 1 and "hamk_exit_steps_k" not in KS.host_table()
    assert len(KS.host_table()) == 11
    assert "launch_kernel<sig_exit::hamk_exit_steps_k>::on(" in KS._text("hamk_dispatch.cpp")
    # the gates travel by value: one struct, the same text on both sides
    decl = r"struct HamkGates \{ double lo\[4\], hi\[4\]; int coord\[4\]; int ngates; int reserved; \};"
    assert re.search(decl, host_h) and re.search(decl, KS._text("hamk_exit.hpp"))
    for cpp in ("hamk_api.cpp", "hamk_build.cpp", "hamk_dispatch.cpp", "hamk_comm.cpp", "hamk_codegen.cpp"):
        assert "hipModuleLaunchKernel" not in KS._text(cpp), cpp              # launch_kernel (hamk_host.h) stays the only caller


def test_the_step_loop_has_no_barrier_and_no_lds():
    """Wavefronts of one block leave the step loop at different steps: a block-wide barrier there would hang the block."""
    text = re.sub(r"//[^\n]*", "", KS._text("hamk_exit.hpp"))
    assert "__syncthreads" not in text and "__shared__" not in text and "s_barrier" not in text
    assert "__ballot(alive) == 0" in text and "TRIG_TABLE" not in text


def gate_struct(gates):
    from hamilton_amd import _abi
    arr = (_abi.hamk_gate * max(1, len(gates)))()
    for g, (c, lo, hi) in enumerate(gates):
        arr[g].coord, arr[g].reserved, arr[g].lo, arr[g].hi = c, 0, lo, hi
    return arr


def test_argument_checks(hamk_lib):
    """Every refusal of include/hamk.h, each with its code and a message naming the argument, before any device is looked at;
    nothing to do is HAMK_OK and leaves every array as it was."""
    from hamilton_amd import _abi, api
    L = hamk_lib
    s = api.system_from_spec(E.get("pendulum"))
    q, p = np.array([[0.1, 0.2]]), np.array([[0.3, 0.4]])
    e = new_exits(1, 2, -7.0)
    st = np.full(2, -5, np.int32)
    good = gate_struct([(0, -1.0, 1.0)])
    base = dict(s=s._h, B=2, q=q.ctypes.data, p=p.ctypes.data, dt=0.01, nsteps=5, gates=ctypes.addressof(good), ngates=1, code=e["code"].ctypes.data,
                texit=e["t"].ctypes.data, qexit=e["q"].ctypes.data, pexit=e["p"].ctypes.data, step0=0, status=st.ctypes.data, mem=0)

    def call(**kw):
        return L.hamk_exit_steps(*dict(base, **kw).values())

    def with_gates(gates, **kw):
        arr = gate_struct(gates)
        return call(gates=ctypes.addressof(arr), ngates=len(gates), **kw)

    INV = _abi.HAMK_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    assert call(s=None) == INV and b"handle" in L.hamk_last_error()
    for k in ("q", "p", "gates", "code", "texit"):
        assert call(**{k: None}) == INV and b"null" in L.hamk_last_error(), k
    for k in ("qexit", "pexit"):
        assert call(**{k: None}) == INV and b"qexit" in L.hamk_last_error(), k
    assert call(B=-1) == INV
    assert call(nsteps=-1) == INV and b"nsteps" in L.hamk_last_error()
    for ngates in (0, -1, 5, 1 << 20):
        assert call(ngates=ngates) == INV and b"ngates" in L.hamk_last_error(), ngates
    for coord in (-1, 2, 7):
        assert with_gates([(coord, -1.0, 1.0)]) == INV and b"coord" in L.hamk_last_error(), coord
        assert with_gates([(0, -1.0, 1.0), (1, -1.0, 1.0), (coord, -1.0, 1.0)]) == INV and b"gate 2" in L.hamk_last_error(), coord
    for lo, hi in ((nan, 1.0), (-1.0, nan), (nan, nan)):
        assert with_gates([(0, lo, hi)]) == INV and b"NaN" in L.hamk_last_error()
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (inf, inf), (-inf, -inf), (inf, -inf)):
        assert with_gates([(0, lo, hi)]) == INV and b"lo" in L.hamk_last_error(), (lo, hi)
    for dt in (nan, inf, -inf):
        assert call(dt=dt) == INV and b"dt" in L.hamk_last_error()
    assert call(step0=-1) == INV and b"step0" in L.hamk_last_error()
    assert call(step0=(1 << 52) + 1) == INV and b"2^52" in L.hamk_last_error()
    assert call(mem=7) == INV
    # nothing to do: HAMK_OK with nothing launched (no GPU is needed for that) and nothing written
    before = [x.copy() for x in (q, p, e["code"], e["t"], e["q"], e["p"], st)]
    assert call(B=0) == _abi.HAMK_OK
    assert call(nsteps=0) == _abi.HAMK_OK
    assert with_gates([(0, -inf, inf), (1, -inf, 0.0), (1, 0.0, inf), (0, -1e-300, 1e-300)], nsteps=0, dt=-0.01, qexit=None, pexit=None, status=None,
                      step0=1 << 52, mem=1) == _abi.HAMK_OK
    assert all(np.array_equal(a, b) for a, b in zip(before, (q, p, e["code"], e["t"], e["q"], e["p"], st)))
    # ... and through the binding: the state back unchanged, a new run's Exits, status 0; given Exits come back
    ph, ex = api.exitSteps(0.01, 0, s, api.Phase(q, p), [(0, -1.0, 1.0)])
    assert np.array_equal(ph.positions, q) and np.array_equal(ph.momenta, p)
    assert ex.code.shape == (2,) and ex.t.shape == (2,) and ex.q.shape == (1, 2) and ex.p.shape == (1, 2)
    assert ex.code.dtype == np.int32 and (ex.code == ALIVE).all() and not ex.t.any() and not ex.q.any() and not ex.p.any()
    assert not np.asarray(s.last_status).any()
    given = api.Exits(np.array([1, ALIVE], np.int32), e["t"], e["q"], e["p"])
    ph, ex = api.exitSteps(0.01, 0, s, api.Phase(q, p), [(0, -1.0, 1.0)], exits=given, step0=9)
    assert np.array_equal(ex.code, [1, ALIVE]) and np.array_equal(ex.t, e["t"]) and np.array_equal(ex.q, e["q"])
    assert ex.code is not given.code                                                        # out of place
    for gates in ([], [(2, -1.0, 1.0)], [(0, 1.0, -1.0)], [(0, -1.0, 1.0)] * 5):
        with pytest.raises(api.HamkError):
            api.exitSteps(0.01, 0, s, api.Phase(q, p), gates)                               # refused through the binding too
    if L.hamk_device_count() == 0:                                                          # no CPU fall-back: a real call needs the GPU
        with pytest.raises(api.HamkError):
            api.exitSteps(0.01, 1, s, api.Phase(q, p), [(0, -1.0, 1.0)])


def test_unsupported_handles_name_the_limit(hamk_lib):
    """One trajectory per lane: n <= 16, and no handle whose options state another mapping."""
    from hamilton_amd import _abi, api
    z = np.zeros((20, 2))
    code = np.full(2, ALIVE, np.int32)
    g = gate_struct([(0, -1.0, 1.0)])
    big = api.system_from_spec(E.get("chain20"))
    wave = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_WAVE})
    quad = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_QUAD})
    for s, word in ((big, "n <= 16"), (wave, "HAMK_MAP_WAVE"), (quad, "HAMK_MAP_QUAD")):
        rc = hamk_lib.hamk_exit_steps(s._h, 2, z.ctypes.data, z.ctypes.data, 0.01, 1, ctypes.addressof(g), 1, code.ctypes.data, z.ctypes.data, None, None,
                                      0, None, 0)
        msg = hamk_lib.hamk_last_error().decode()
        assert rc == _abi.HAMK_ERR_UNSUPPORTED and word in msg and "n <= 16" in msg and "exit-time" in msg, (rc, msg)
        assert hamk_lib.hamk_exit_source(s._h) is None and hamk_lib.hamk_exit_build_info(s._h) is None
        with pytest.raises(api.HamkError, match="n <= 16") as err:
            s.exit_source
        assert err.value.code == _abi.HAMK_ERR_UNSUPPORTED
    assert hamk_lib.hamk_exit_source(None) is None and hamk_lib.hamk_exit_build_info(None) is None
    lane = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_LANE})          # the lane mapping stated: fine
    assert "HAMK_INSTANTIATE_EXIT(HamkSys)" in lane.exit_source


# ---------------------------------------------------------------------------------------------------------------------- 1. build
@pytest.mark.parametrize("name", SYSTEMS + ["chain16"])
def test_companion_module_compiles_for_gfx950(hamk_lib, name):
    """The kernel lives in a module of its own: the per-system module keeps its nine function symbols, its nine build_info rows and
    its source; the three other companions are what they were; the new one is the source with the final instantiation replaced."""
    from hamilton_amd import api
    s = api.system_from_spec(E.get(name))
    src, info, symp, lyap, psec = s.source, s.build_info, s.symplectic_source, s.lyapunov_source, s.poincare_source
    head = src[:src.rindex("HAMK_INSTANTIATE(HamkSys)")]
    line = s.exit_build_info
    assert line.count("\n") == 1 and line.endswith("\n")
    m = re.fullmatch(r"hamk_exit_steps_k build=default bytes=(\d+) sgpr_spills=(-?\d+) vgpr_spills=(-?\d+) vgprs=(\d+) functions=(\d+)\n", line)
    assert m, line
    nbytes, _, vspill, vgprs, nfunc = (int(x) for x in m.groups())
    print(name, line.strip())
    assert nfunc == 1, (name, nfunc)                          # every device function inlined into the one kernel
    assert 0 < nbytes < 100 * 1024, (name, nbytes)
    assert 0 < vgprs <= 512 and vspill >= 0
    if name != "chain16":
        assert vspill == 0, (name, vspill)                    # chain8 fits; chain16 spills as the other companions do
    assert s.num_device_functions == 9 and s.build_info == info and len(info.splitlines()) == 9 and s.source == src
    assert s.symplectic_source == symp and symp == head + '#include "hamk_symp.hpp"\nHAMK_INSTANTIATE_SYMP(HamkSys)\n'
    assert s.lyapunov_source == lyap and lyap == head + '#include "hamk_lyap.hpp"\nHAMK_INSTANTIATE_LYAP(HamkSys)\n'
    assert s.poincare_source == psec and psec == head + '#include "hamk_psec.hpp"\nHAMK_INSTANTIATE_PSEC(HamkSys)\n'
    fresh = api.system_from_spec(E.get(name))                                               # ... and without the new companion built
    assert fresh.symplectic_source == symp and fresh.lyapunov_source == lyap and fresh.poincare_source == psec
    assert s.exit_source == head + '#include "hamk_exit.hpp"\nHAMK_INSTANTIATE_EXIT(HamkSys)\n'
    assert s.kernel_bytes("hamk_exit_steps_k") == 0                                         # not a kernel of the per-system module
    assert s.exit_build_info == line                                                        # built once


def test_auto_mapping_keeps_the_stepper_on_the_lane_module(hamk_lib):
    """chain12: AUTO serves small RK4 ensembles on the four-lane kernels; the exit-time module is the lane module's companion."""
    from hamilton_amd import _abi, api
    s = api.system_from_spec(E.get("chain12"))
    assert s.options(8192)["mapping"] == _abi.MAP_QUAD
    s.describe_batch(8192)
    comp = s.exit_source
    assert '#include "hamk_device.hpp"' in comp and "hamk_quad.hpp" not in comp and comp.endswith("HAMK_INSTANTIATE_EXIT(HamkSys)\n")


# ---------------------------------------------------------------------------------------------------------------------- 2. anchors
def test_rotor_anchor(emulate, oracle_lib):
    """Code and side follow the sign of p, lanes at rest keep code -1, exit times from (+-pi - q0) / p within the rounding bound:
    the restatement first, then the kernel."""
    o = oracle_lib.OracleSystem(anchor_spec("rotor"))
    q, p = rotor_inputs()
    r = restate(o, q, p, ROTOR_DT, ROTOR_N, ROTOR_GATES, exits=new_exits(1, ANCHOR_B, -7.0))
    check_rotor(r, "restatement")
    check_rotor(emu_steps(emulate(anchor_system("rotor")), q, p, ROTOR_DT, ROTOR_N, ROTOR_GATES, sentinel=-7.0), "kernel on host")


@pytest.mark.parametrize("case", OSC_CASES, ids=lambda c: "dt%g-n%d" % c)
def test_oscillator_anchor(emulate, oracle_lib, case):
    """Code, theta and the exit state against numpy.roots on the closed-form cubic of the exit step."""
    dt, nsteps = case
    o = oracle_lib.OracleSystem(anchor_spec("oscillator"))
    q, p = osc_inputs()
    gates = [(0, -OSC_C, OSC_C)]
    check_oscillator(restate(o, q, p, dt, nsteps, gates), dt, nsteps, "restatement")
    check_oscillator(emu_steps(emulate(anchor_system("oscillator")), q, p, dt, nsteps, gates), dt, nsteps, "kernel on host")


def test_free_particle_gate_order(emulate, oracle_lib):
    """Two gates violated in one step (the smaller theta wins), an exact tie (the lower index wins), a start outside a gate
    (theta = 0, texit = step0)."""
    o = oracle_lib.OracleSystem(free_spec())
    q, p = free_inputs()
    check_free(restate(o, q, p, FREE_DT, 4, FREE_GATES, exits=new_exits(2, len(FREE_LANES), -7.0), step0=10), "restatement")
    check_free(emu_steps(emulate(anchor_system("free")), q, p, FREE_DT, 4, FREE_GATES, sentinel=-7.0, step0=10), "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 3. values
@pytest.mark.parametrize("name", SYSTEMS)
def test_kernel_on_host_matches_the_restatement(emulate, oracle_lib, name):
    from hamilton_amd import api
    ref = reference(oracle_lib, name)
    got = emu_steps(emulate(api.system_from_spec(E.get(name))), ref["q"], ref["p"], DT, ref["nsteps"], ref["gates"])
    check_against_reference(ref, name, got, "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 4. bits
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_properties_on_host(emulate, oracle_lib, name):
    """Cut invariance, freeze, gate independence, lanes stopped at entry, qexit = pexit = NULL, infinite bounds."""
    from hamilton_amd import api
    ref = reference(oracle_lib, name)
    L = emulate(api.system_from_spec(E.get(name)))
    run_properties(lambda q, p, nsteps, gates, **kw: emu_steps(L, q, p, DT, nsteps, gates, **kw), ref, name)


def test_a_nan_lane_among_healthy_ones_on_host(emulate, oracle_lib):
    from hamilton_amd import api
    ref = reference(oracle_lib, "doublePendulum")
    L = emulate(api.system_from_spec(E.get("doublePendulum")))
    run_nan_lane(lambda q, p, nsteps, gates, **kw: emu_steps(L, q, p, DT, nsteps, gates, **kw), ref, 37)
    # status may be null
    a = emu_steps(L, ref["q"], ref["p"], DT, 20, ref["gates"])
    assert same(a, emu_steps(L, ref["q"], ref["p"], DT, 20, ref["gates"], status=False))
