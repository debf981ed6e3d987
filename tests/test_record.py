"""CPU: trajectory recording fused with RK4 (hamk_record_steps; hamilton_amd/csrc/hamk_rec.hpp) -- its three entry points and their
argument checks, the host's statement of the kernel's signature, the companion module that carries the kernel (compiled for gfx950
here: hiprtc needs no GPU), and the kernel itself run thread by thread on the host (tests/host_emulation/rec_driver.inc appended
to System.record_source, the g++ flags of test_lyapunov.py's `emulate`) against a literal numpy restatement of the scheme over the
oracle's hamEqs (below), against the oracle's own rk4_steps_batch and observe_batch, against the harmonic oscillator's closed
form, and for the bit-level properties the scheme promises.  What this cannot see is the GPU compiler and the host's staging of the
rows (tests/test_gpu_record.py, which imports the restatement, the anchor, the inputs, the bounds and the properties from here)."""
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
from test_lyapunov import anchor_spec, anchor_system, sample_phase

EMU = os.path.join(ROOT, "tests", "host_emulation")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
P = lambda a: None if a is None else a.ctypes.data_as(_dp)
I = lambda a: None if a is None else a.ctypes.data_as(_ip)
LL = ctypes.c_longlong
F = ctypes.c_double
NAMES = ("hamk_record_steps", "hamk_record_source", "hamk_record_build_info")
EPS = 2.2e-16
ST_SINGULAR, ST_NONFINITE = 1, 2
PAYLOAD = np.array([0x7ff8dead0000beef], np.uint64).view(np.float64)[0]          # a NaN whose bits say who wrote it


# ---------------------------------------------------------------------------------------------------------------------- reference
# The row rule of include/hamk.h, on integers alone.  G counts the steps of the whole run: step0 at entry, step0 + s + 1 after the
# call's step s.  Where G is a multiple of `every`, the state after G steps is row G / every: recorded at entry only for step0 == 0
# (row 0), after every step whose G in (step0, step0 + nsteps] is a multiple; rows at or beyond max_rows are dropped.
def row_plan(nsteps, every, max_rows, step0=0):
    """-> [(row, G), ...]: what a call writes, in order.  nsteps = 0 writes nothing (the entry point returns before any launch)."""
    if nsteps == 0:
        return []
    plan = [(0, 0)] if step0 == 0 else []
    plan += [(G // every, G) for G in range(step0 + 1, step0 + nsteps + 1) if G % every == 0]
    return [(k, G) for k, G in plan if k < max_rows]


def rows_filled(nsteps, every, max_rows, step0=0):
    """What the header tells the caller to compute."""
    return min(max_rows, (step0 + nsteps) // every + 1)


def new_bufs(n, nb, rows, fill=0.0, states=True, energy=True):
    return dict(qout=np.full((rows, n, nb), fill) if states else None, pout=np.full((rows, n, nb), fill) if states else None,
                hout=np.full((rows, nb), fill) if energy else None)


# A LITERAL numpy restatement of the scheme of hamilton_amd/csrc/hamk_rec.hpp over the oracle's hamEqs and hamiltonian (the oracle
# itself is not changed): classic RK4 over hamEqs, the rows by row_plan.
def restate(o, q, p, dt, nsteps, every, max_rows, step0=0, bufs=None):
    """-> dict(q, p [n, B]; qout, pout [max_rows, n, B]; hout [max_rows, B]; status [B])."""
    q, p = np.array(q, dtype=np.float64), np.array(p, dtype=np.float64)
    n, nb = q.shape
    b = new_bufs(n, nb, max_rows) if bufs is None else {k: None if v is None else np.array(v) for k, v in bufs.items()}
    st = np.zeros(nb, np.int32)
    due = dict((G, k) for k, G in row_plan(nsteps, every, max_rows, step0))

    def f(a, c):
        dq, dp_, s1 = o.hameqs_batch(a, c, threads=1)
        st[:] |= s1
        return dq, dp_

    def record(G):
        if G in due:
            k = due[G]
            if b["qout"] is not None:
                b["qout"][k], b["pout"][k] = q, p
            if b["hout"] is not None:
                b["hout"][k] = o.observe_batch(q, p, threads=1)[2]

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        record(step0)
        for s in range(nsteps):
            k1 = f(q, p)
            k2 = f(q + 0.5 * dt * k1[0], p + 0.5 * dt * k1[1])
            k3 = f(q + 0.5 * dt * k2[0], p + 0.5 * dt * k2[1])
            k4 = f(q + dt * k3[0], p + dt * k3[1])
            q = q + dt / 6.0 * (k1[0] + 2.0 * k2[0] + 2.0 * k3[0] + k4[0])
            p = p + dt / 6.0 * (k1[1] + 2.0 * k2[1] + 2.0 * k3[1] + k4[1])
            record(step0 + s + 1)
    st[~(np.isfinite(q).all(0) & np.isfinite(p).all(0))] |= ST_NONFINITE
    return dict(q=q, p=p, status=st, **b)


OUT = ("q", "p", "qout", "pout", "hout")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b, keys=OUT):
    """Bit for bit, NaN payloads included; an output that was not asked for is None on both sides."""
    return all((a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and np.array_equal(bits(a[k]), bits(b[k]))) for k in keys)


def lanes(r, w, keys=OUT + ("status",)):
    return {k: None if r[k] is None else r[k][..., w] for k in keys}


def carry(r):
    return dict(qout=r["qout"], pout=r["pout"], hout=r["hout"])


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))))


# The comparison of the kernel with the restatement and the oracle: four systems, B = 257 (two blocks, the second holding one
# lane), dt = 0.01, 20 steps, every = 3, max_rows = 8: rows 0 .. 6 are filled (steps 0, 3, .., 18), row 7 is not, and `every` does not
# divide nsteps.
SYSTEMS = ["pendulum", "doublePendulum", "opcodeZoo", "chain8"]
B = 257
DT, NSTEPS, EVERY, MAX_ROWS = 0.01, 20, 3, 8
FILLED = 7
# hout against the oracle's hamiltonian of the kernel's OWN recorded row: the figure tests/test_gpu_parity.py
# test_hameqs_vs_oracle_ensemble applies to the Hamiltonian, relative to max(1, |H|)
H_BOUND = 1e-11
_reference = {}


def reference(oracle_lib, name):
    """Inputs, the restatement's result and the oracle's own state at every filled row, computed once and shared by every test of
    both modules."""
    if name not in _reference:
        spec = E.get(name)
        o = oracle_lib.OracleSystem(spec)
        q, p = sample_phase(spec, o, 17, B)
        want = restate(o, q, p, DT, NSTEPS, EVERY, MAX_ROWS)
        assert rows_filled(NSTEPS, EVERY, MAX_ROWS) == FILLED
        assert all(np.isfinite(want[k]).all() for k in OUT) and not want["status"].any(), name        # all 257 lanes: none is left out below
        rows = [(q, p)] + [o.rk4_steps_batch(q, p, DT, k * EVERY) for k in range(1, FILLED)]
        _reference[name] = dict(o=o, q=q, p=p, want=want, rows=rows)
    return _reference[name]


def check_against_reference(ref, name, got, what):
    """got: a kernel run on ref's inputs with NaN-payload buffers (a dict like restate's): every lane, every filled row.
    -> the measured figures (state error, hout error), printed before they are held against the bounds."""
    o, want = ref["o"], ref["want"]
    state = max(max(relerr(got["qout"][k], rq), relerr(got["pout"][k], rp)) for k, (rq, rp) in enumerate(ref["rows"]))
    final = max(relerr(got["q"], want["q"]), relerr(got["p"], want["p"]))
    again = max(relerr(got[key][:FILLED], want[key][:FILLED]) for key in ("qout", "pout", "hout"))
    herr = max(relerr(got["hout"][k], o.observe_batch(got["qout"][k], got["pout"][k], threads=1)[2]) for k in range(FILLED))
    print(what, name, "rows vs oracle rk4_steps_batch", state, "bound", STATE_BOUND[name], "| vs restatement: final state", final, "rows", again,
          "| hout vs oracle hamiltonian of the recorded row", herr, "bound", H_BOUND)
    assert np.array_equal(got["status"], want["status"]), (got["status"], want["status"])
    assert same(dict(q=got["qout"][0], p=got["pout"][0]), dict(q=ref["q"], p=ref["p"]), ("q", "p"))          # row 0: the input, bit for bit
    assert state < STATE_BOUND[name], (name, state)
    assert final < STATE_BOUND[name] and again < STATE_BOUND[name], (name, final, again)
    assert max(relerr(want["qout"][k], rq) for k, (rq, _) in enumerate(ref["rows"])) < STATE_BOUND[name]       # the restatement itself
    assert herr <= H_BOUND, (name, herr)
    for key in ("qout", "pout", "hout"):                                                                     # row 7 was never written
        assert (bits(got[key][FILLED:]) == bits(np.array([PAYLOAD]))[0]).all(), key
    return state, herr


# ---- the anchor: the harmonic oscillator --------------------------------------------------------------------------------
# n = 1, inertia 1, f(q) = q, U = x^2 / 2 (test_lyapunov's anchor): hamEqs = (p, -q), and one RK4 step is the matrix test_lyapunov.py
# states, M = [[a, b], [-b, a]] with a = 1 - dt^2 / 2 + dt^4 / 24, b = dt - dt^3 / 6: a rotation scaled by sqrt(a^2 + b^2).  Row k is
# M^(k every) y0, and H = (q^2 + p^2) / 2 of row k is H0 (a^2 + b^2)^(k every).
# Bounds.  One step is four stages of a few roundings each on values no larger than |y|: 8 eps |y| per step, which the (nearly norm
# preserving) later steps carry along unamplified -- (8 G + 2) eps ymax after G steps, the form test_exit.py's rotor uses.  H is
# quadratic in the state, so twice that relative error, plus energy's own handful of roundings: (16 G + 8) eps H.
ANCHOR_B = 64
ANCHOR_CASES = [(0.1, 50, 1, 64), (0.1, 50, 7, 8), (0.01, 400, 25, 17)]        # (dt, nsteps, every, max_rows)


def osc_inputs(nb=ANCHOR_B):
    rng = np.random.default_rng(11)
    return rng.uniform(-2, 2, (1, nb)), rng.uniform(-2, 2, (1, nb))


def check_oscillator(got, case, what, nb=ANCHOR_B):
    """got: a run of `case` from osc_inputs(nb) on NaN-payload buffers.  -> the worst error / bound."""
    dt, nsteps, every, max_rows = case
    q0, p0 = osc_inputs(nb)
    a, b = 1.0 - dt ** 2 / 2 + dt ** 4 / 24, dt - dt ** 3 / 6
    M = np.array([[a, b], [-b, a]])
    y0 = np.concatenate([q0, p0])
    ymax = max(1.0, float(np.hypot(q0, p0).max()))
    h0 = 0.5 * (q0[0] ** 2 + p0[0] ** 2)
    filled = rows_filled(nsteps, every, max_rows)
    worst = 0.0
    assert not got["status"].any()
    for k in range(filled):
        G = k * every
        y = np.linalg.matrix_power(M, G) @ y0
        err = max(float(np.abs(got["qout"][k] - y[:1]).max()), float(np.abs(got["pout"][k] - y[1:]).max()))
        herr = float((np.abs(got["hout"][k] - h0 * (a * a + b * b) ** G) / h0).max())
        worst = max(worst, err / ((8 * G + 2) * EPS * ymax), herr / ((16 * G + 8) * EPS))
        assert err <= (8 * G + 2) * EPS * ymax, (what, case, k, err)
        assert herr <= (16 * G + 8) * EPS, (what, case, k, herr)
    y = np.linalg.matrix_power(M, nsteps) @ y0
    assert max(float(np.abs(got["q"] - y[:1]).max()), float(np.abs(got["p"] - y[1:]).max())) <= (8 * nsteps + 2) * EPS * ymax
    for key in ("qout", "pout", "hout"):
        assert (bits(got[key][filled:]) == bits(np.array([PAYLOAD]))[0]).all(), key
    print(what, "oscillator", case, "rows", filled, "worst error / bound", worst)
    return worst


# ---------------------------------------------------------------------------------------------------------------------- emulation
@pytest.fixture(scope="module")
def emulate(hamk_lib, tmp_path_factory):
    """System -> hamk_rec_steps_k of its companion module on the host."""
    cache = {}
    tmp = tmp_path_factory.mktemp("rec_emu")

    def make(s):
        src = s.record_source
        key = hashlib.sha1(src.encode()).hexdigest()[:16]
        if key not in cache:
            cpp, so = str(tmp / f"{key}.cpp"), str(tmp / f"{key}.so")
            with open(cpp, "w") as fh:
                fh.write(src + open(os.path.join(EMU, "rec_driver.inc")).read())
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-gnu-unique", "-Wno-unknown-pragmas", "-Wno-attributes",
                                   "-include", os.path.join(EMU, "hip_shim.hpp"), "-I" + os.path.join(ROOT, "hamilton_amd", "csrc"),
                                   "-o", so, cpp])
            cache[key] = ctypes.CDLL(so)
        return cache[key]
    return make


def emu_steps(L, q, p, dt, nsteps, every, max_rows, step0=0, bufs=None, fill=0.0, states=True, energy=True, status=True, rows=None):
    """hamk_rec_steps_k on the host, on copies -> a dict like restate's.  bufs: a dict qout, pout, hout to continue in (copied);
    otherwise new buffers of `rows` (default max_rows) rows holding `fill`; states / energy = False: that group is NULL.  As the entry
    point, nothing is launched for nsteps = 0."""
    q, p = (np.ascontiguousarray(a, dtype=np.float64).copy() for a in (q, p))
    n, nb = q.shape
    b = new_bufs(n, nb, max_rows if rows is None else rows, fill, states, energy) if bufs is None else \
        {k: None if v is None else np.array(v) for k, v in bufs.items()}
    st = np.full(nb, -1, np.int32) if status else None
    if nsteps > 0:
        L.emu_rec(P(q), P(p), LL(nb), F(dt), int(nsteps), int(every), int(max_rows), P(b["qout"]), P(b["pout"]), P(b["hout"]), LL(step0), LL(0), I(st))
    return dict(q=q, p=p, status=st, **b)


def run_properties(run, ref, name):
    """What the scheme promises bit for bit, for any way `run(q, p, nsteps, every, max_rows, **kw) -> dict` of running the kernel
    (the host emulation here, hamk_record_steps on the GPU in tests/test_gpu_record.py; kw as emu_steps')."""
    q, p = ref["q"], ref["p"]
    n, nb = q.shape
    one = run(q, p, NSTEPS, EVERY, MAX_ROWS, fill=PAYLOAD)
    untouched = lambda a: bool((bits(a) == bits(np.array([PAYLOAD]))[0]).all())
    assert all(untouched(one[k][FILLED:]) and not np.isnan(one[k][:FILLED]).any() for k in ("qout", "pout", "hout"))
    assert same(dict(q=one["qout"][0], p=one["pout"][0]), dict(q=q, p=p), ("q", "p"))
    # prefix: row k is the q, p of a fresh call with nsteps = k every
    for k in range(1, FILLED):
        r = run(q, p, k * EVERY, EVERY, MAX_ROWS)
        assert same(dict(q=one["qout"][k], p=one["pout"][k]), r, ("q", "p")), k
        assert all(np.array_equal(bits(r[key][:k + 1]), bits(one[key][:k + 1])) for key in ("qout", "pout", "hout")), k
    # cut invariance: N = N1 + N2 with step0 and the buffers carried, a cut off a recorded step (7) and one on it (9)
    for n1 in (7, 9):
        h1 = run(q, p, n1, EVERY, MAX_ROWS, fill=PAYLOAD)
        first = rows_filled(n1, EVERY, MAX_ROWS)
        assert all(untouched(h1[k][first:]) for k in ("qout", "pout", "hout")), n1
        h2 = run(h1["q"], h1["p"], NSTEPS - n1, EVERY, MAX_ROWS, step0=n1, bufs=carry(h1))
        assert same(one, h2), n1
        if one["status"] is not None:
            assert np.array_equal(one["status"], h1["status"] | h2["status"])
        # a continued call leaves the rows of the first call untouched: they are overwritten with the payload in between
        marked = {k: v.copy() for k, v in carry(h1).items()}
        for v in marked.values():
            v[:first] = PAYLOAD
        h3 = run(h1["q"], h1["p"], NSTEPS - n1, EVERY, MAX_ROWS, step0=n1, bufs=marked)
        for k in ("qout", "pout", "hout"):
            assert untouched(h3[k][:first]) and np.array_equal(bits(h3[k][first:]), bits(one[k][first:])), (n1, k)
    # the final state does not depend on every, max_rows, or on which outputs are given
    for every in (1, 3, 21):
        for max_rows in (1, 8):
            r = run(q, p, NSTEPS, every, max_rows, fill=PAYLOAD)
            assert same(one, r, ("q", "p")), (every, max_rows)
            plan = row_plan(NSTEPS, every, max_rows)
            assert all(not np.isnan(r[k][:len(plan)]).any() and untouched(r[k][len(plan):]) for k in ("qout", "pout", "hout")), (every, max_rows)
    only_states = run(q, p, NSTEPS, EVERY, MAX_ROWS, fill=PAYLOAD, energy=False)
    only_h = run(q, p, NSTEPS, EVERY, MAX_ROWS, fill=PAYLOAD, states=False)
    assert same(one, only_states, ("q", "p", "qout", "pout")) and only_states["hout"] is None
    assert same(one, only_h, ("q", "p", "hout")) and only_h["qout"] is None and only_h["pout"] is None
    every1 = run(q, p, NSTEPS, 1, NSTEPS + 1)                                     # every = 1: a row per step, row 3 k is row k of `one`
    assert all(np.array_equal(bits(every1[k][::EVERY]), bits(one[k][:FILLED])) for k in ("qout", "pout", "hout"))
    # guard rows: max_rows + 1 rows of payload, max_rows = 3: rows 0 .. 2 are filled, row 3 keeps its bits, the dropped rows went nowhere
    g = run(q, p, NSTEPS, EVERY, 3, fill=PAYLOAD, rows=4)
    for k in ("qout", "pout", "hout"):
        assert np.array_equal(bits(g[k][:3]), bits(one[k][:3])) and untouched(g[k][3:]), k
    assert same(one, g, ("q", "p"))
    # status = NULL is accepted
    assert same(one, run(q, p, NSTEPS, EVERY, MAX_ROWS, fill=PAYLOAD, status=False))
    return one


def run_nan_lane(run, ref, lane):
    """A NaN lane among healthy ones ends flagged HAMK_ST_NONFINITE; its neighbours keep their bits on q, p and every row."""
    q, p = ref["q"], ref["p"]
    want = run(q, p, NSTEPS, EVERY, MAX_ROWS, step0=5)
    bad = q.copy()
    bad[0, lane] = np.nan
    got = run(bad, p, NSTEPS, EVERY, MAX_ROWS, step0=5)
    keep = np.arange(q.shape[1]) != lane
    assert got["status"][lane] & ST_NONFINITE and not (got["status"][keep] & ST_NONFINITE).any()
    assert same(lanes(got, keep), lanes(want, keep), OUT + ("status",))
    written = [k for k, _ in row_plan(NSTEPS, EVERY, MAX_ROWS, 5)]             # rows 2 .. 7: steps 6, 9, .., 21
    assert written == list(range(2, 8)) and np.isnan(got["qout"][written, 0, lane]).all()         # its rows hold what the arithmetic gives
    assert not got["qout"][:2].any() and not want["hout"][:2].any()          # rows 0 and 1 belong to earlier calls


def run_singular_lane(run, oracle_lib, lane=37):
    """twoBody at r = 0 (the siblings' input: K = diag(mu, mu r^2) is singular there): that lane is flagged HAMK_ST_SINGULAR, the
    other lanes hold the bits of a run in which that lane had an ordinary input."""
    spec = E.get("twoBody")
    o = oracle_lib.OracleSystem(spec)
    q, p = sample_phase(spec, o, 9, B)
    bad_q, bad_p = q.copy(), p.copy()
    bad_q[:, lane] = (0.0, 0.0)
    bad_p[:, lane] = (0.0, 1.0)
    want = run(q, p, 5, 2, 4)
    got = run(bad_q, bad_p, 5, 2, 4)
    keep = np.arange(B) != lane
    assert got["status"][lane] & ST_SINGULAR and not got["status"][keep].any() and not want["status"].any(), got["status"][lane]
    assert same(lanes(got, keep), lanes(want, keep))
    only_h = run(bad_q, bad_p, 1, 5, 1, states=False)                        # one row at entry, one step: energy's solve sees r = 0 too
    assert only_h["status"][lane] & ST_SINGULAR


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
    proto = re.search(r"int hamk_record_steps\(([^)]*)\);", header).group(1)
    assert KS._types(proto, named=True) == ["hamk_system*", "int64_t", "double*", "double*", "double", "int32_t", "int32_t", "int32_t", "double*", "double*",
                                            "double*", "int64_t", "int32_t*", "int32_t"]
    assert re.search(r"const char\* hamk_record_source\(hamk_system\* s\);", header) and re.search(r"const char\* hamk_record_build_info\(hamk_system\* s\);", header)
    c = ctypes
    assert _abi.SIGNATURES["hamk_record_steps"] == (c.c_int, [c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_double, c.c_int32, c.c_int32, c.c_int32,
                                                              c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_int32])
    assert _abi.SIGNATURES["hamk_record_source"][0] is c.c_char_p and _abi.SIGNATURES["hamk_record_build_info"][0] is c.c_char_p
    assert "hamk_record_steps" in raw[:raw.index("#define HAMK_H")]                       # the header comment's table of entry points
    assert callable(api.recordSteps) and isinstance(api.System.record_source, property) and isinstance(api.System.record_build_info, property)
    hpp = open(os.path.join(ROOT, "include", "hamilton.hpp")).read()
    hs = open(os.path.join(ROOT, "bindings", "haskell", "Numeric", "Hamilton", "HIP.hs")).read()
    assert "hamk_record_steps" in hpp and "recordSteps" in hpp
    assert 'foreign import ccall safe "hamk_record_steps"' in hs and "recordStepsBatch" in hs


def test_host_signature_equals_the_kernel(hamk_lib):
    """The host states the kernel's parameter list once, in namespace sig_rec of hamk_host.h (namespace sig keeps its eleven
    entries); launch_rec builds the argument array from it.  Text only, as tests/test_kernel_signatures.py."""
    device = KS.device_kernels("hamk_rec.hpp")
    assert list(device) == ["hamk_rec_steps_k"]
    host_h = KS._text("hamk_host.h")
    body = re.search(r"namespace sig_rec \{(.*?)\}  // namespace sig_rec", host_h, re.S).group(1)
    host = {m.group(1): KS._types(m.group(2), named=False) for m in re.finditer(r"using (hamk_\w+_k) = void\(([^)]*)\);", body)}
    assert host == device
    assert device["hamk_rec_steps_k"] == ["double*", "double*", "long long", "double", "int", "int", "int", "double*", "double*", "double*", "long long",
                                          "long long", "int*"]
    assert len(re.findall(r"using hamk_rec_steps_k\b", host_h)) == 1 and "hamk_rec_steps_k" not in KS.host_table()
    assert len(KS.host_table()) == 11
    assert "launch_kernel<sig_rec::hamk_rec_steps_k>::on(" in KS._text("hamk_dispatch.cpp")
    for cpp in ("hamk_api.cpp", "hamk_build.cpp", "hamk_dispatch.cpp", "hamk_comm.cpp", "hamk_codegen.cpp"):
        assert "hipModuleLaunchKernel" not in KS._text(cpp), cpp              # launch_kernel (hamk_host.h) stays the only caller


def test_the_header_shares_the_step_and_needs_no_lds():
    """The right-hand side is not spelled again: the step is hamk_fused_rk4.hpp's, without dense output; no barrier, no LDS, plain
    launch bounds."""
    raw = KS._text("hamk_rec.hpp")
    text = re.sub(r"//[^\n]*", "", raw)
    assert "ham_eqs<" not in raw and "__syncthreads" not in raw and "__shared__" not in raw and "s_barrier" not in raw
    assert '#include "hamk_fused_rk4.hpp"' in text and "HAMK_RK4_STAGES(S, 0," in text and "TRIG_TABLE" not in text
    assert len(re.findall(r"HAMK_RK4_STAGES\(", text)) == 1 and len(re.findall(r"energy<S>\(", text)) == 1          # one copy of each
    assert "__launch_bounds__(256) hamk_rec_steps_k" in text and "#define HAMK_INSTANTIATE_REC(S)" in text
    assert "__builtin_nontemporal" not in text                                                                    # plain stores


def test_argument_checks(hamk_lib):
    """Every refusal of include/hamk.h, each with its code and a message naming the argument, before any device is looked at;
    nothing to do is HAMK_OK; every array is left as it was."""
    from hamilton_amd import _abi, api
    L = hamk_lib
    s = api.system_from_spec(E.get("pendulum"))
    q, p = np.array([[0.1, 0.2]]), np.array([[0.3, 0.4]])
    b = new_bufs(1, 2, 4, -7.0)
    st = np.full(2, -5, np.int32)
    base = dict(s=s._h, B=2, q=q.ctypes.data, p=p.ctypes.data, dt=0.01, nsteps=5, every=2, max_rows=4, qout=b["qout"].ctypes.data,
                pout=b["pout"].ctypes.data, hout=b["hout"].ctypes.data, step0=0, status=st.ctypes.data, mem=0)
    before = [x.copy() for x in (q, p, b["qout"], b["pout"], b["hout"], st)]

    def call(**kw):
        return L.hamk_record_steps(*dict(base, **kw).values())

    INV = _abi.HAMK_ERR_INVALID
    nan, inf = float("nan"), float("inf")
    assert call(s=None) == INV and b"handle" in L.hamk_last_error()
    for k in ("q", "p"):
        assert call(**{k: None}) == INV and b"null" in L.hamk_last_error(), k
    for k in ("qout", "pout"):
        assert call(**{k: None}) == INV and b"qout" in L.hamk_last_error(), k
        assert call(**{k: None}, hout=None) == INV, k
    assert call(qout=None, pout=None, hout=None) == INV and b"nothing to record" in L.hamk_last_error()
    assert call(B=-1) == INV
    assert call(nsteps=-1) == INV and b"nsteps" in L.hamk_last_error()
    for every in (0, -3):
        assert call(every=every) == INV and b"every" in L.hamk_last_error()
    for max_rows in (0, -1):
        assert call(max_rows=max_rows) == INV and b"max_rows" in L.hamk_last_error()
    assert call(max_rows=0x7fffffff, B=1 << 18) == INV and b"2^48" in L.hamk_last_error()          # 2^31 * 2^18 > 2^48
    assert call(max_rows=(1 << 30) + 1, B=1 << 18) == INV and b"2^48" in L.hamk_last_error()       # just beyond
    assert call(step0=-1) == INV and b"step0" in L.hamk_last_error()
    assert call(step0=(1 << 52) + 1) == INV and b"2^52" in L.hamk_last_error()
    for dt in (nan, inf, -inf):
        assert call(dt=dt) == INV and b"dt" in L.hamk_last_error()
    assert call(mem=7) == INV
    # nothing to do: HAMK_OK with nothing launched (no GPU is needed for that) and nothing written, row 0 included
    assert call(B=0) == _abi.HAMK_OK
    assert call(nsteps=0) == _abi.HAMK_OK
    assert call(nsteps=0, dt=-0.01, every=0x7fffffff, max_rows=1, qout=None, pout=None, status=None, step0=1 << 52, mem=1) == _abi.HAMK_OK
    assert call(nsteps=0, hout=None, max_rows=1 << 30, B=1 << 18, mem=1) == _abi.HAMK_OK           # exactly 2^48 elements
    assert all(np.array_equal(x, y) for x, y in zip(before, (q, p, b["qout"], b["pout"], b["hout"], st)))
    # ... and through the binding: the state back unchanged, a new run's Record with no row filled, status 0; a given Record comes back
    ph, rec = api.recordSteps(0.01, 0, 2, s, api.Phase(q, p), energy=True)
    assert np.array_equal(ph.positions, q) and np.array_equal(ph.momenta, p)
    assert rec.positions.shape == (1, 1, 2) and rec.momenta.shape == (1, 1, 2) and rec.energy.shape == (1, 2) and rec.rows == 0
    assert not rec.positions.any() and not rec.energy.any() and not np.asarray(s.last_status).any()
    ph, rec = api.recordSteps(0.01, 0, 2, s, api.Phase(q, p), max_rows=5, states=False, energy=True)
    assert rec.positions is None and rec.momenta is None and rec.energy.shape == (5, 2)
    given = api.Record(b["qout"], b["pout"], b["hout"], 3)
    ph, rec = api.recordSteps(0.01, 0, 2, s, api.Phase(q, p), record=given, step0=5)
    assert rec.rows == 3 and np.array_equal(rec.positions, b["qout"]) and np.array_equal(rec.energy, b["hout"]) and rec.positions is not given.positions
    ph, rec = api.recordSteps(0.01, 0, 2, s, api.Phase(q[:, 0], p[:, 0]), max_rows=3, energy=True)             # one trajectory: no B axis
    assert ph.positions.shape == (1,) and rec.positions.shape == (3, 1) and rec.energy.shape == (3,)
    for kw in (dict(states=False), dict(max_rows=0), dict(record=api.Record(b["qout"], None, None, 0)), dict(record=api.Record(b["qout"][:, :, :1], b["pout"], None, 0))):
        with pytest.raises(ValueError):
            api.recordSteps(0.01, 0, 2, s, api.Phase(q, p), **kw)
    with pytest.raises(ValueError):
        api.recordSteps(0.01, 0, 0, s, api.Phase(q, p))
    if L.hamk_device_count() == 0:                                                          # no CPU fall-back: a real call needs the GPU
        with pytest.raises(api.HamkError):
            api.recordSteps(0.01, 1, 1, s, api.Phase(q, p))


def test_unsupported_handles_name_the_limit(hamk_lib):
    """One trajectory per lane: n <= 16, and no handle whose options state another mapping."""
    from hamilton_amd import _abi, api
    z = np.zeros((20, 2))
    h = np.zeros((1, 2))
    big = api.system_from_spec(E.get("chain20"))
    wave = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_WAVE})
    quad = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_QUAD})
    for s, word in ((big, "n <= 16"), (wave, "HAMK_MAP_WAVE"), (quad, "HAMK_MAP_QUAD")):
        rc = hamk_lib.hamk_record_steps(s._h, 2, z.ctypes.data, z.ctypes.data, 0.01, 1, 1, 1, None, None, h.ctypes.data, 0, None, 0)
        msg = hamk_lib.hamk_last_error().decode()
        assert rc == _abi.HAMK_ERR_UNSUPPORTED and word in msg and "n <= 16" in msg and "recording" in msg, (rc, msg)
        assert not h.any()
        assert hamk_lib.hamk_record_source(s._h) is None and hamk_lib.hamk_record_build_info(s._h) is None
        with pytest.raises(api.HamkError, match="n <= 16") as err:
            s.record_source
        assert err.value.code == _abi.HAMK_ERR_UNSUPPORTED
    assert hamk_lib.hamk_record_source(None) is None and hamk_lib.hamk_record_build_info(None) is None
    lane = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_LANE})          # the lane mapping stated: fine
    assert "HAMK_INSTANTIATE_REC(HamkSys)" in lane.record_source


# ---------------------------------------------------------------------------------------------------------------------- 1. build
@pytest.mark.parametrize("name", SYSTEMS + ["chain16"])
def test_companion_module_compiles_for_gfx950(hamk_lib, name):
    """The kernel lives in a module of its own: the per-system module keeps its nine function symbols, its nine build_info rows and
    its source; the four other companions are what they were; the new one is the source with the final instantiation replaced."""
    from hamilton_amd import api
    s = api.system_from_spec(E.get(name))
    src, info = s.source, s.build_info
    others = dict(symp=s.symplectic_source, lyap=s.lyapunov_source, psec=s.poincare_source, exit=s.exit_source)
    head = src[:src.rindex("HAMK_INSTANTIATE(HamkSys)")]
    line = s.record_build_info
    assert line.count("\n") == 1 and line.endswith("\n")
    m = re.fullmatch(r"hamk_rec_steps_k build=default bytes=(\d+) sgpr_spills=(-?\d+) vgpr_spills=(-?\d+) vgprs=(\d+) functions=(\d+)\n", line)
    assert m, line
    nbytes, _, vspill, vgprs, nfunc = (int(x) for x in m.groups())
    print(name, line.strip())
    assert nfunc == 1, (name, nfunc)                          # every device function inlined into the one kernel
    # the step and the energy, one copy each: below twice the largest sibling's bound (100 KiB for the step alone)
    assert 0 < nbytes < 200 * 1024, (name, nbytes)
    assert 0 < vgprs <= 512 and vspill >= 0
    if name != "chain16":
        assert vspill == 0, (name, vspill)                    # chain8 fits; chain16 spills as the other companions do
    assert s.num_device_functions == 9 and s.build_info == info and len(info.splitlines()) == 9 and s.source == src
    for kind, text in others.items():
        assert text == head + f'#include "hamk_{kind}.hpp"\nHAMK_INSTANTIATE_{kind.upper()}(HamkSys)\n', kind
    assert (s.symplectic_source, s.lyapunov_source, s.poincare_source, s.exit_source) == tuple(others.values())
    assert s.record_source == head + '#include "hamk_rec.hpp"\nHAMK_INSTANTIATE_REC(HamkSys)\n'
    assert s.kernel_bytes("hamk_rec_steps_k") == 0                                          # not a kernel of the per-system module
    assert s.record_build_info == line                                                      # built once


def test_auto_mapping_keeps_the_stepper_on_the_lane_module(hamk_lib):
    """chain12: AUTO serves small RK4 ensembles on the four-lane kernels; the recording module is the lane module's companion."""
    from hamilton_amd import _abi, api
    s = api.system_from_spec(E.get("chain12"))
    assert s.options(8192)["mapping"] == _abi.MAP_QUAD
    s.describe_batch(8192)
    comp = s.record_source
    assert '#include "hamk_device.hpp"' in comp and "hamk_quad.hpp" not in comp and comp.endswith("HAMK_INSTANTIATE_REC(HamkSys)\n")


# ---------------------------------------------------------------------------------------------------------------------- 2. the row rule
def test_row_rule_on_paper():
    """row_plan against cases worked out by hand, and against the count the header gives the caller."""
    assert row_plan(3, 1, 10) == [(0, 0), (1, 1), (2, 2), (3, 3)]                        # every = 1: a row per step, and row 0
    assert row_plan(3, 5, 10) == [(0, 0)]                                                # every > nsteps: the initial state alone
    assert row_plan(3, 5, 10, step0=3) == [(1, 5)]                                       # ... the next call reaches step 5
    assert row_plan(7, 3, 10, step0=6) == [(3, 9), (4, 12)]                              # step0 a multiple of every: row 2 is the earlier call's
    assert row_plan(6, 3, 10, step0=7) == [(3, 9), (4, 12)]                              # step0 no multiple
    assert row_plan(1, 3, 10, step0=7) == []                                             # no recorded step in range
    assert row_plan(5, 1, 3) == [(0, 0), (1, 1), (2, 2)]                                 # rows 3, 4, 5 dropped
    assert row_plan(5, 1, 3, step0=2) == [] and row_plan(5, 2, 3, step0=1) == [(1, 2), (2, 4)]
    assert row_plan(0, 1, 3) == []                                                       # nothing to do: row 0 is not written either
    assert row_plan(NSTEPS, EVERY, MAX_ROWS) == [(k, 3 * k) for k in range(7)]
    for nsteps, every, max_rows in ((20, 3, 8), (20, 3, 3), (20, 1, 64), (20, 21, 8), (21, 21, 8), (9, 3, 8)):
        assert len(row_plan(nsteps, every, max_rows)) == rows_filled(nsteps, every, max_rows)
        for n1 in range(1, nsteps):                                                      # a cut run writes the one-call rows, each once
            assert row_plan(n1, every, max_rows) + row_plan(nsteps - n1, every, max_rows, step0=n1) == row_plan(nsteps, every, max_rows)


def test_restatement_on_paper(oracle_lib):
    """The restatement on the oscillator: rows where row_plan says, each the state of that many oracle RK4 steps; others untouched."""
    o = oracle_lib.OracleSystem(anchor_spec("oscillator"))
    q, p = osc_inputs(5)
    for nsteps, every, max_rows, step0 in ((3, 1, 10, 0), (3, 5, 10, 0), (7, 3, 10, 6), (6, 3, 10, 7), (5, 1, 3, 0)):
        r = restate(o, q, p, 0.1, nsteps, every, max_rows, step0, bufs=new_bufs(1, 5, max_rows, PAYLOAD))
        plan = dict(row_plan(nsteps, every, max_rows, step0))
        for k in range(max_rows):
            if k in plan:
                wq, wp = (q, p) if plan[k] == step0 else o.rk4_steps_batch(q, p, 0.1, plan[k] - step0)
                assert relerr(r["qout"][k], wq) < 1e-14 and relerr(r["pout"][k], wp) < 1e-14
                assert relerr(r["hout"][k], 0.5 * (r["qout"][k][0] ** 2 + r["pout"][k][0] ** 2)) < 1e-15
            else:
                assert np.isnan(r["qout"][k]).all() and np.isnan(r["pout"][k]).all() and np.isnan(r["hout"][k]).all()


# ---------------------------------------------------------------------------------------------------------------------- 3. anchor
@pytest.mark.parametrize("case", ANCHOR_CASES, ids=lambda c: "dt%g-n%d-every%d-rows%d" % c)
def test_oscillator_anchor(emulate, oracle_lib, case):
    """Row k is the (k every)-th power of the RK4 matrix applied to the start; H of row k is H0 (a^2 + b^2)^(k every): the
    restatement first, then the kernel."""
    dt, nsteps, every, max_rows = case
    o = oracle_lib.OracleSystem(anchor_spec("oscillator"))
    q, p = osc_inputs()
    check_oscillator(restate(o, q, p, dt, nsteps, every, max_rows, bufs=new_bufs(1, ANCHOR_B, max_rows, PAYLOAD)), case, "restatement")
    check_oscillator(emu_steps(emulate(anchor_system("oscillator")), q, p, dt, nsteps, every, max_rows, fill=PAYLOAD), case, "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 4. values
@pytest.mark.parametrize("name", SYSTEMS)
def test_kernel_on_host_matches_the_oracle(emulate, oracle_lib, name):
    """Measured on the host emulation (state rows vs rk4_steps_batch relative to max(1, |y|); hout vs the oracle's hamiltonian of the
    recorded row relative to max(1, |H|)): see DESIGN.md section 15."""
    from hamilton_amd import api
    ref = reference(oracle_lib, name)
    got = emu_steps(emulate(api.system_from_spec(E.get(name))), ref["q"], ref["p"], DT, NSTEPS, EVERY, MAX_ROWS, fill=PAYLOAD)
    check_against_reference(ref, name, got, "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 5. bits
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_properties_on_host(emulate, oracle_lib, name):
    """Prefix, cut invariance on and off a recorded step, independence of every / max_rows / the outputs given, guard rows, rows
    of an earlier call, status = NULL."""
    from hamilton_amd import api
    ref = reference(oracle_lib, name)
    L = emulate(api.system_from_spec(E.get(name)))
    run_properties(lambda q, p, nsteps, every, max_rows, **kw: emu_steps(L, q, p, DT, nsteps, every, max_rows, **kw), ref, name)


def test_a_nan_lane_and_a_singular_lane_on_host(emulate, oracle_lib):
    from hamilton_amd import api
    ref = reference(oracle_lib, "doublePendulum")
    L = emulate(api.system_from_spec(E.get("doublePendulum")))
    run_nan_lane(lambda q, p, nsteps, every, max_rows, **kw: emu_steps(L, q, p, DT, nsteps, every, max_rows, **kw), ref, 37)
    L2 = emulate(api.system_from_spec(E.get("twoBody")))
    run_singular_lane(lambda q, p, nsteps, every, max_rows, **kw: emu_steps(L2, q, p, DT, nsteps, every, max_rows, **kw), oracle_lib)


def test_row_base_addresses_the_staged_rows(emulate, oracle_lib):
    """What the host's staging relies on: with the three pointers at the call's first row and row_base = that row, the kernel writes
    the same bits into a buffer that holds only the rows this call fills."""
    from hamilton_amd import api
    ref = reference(oracle_lib, "doublePendulum")
    L = emulate(api.system_from_spec(E.get("doublePendulum")))
    q, p = ref["q"], ref["p"]
    n, nb = q.shape
    h1 = emu_steps(L, q, p, DT, 7, EVERY, MAX_ROWS)
    whole = emu_steps(L, h1["q"], h1["p"], DT, 13, EVERY, MAX_ROWS, step0=7, bufs=new_bufs(n, nb, MAX_ROWS, PAYLOAD))
    first, last = 7 // EVERY + 1, min(MAX_ROWS - 1, 20 // EVERY)
    assert (first, last) == (3, 6)
    part = new_bufs(n, nb, last - first + 1, PAYLOAD)
    q2, p2, st = h1["q"].copy(), h1["p"].copy(), np.zeros(nb, np.int32)
    L.emu_rec(P(q2), P(p2), LL(nb), F(DT), 13, EVERY, MAX_ROWS, P(part["qout"]), P(part["pout"]), P(part["hout"]), LL(7), LL(first), I(st))
    assert np.array_equal(q2, whole["q"]) and np.array_equal(p2, whole["p"])
    for k in ("qout", "pout", "hout"):
        assert np.array_equal(bits(part[k]), bits(whole[k][first:last + 1])) and not np.isnan(part[k]).any(), k
