"""CPU: largest-Lyapunov-exponent stepping fused with RK4 (hamk_lyapunov_steps; hamilton_amd/csrc/hamk_lyap.hpp) -- its three entry
points and their argument checks, the host's statement of the kernel's signature, the companion module that carries the kernel
(compiled for gfx950 here: hiprtc needs no GPU), and the kernel itself run thread by thread on the host
(tests/host_emulation/lyap_driver.inc appended to System.lyapunov_source, the g++ flags of test_symplectic.py's `emulate`) against
a literal numpy restatement of the scheme over the oracle's hamEqs (below), against two analytic anchors, and for the bit-level
properties the scheme promises.  What this cannot see is the GPU compiler (tests/test_gpu_lyapunov.py, which imports the
restatement, the anchors and the inputs from this module)."""
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

EMU = os.path.join(ROOT, "tests", "host_emulation")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
P = lambda a: a.ctypes.data_as(_dp)
I = lambda a: None if a is None else a.ctypes.data_as(_ip)
LL = ctypes.c_longlong
F = ctypes.c_double
NAMES = ("hamk_lyapunov_steps", "hamk_lyapunov_source", "hamk_lyapunov_build_info")


# ---------------------------------------------------------------------------------------------------------------------- reference
# A LITERAL numpy restatement of the scheme of hamilton_amd/csrc/hamk_lyap.hpp over the oracle's hamEqs (the oracle itself is not
# changed).  Per trajectory: y = [q; p], a deviation w = [wq; wp] used as given, a running logsum.  One interval:
#   1. s = y + d0 w
#   2. `every` times:  y <- RK4(y, dt);  s <- RK4(s, dt)        (classic RK4 over hamEqs)
#   3. delta = s - y;  d = sqrt(sum_j delta_j^2);  logsum += log(d / d0);  w = delta / d
# status: OR of the status of every hamEqs evaluation (1 = singular K), plus 2 where the final state, w or logsum is not finite.
def restate(o, q, p, wq, wp, dt, nintervals, every, d0, logsum, perturb=None):
    """-> (q, p, wq, wp, logsum, status); q, p, wq, wp are [n, B], logsum [B].  perturb: a numpy Generator -- every hamEqs
    output is multiplied by 1 +- 1e-12, the signs drawn from it (the sensitivity run of `reference` below)."""
    q, p, wq, wp = (np.array(a, dtype=np.float64) for a in (q, p, wq, wp))
    logsum = np.array(logsum, dtype=np.float64)
    st = np.zeros(q.shape[1], np.int32)

    def f(a, b):
        dq, dp, s1 = o.hameqs_batch(a, b, threads=1)
        st[:] |= s1
        if perturb is not None:
            dq = dq * (1.0 + 1e-12 * perturb.choice([-1.0, 1.0], size=dq.shape))
            dp = dp * (1.0 + 1e-12 * perturb.choice([-1.0, 1.0], size=dp.shape))
        return dq, dp

    def rk4(a, b):
        k1 = f(a, b)
        k2 = f(a + 0.5 * dt * k1[0], b + 0.5 * dt * k1[1])
        k3 = f(a + 0.5 * dt * k2[0], b + 0.5 * dt * k2[1])
        k4 = f(a + dt * k3[0], b + dt * k3[1])
        return (a + dt / 6.0 * (k1[0] + 2.0 * k2[0] + 2.0 * k3[0] + k4[0]), b + dt / 6.0 * (k1[1] + 2.0 * k2[1] + 2.0 * k3[1] + k4[1]))

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(nintervals):
            sq, sp = q + d0 * wq, p + d0 * wp
            for _ in range(every):
                q, p = rk4(q, p)
                sq, sp = rk4(sq, sp)
            dq, dp = sq - q, sp - p
            d = np.sqrt((dq * dq).sum(0) + (dp * dp).sum(0))
            logsum = logsum + np.log(d / d0)
            wq, wp = dq / d, dp / d
        fin = np.isfinite(q).all(0) & np.isfinite(p).all(0) & np.isfinite(wq).all(0) & np.isfinite(wp).all(0) & np.isfinite(logsum)
    st[~fin] |= 2
    return q, p, wq, wp, logsum, st


def sample_phase(spec, o, start, B):
    """test_gpu_symplectic.sample_phase: the chains' sampling box has qd = 0, so they get a velocity offset."""
    q, qd = E.sample_config(spec, start, B)
    if spec.name.startswith("chain"):
        qd = qd + 0.4 * np.cos(1.0 + np.arange(spec.n * B, dtype=np.float64).reshape(spec.n, B))
    return q, o.to_phase_batch(q, qd)


def unit_w(n, B, seed):
    """A random unit deviation per trajectory (Euclidean norm over all 2n components) from a fixed seed -> wq, wp [n, B]."""
    w = np.random.default_rng(seed).standard_normal((2 * n, B))
    w /= np.sqrt((w * w).sum(0))
    return np.ascontiguousarray(w[:n]), np.ascontiguousarray(w[n:])


def relstate(gq, gp, rq, rp):
    """The state error test_gpu_symplectic.py holds against STATE_BOUND: relative to max(1, |y|), the largest over all lanes."""
    return float(max((np.abs(gq - rq) / np.maximum(1.0, np.abs(rq))).max(), (np.abs(gp - rp) / np.maximum(1.0, np.abs(rp))).max()))


# The comparison of the kernel with the restatement: four systems, B = 257 (two blocks, the second holding one lane), dt = 0.01,
# 4 intervals of 5 steps, two sizes of d0, a random unit w.
SYSTEMS = ["pendulum", "doublePendulum", "opcodeZoo", "chain8"]
B = 257
DT, NINT, EVERY = 0.01, 4, 5
D0S = [1e-4, 1e-6]
_reference = {}


def reference(oracle_lib, name, d0):
    """Inputs, the restatement's result and the bounds for (system, d0), computed once and shared by every test of both modules.
    State: the oracle's own rk4_steps_batch.  logsum and w: the restatement a second time with every hamEqs output multiplied by
    1 +- 1e-12 (fixed-seed signs) -- 1e-12 is the tolerance ladder's own hamEqs figure -- and the bound is
    4 x the largest |difference| of logsum (resp. w) between the two runs: delta = s - y amplifies a relative error of the
    right-hand side by |y| / d0, so the bound grows as d0 shrinks; the factor 4 covers random signs against a systematic offset.
    Measured (largest over the four systems; the bounds are 4 x these figures):
        between the two restatement runs      d0 = 1e-6: |dlogsum| 1.0e-6, |dw| 1.1e-6;    d0 = 1e-4: |dlogsum| 1.0e-8, |dw| 1.1e-8
        kernel on the host - restatement      d0 = 1e-6: |dlogsum| 5.3e-9, |dw| 5.3e-9;    d0 = 1e-4: |dlogsum| 4.7e-11, |dw| 8.0e-11
        kernel on an MI355X - restatement     d0 = 1e-6: |dlogsum| 5.3e-9, |dw| 5.5e-9;    d0 = 1e-4: |dlogsum| 4.7e-11, |dw| 8.0e-11
    (tests/test_gpu_lyapunov.py)."""
    if (name, d0) not in _reference:
        spec = E.get(name)
        o = oracle_lib.OracleSystem(spec)
        q, p = sample_phase(spec, o, 17, B)
        wq, wp = unit_w(spec.n, B, 20261019)
        zero = np.zeros(B)
        want = restate(o, q, p, wq, wp, DT, NINT, EVERY, d0, zero)
        other = restate(o, q, p, wq, wp, DT, NINT, EVERY, d0, zero, perturb=np.random.default_rng(7))
        assert all(np.isfinite(a).all() for a in want[:5]) and not want[5].any(), name      # all 257 lanes: none is left out below
        _reference[(name, d0)] = dict(
            q=q, p=p, wq=wq, wp=wp, want=want, state=o.rk4_steps_batch(q, p, DT, NINT * EVERY),
            logsum_bound=4.0 * float(np.abs(want[4] - other[4]).max()),
            w_bound=4.0 * float(max(np.abs(want[2] - other[2]).max(), np.abs(want[3] - other[3]).max())))
    return _reference[(name, d0)]


def check_against_reference(ref, name, got, what):
    """got = (q, p, wq, wp, logsum, status) of a kernel run on ref's inputs: every lane, every output."""
    rq, rp, rwq, rwp, rls, rst = ref["want"]
    state = relstate(got[0], got[1], *ref["state"])
    dls = float(np.abs(got[4] - rls).max())
    dw = float(max(np.abs(got[2] - rwq).max(), np.abs(got[3] - rwp).max()))
    print(what, name, "state err", state, "|dlogsum|", dls, "bound", ref["logsum_bound"], "|dw|", dw, "bound", ref["w_bound"])
    assert np.array_equal(got[5], rst), (got[5], rst)
    assert state < STATE_BOUND[name], (name, state)
    assert relstate(rq, rp, *ref["state"]) < STATE_BOUND[name]
    assert dls <= ref["logsum_bound"], (name, dls, ref["logsum_bound"])
    assert dw <= ref["w_bound"], (name, dw, ref["w_bound"])


# ---- analytic anchors ------------------------------------------------------------------------------------------------
# n = 1, inertia 1, f(q) = q: H = p^2 / 2 + U(x).
#   saddle, U = -x^2 / 2:     hamEqs = (p, x); (1, 1) / sqrt 2 is an eigenvector of every RK4 step, multiplied by
#                             R = 1 + dt + dt^2 / 2 + dt^3 / 6 + dt^4 / 24  ->  logsum = N log R, N = nintervals * every
#   oscillator, U = +x^2 / 2: hamEqs = (p, -x); the RK4 map is a rotation scaled by sqrt(1 - dt^6 / 72 + dt^8 / 576), so for ANY
#                             unit w  logsum = N / 2 log1p(-dt^6 / 72 + dt^8 / 576)
# Bound: N (8 eps ymax / d0 + 32 eps), eps = 2.2e-16, ymax = max(1, largest final |q|, |p| of the ensemble): the first term is the
# cancellation in s - y, the second the step's own roundings.  The restatement is inside it by a factor of 100 or more in every
# case (worst 5.5e-9 against 3.5e-6).
EPS = 2.2e-16
ANCHOR_B = 64
ANCHOR_CASES = [(0.01, 10, 20, 1e-6), (0.1, 5, 8, 1e-6), (0.1, 5, 8, 1e-3)]        # (dt, every, nintervals, d0)
ANCHOR_KINDS = ["saddle", "oscillator"]


def anchor_spec(kind):
    sign = -0.5 if kind == "saddle" else 0.5
    return E.SystemSpec(name=kind, m=1, n=1, inertia=(1.0,), f=lambda q, ops: [q[0]], u=lambda z, ops: sign * z[0] * z[0],
                        u_space=0, q0=(0.0,), qd0=(0.0,))


_anchor_systems = {}


def anchor_system(kind):
    """The library's handle, by mkSystem (one per kind and process)."""
    from hamilton_amd import api
    if kind not in _anchor_systems:
        sign = -0.5 if kind == "saddle" else 0.5
        _anchor_systems[kind] = api.mkSystem([1.0], lambda q: [q[0]], lambda q: sign * q[0] * q[0], 1)
    return _anchor_systems[kind]


def anchor_inputs(kind, start):
    """start: "zero" (y = 0) or "random" (y drawn from [-2, 2]) -> q, p, wq, wp [1, ANCHOR_B]."""
    rng = np.random.default_rng(11)
    q, p = (np.zeros((1, ANCHOR_B)), np.zeros((1, ANCHOR_B))) if start == "zero" else (rng.uniform(-2, 2, (1, ANCHOR_B)), rng.uniform(-2, 2, (1, ANCHOR_B)))
    if kind == "saddle":
        wq = wp = np.full((1, ANCHOR_B), 1.0 / np.sqrt(2.0))
    else:
        wq, wp = unit_w(1, ANCHOR_B, 13)
    return q, p, wq.copy(), wp.copy()


def anchor_expected(kind, dt, N):
    if kind == "saddle":
        return N * np.log(1.0 + dt + dt ** 2 / 2 + dt ** 3 / 6 + dt ** 4 / 24)
    return N * 0.5 * np.log1p(-dt ** 6 / 72 + dt ** 8 / 576)


def check_anchor(kind, case, got, what):
    """got = (q, p, wq, wp, logsum, status) from zero logsum: every lane's logsum within the bound of the closed form."""
    dt, every, nint, d0 = case
    N = nint * every
    ymax = max(1.0, float(np.abs(got[0]).max()), float(np.abs(got[1]).max()))
    bound = N * (8 * EPS * ymax / d0 + 32 * EPS)
    err = float(np.abs(got[4] - anchor_expected(kind, dt, N)).max())
    print(what, kind, case, "logsum err", err, "bound", bound)
    assert not got[5].any()
    assert err <= bound, (what, kind, case, err, bound)


# ---------------------------------------------------------------------------------------------------------------------- emulation
@pytest.fixture(scope="module")
def emulate(hamk_lib, tmp_path_factory):
    """System -> hamk_lyap_steps_k of its companion module on the host."""
    cache = {}
    tmp = tmp_path_factory.mktemp("lyap_emu")

    def make(s):
        src = s.lyapunov_source
        key = hashlib.sha1(src.encode()).hexdigest()[:16]
        if key not in cache:
            cpp, so = str(tmp / f"{key}.cpp"), str(tmp / f"{key}.so")
            with open(cpp, "w") as fh:
                fh.write(src + open(os.path.join(EMU, "lyap_driver.inc")).read())
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-gnu-unique", "-Wno-unknown-pragmas", "-Wno-attributes",
                                   "-include", os.path.join(EMU, "hip_shim.hpp"), "-I" + os.path.join(ROOT, "hamilton_amd", "csrc"),
                                   "-o", so, cpp])
            cache[key] = ctypes.CDLL(so)
        return cache[key]
    return make


def emu_steps(L, q, p, wq, wp, dt, nintervals, every, d0, logsum=None, status=True):
    """hamk_lyap_steps_k on the host, on copies -> (q, p, wq, wp, logsum, status)."""
    q, p, wq, wp = (np.ascontiguousarray(a, dtype=np.float64).copy() for a in (q, p, wq, wp))
    nb = q.shape[1]
    ls = np.zeros(nb) if logsum is None else np.array(logsum, dtype=np.float64)
    st = np.full(nb, -1, np.int32) if status else None
    L.emu_lyap(P(q), P(p), P(wq), P(wp), LL(nb), F(dt), int(nintervals), int(every), F(d0), P(ls), I(st))
    return q, p, wq, wp, ls, st


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------- 1. ABI
def test_entry_points_are_declared_exported_and_bound(hamk_lib):
    from hamilton_amd import _abi, api
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hamk.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "hamilton_amd", "libhamk.so")], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in exported and name in _abi.SIGNATURES and hasattr(hamk_lib, name), name
    assert len(_abi.SIGNATURES["hamk_lyapunov_steps"][1]) == 13
    assert callable(api.lyapunovSteps) and isinstance(api.System.lyapunov_source, property) and isinstance(api.System.lyapunov_build_info, property)
    hpp = open(os.path.join(ROOT, "include", "hamilton.hpp")).read()
    hs = open(os.path.join(ROOT, "bindings", "haskell", "Numeric", "Hamilton", "HIP.hs")).read()
    assert "hamk_lyapunov_steps" in hpp and "lyapunovSteps" in hpp
    assert 'foreign import ccall safe "hamk_lyapunov_steps"' in hs and "lyapunovStepsBatch" in hs


def test_host_signature_equals_the_kernel(hamk_lib):
    """The host states the kernel's parameter list once, in namespace sig_lyap of hamk_host.h (namespace sig keeps its eleven
    entries); launch_lyap builds the argument array from it.  Text only, as tests/test_kernel_signatures.py."""
    device = KS.device_kernels("hamk_lyap.hpp")
    assert list(device) == ["hamk_lyap_steps_k"]
    host_h = KS._text("hamk_host.h")
    body = re.search(r"namespace sig_lyap \{(.*?)\}  // namespace sig_lyap", host_h, re.S).group(1)
    host = {m.group(1): KS._types(m.group(2), named=False) for m in re.finditer(r"using (hamk_\w+_k) = void\(([^)]*)\);", body)}
    assert host == device
    assert device["hamk_lyap_steps_k"] == ["double*", "double*", "double*", "double*", "long long", "double", "int", "int", "double", "double*", "int*"]
    assert len(re.findall(r"using hamk_lyap_steps_k\b", host_h)) == 1 and "hamk_lyap_steps_k" not in KS.host_table()
    dispatch = KS._text("hamk_dispatch.cpp")
    assert "launch_kernel<sig_lyap::hamk_lyap_steps_k>::on(" in dispatch
    for cpp in ("hamk_api.cpp", "hamk_build.cpp", "hamk_dispatch.cpp", "hamk_comm.cpp", "hamk_codegen.cpp"):
        assert "hipModuleLaunchKernel" not in KS._text(cpp), cpp              # launch_kernel (hamk_host.h) stays the only caller


def test_argument_checks(hamk_lib):
    """Every refusal of include/hamk.h, each with its code, before any device is looked at; nothing to do is HAMK_OK."""
    from hamilton_amd import _abi, api
    L = hamk_lib
    s = api.system_from_spec(E.get("pendulum"))
    q, p, wq, wp, ls = np.array([[0.1, 0.2]]), np.array([[0.3, 0.4]]), np.array([[0.6, 0.6]]), np.array([[0.8, 0.8]]), np.array([0.5, 0.25])
    h, a = s._h, [x.ctypes.data for x in (q, p, wq, wp)]
    lp = ls.ctypes.data
    call = lambda *x: L.hamk_lyapunov_steps(*x)
    INV = _abi.HAMK_ERR_INVALID
    assert call(None, 2, *a, 0.01, 1, 1, 1e-7, lp, None, 0) == INV
    for k in range(4):
        b = list(a); b[k] = None
        assert call(h, 2, *b, 0.01, 1, 1, 1e-7, lp, None, 0) == INV, k
    assert call(h, 2, *a, 0.01, 1, 1, 1e-7, None, None, 0) == INV
    assert call(h, -1, *a, 0.01, 1, 1, 1e-7, lp, None, 0) == INV
    assert call(h, 2, *a, 0.01, -1, 1, 1e-7, lp, None, 0) == INV and b"nintervals" in L.hamk_last_error()
    for every in (0, -3):
        assert call(h, 2, *a, 0.01, 1, every, 1e-7, lp, None, 0) == INV and b"every" in L.hamk_last_error()
    assert call(h, 2, *a, 0.01, 1 << 16, 1 << 15, 1e-7, lp, None, 0) == INV and b"int32" in L.hamk_last_error()
    assert call(h, 2, *a, 0.01, 0x7fffffff, 2, 1e-7, lp, None, 0) == INV
    for dt in (float("nan"), float("inf"), -float("inf")):
        assert call(h, 2, *a, dt, 1, 1, 1e-7, lp, None, 0) == INV and b"dt" in L.hamk_last_error()
    for d0 in (float("nan"), float("inf"), 0.0, -1e-7):
        assert call(h, 2, *a, 0.01, 1, 1, d0, lp, None, 0) == INV and b"d0" in L.hamk_last_error()
    assert call(h, 2, *a, 0.01, 1, 1, 1e-7, lp, None, 7) == INV                           # mem
    # nothing to do: HAMK_OK with nothing launched (no GPU is needed for that) and nothing written
    before = [x.copy() for x in (q, p, wq, wp, ls)]
    st = np.full(2, -5, np.int32)
    assert call(h, 0, *a, 0.01, 5, 2, 1e-7, lp, st.ctypes.data, 0) == _abi.HAMK_OK
    assert call(h, 2, *a, 0.01, 0, 2, 1e-7, lp, st.ctypes.data, 0) == _abi.HAMK_OK
    assert call(h, 2, *a, -0.01, 0, 1, 1e-3, lp, None, 1) == _abi.HAMK_OK
    assert same(before, (q, p, wq, wp, ls)) and np.array_equal(st, [-5, -5])
    # ... and through the binding: the state back unchanged, w = 1 / sqrt(2n), logsum = 0, status 0
    ph, w, lsum = api.lyapunovSteps(0.01, 0, 3, s, api.Phase(q, p))
    assert np.array_equal(ph.positions, q) and np.array_equal(ph.momenta, p) and not lsum.any() and lsum.shape == (2,)
    assert np.array_equal(w.positions, np.full((1, 2), 1 / np.sqrt(2.0))) and np.array_equal(w.momenta, w.positions)
    assert not np.asarray(s.last_status).any()
    ph, w, lsum = api.lyapunovSteps(0.01, 0, 3, s, api.Phase(q, p), w=api.Phase(wq, wp), logsum=ls)
    assert np.array_equal(w.positions, wq) and np.array_equal(w.momenta, wp) and np.array_equal(lsum, ls)
    if L.hamk_device_count() == 0:                                                        # no CPU fall-back: a real call needs the GPU
        with pytest.raises(api.HamkError):
            api.lyapunovSteps(0.01, 1, 1, s, api.Phase(q, p))


def test_unsupported_handles_name_the_limit(hamk_lib):
    """One trajectory per lane: n <= 16, and no handle whose options state another mapping."""
    from hamilton_amd import _abi, api
    z = np.zeros((20, 2))
    ls = np.zeros(2)
    big = api.system_from_spec(E.get("chain20"))
    wave = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_WAVE})
    quad = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_QUAD})
    for s, word in ((big, "n <= 16"), (wave, "HAMK_MAP_WAVE"), (quad, "HAMK_MAP_QUAD")):
        rc = hamk_lib.hamk_lyapunov_steps(s._h, 2, z.ctypes.data, z.ctypes.data, z.ctypes.data, z.ctypes.data, 0.01, 1, 1, 1e-7, ls.ctypes.data, None, 0)
        msg = hamk_lib.hamk_last_error().decode()
        assert rc == _abi.HAMK_ERR_UNSUPPORTED and word in msg and "n <= 16" in msg and "Lyapunov" in msg, (rc, msg)
        assert hamk_lib.hamk_lyapunov_source(s._h) is None and hamk_lib.hamk_lyapunov_build_info(s._h) is None
        with pytest.raises(api.HamkError, match="n <= 16") as e:
            s.lyapunov_source
        assert e.value.code == _abi.HAMK_ERR_UNSUPPORTED
    assert hamk_lib.hamk_lyapunov_source(None) is None and hamk_lib.hamk_lyapunov_build_info(None) is None
    lane = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_LANE})          # the lane mapping stated: fine
    assert "HAMK_INSTANTIATE_LYAP(HamkSys)" in lane.lyapunov_source


# ---------------------------------------------------------------------------------------------------------------------- 2. build
@pytest.mark.parametrize("name", SYSTEMS)
def test_companion_module_compiles_for_gfx950(hamk_lib, name):
    """The kernel lives in a module of its own: the per-system module keeps its nine function symbols, its nine build_info rows and
    its source; the symplectic companion is what it was; the Lyapunov companion is the source with the final instantiation replaced."""
    from hamilton_amd import api
    s = api.system_from_spec(E.get(name))
    src, info, symp = s.source, s.build_info, s.symplectic_source
    line = s.lyapunov_build_info
    assert line.count("\n") == 1 and line.endswith("\n")
    m = re.fullmatch(r"hamk_lyap_steps_k build=default bytes=(\d+) sgpr_spills=(-?\d+) vgpr_spills=(-?\d+) vgprs=(\d+) functions=(\d+)\n", line)
    assert m, line
    nbytes, _, vspill, vgprs, nfunc = (int(x) for x in m.groups())
    assert nfunc == 1, (name, nfunc)                          # every device function inlined into the one kernel
    assert 0 < nbytes < 100 * 1024, (name, nbytes)
    assert 0 < vgprs <= 512 and vspill >= 0
    assert s.num_device_functions == 9 and s.build_info == info and len(info.splitlines()) == 9 and s.source == src
    assert s.symplectic_source == symp and symp == src[:src.rindex("HAMK_INSTANTIATE(HamkSys)")] + '#include "hamk_symp.hpp"\nHAMK_INSTANTIATE_SYMP(HamkSys)\n'
    assert api.system_from_spec(E.get(name)).symplectic_source == symp                      # ... and without the Lyapunov companion built
    assert s.lyapunov_source == src[:src.rindex("HAMK_INSTANTIATE(HamkSys)")] + '#include "hamk_lyap.hpp"\nHAMK_INSTANTIATE_LYAP(HamkSys)\n'
    assert s.kernel_bytes("hamk_lyap_steps_k") == 0                                         # not a kernel of the per-system module
    assert s.lyapunov_build_info == line                                                    # built once


def test_auto_mapping_keeps_the_stepper_on_the_lane_module(hamk_lib):
    """chain12: AUTO serves small RK4 ensembles on the four-lane kernels; the Lyapunov module is the lane module's companion."""
    from hamilton_amd import _abi, api
    s = api.system_from_spec(E.get("chain12"))
    assert s.options(8192)["mapping"] == _abi.MAP_QUAD
    s.describe_batch(8192)
    comp = s.lyapunov_source
    assert '#include "hamk_device.hpp"' in comp and "hamk_quad.hpp" not in comp and comp.endswith("HAMK_INSTANTIATE_LYAP(HamkSys)\n")


# ---------------------------------------------------------------------------------------------------------------------- 3. anchors
@pytest.mark.parametrize("case", ANCHOR_CASES, ids=lambda c: "dt%g-every%d-n%d-d0%g" % c)
@pytest.mark.parametrize("start", ["zero", "random"])
@pytest.mark.parametrize("kind", ANCHOR_KINDS)
def test_analytic_anchors(emulate, oracle_lib, kind, start, case):
    """logsum against the closed form: the restatement first, then the kernel."""
    dt, every, nint, d0 = case
    o = oracle_lib.OracleSystem(anchor_spec(kind))
    q, p, wq, wp = anchor_inputs(kind, start)
    check_anchor(kind, case, restate(o, q, p, wq, wp, dt, nint, every, d0, np.zeros(ANCHOR_B)), "restatement")
    check_anchor(kind, case, emu_steps(emulate(anchor_system(kind)), q, p, wq, wp, dt, nint, every, d0), "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 4. values
@pytest.mark.parametrize("d0", D0S)
@pytest.mark.parametrize("name", SYSTEMS)
def test_kernel_on_host_matches_the_restatement(emulate, oracle_lib, name, d0):
    from hamilton_amd import api
    ref = reference(oracle_lib, name, d0)
    got = emu_steps(emulate(api.system_from_spec(E.get(name))), ref["q"], ref["p"], ref["wq"], ref["wp"], DT, NINT, EVERY, d0)
    check_against_reference(ref, name, got, "kernel on host")


# ---------------------------------------------------------------------------------------------------------------------- 5. bits
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_cut_invariance_and_independence_from_the_shadow(emulate, oracle_lib, name):
    """4 intervals in one call equal 2 + 2 with w and logsum carried, bitwise on all five outputs (status: the OR); q, p are
    bitwise independent of w and d0 (another unit w, another d0, a w that is no unit vector)."""
    from hamilton_amd import api
    ref = reference(oracle_lib, name, 1e-6)
    L = emulate(api.system_from_spec(E.get(name)))
    q, p, wq, wp = ref["q"], ref["p"], ref["wq"], ref["wp"]
    start = np.linspace(-1.0, 1.0, B)                       # a logsum that is not zero at entry
    one = emu_steps(L, q, p, wq, wp, DT, 4, EVERY, 1e-6, start)
    h1 = emu_steps(L, q, p, wq, wp, DT, 2, EVERY, 1e-6, start)
    h2 = emu_steps(L, *h1[:4], DT, 2, EVERY, 1e-6, h1[4])
    assert same(one[:5], h2[:5]) and np.array_equal(one[5], h1[5] | h2[5])
    assert not np.array_equal(one[4], start)
    w2q, w2p = unit_w(q.shape[0], B, 99)
    for other in (emu_steps(L, q, p, w2q, w2p, DT, 4, EVERY, 1e-6), emu_steps(L, q, p, wq, wp, DT, 4, EVERY, 1e-3),
                  emu_steps(L, q, p, 3.0 * w2q, -2.0 * w2p, DT, 4, EVERY, 1e-9)):
        assert np.array_equal(other[0], one[0]) and np.array_equal(other[1], one[1])
        assert not np.array_equal(other[2], one[2])


def test_status_and_null_status_on_host(emulate, oracle_lib):
    """A NaN lane among healthy ones ends flagged HAMK_ST_NONFINITE, its neighbours' bits are those of a run without it; a w of zero
    (d = 0: log 0) is flagged the same way; status may be null."""
    from hamilton_amd import api
    ref = reference(oracle_lib, "doublePendulum", 1e-6)
    L = emulate(api.system_from_spec(E.get("doublePendulum")))
    q, p, wq, wp = (ref[k][:, :9] for k in ("q", "p", "wq", "wp"))
    want = emu_steps(L, q, p, wq, wp, DT, 2, EVERY, 1e-6)
    assert not want[5].any()
    q2 = q.copy(); q2[0, 2] = np.nan
    w2 = wq.copy(); w2[:, 5] = 0.0
    got = emu_steps(L, q2, p, w2, np.where(np.arange(9) == 5, 0.0, wp), DT, 2, EVERY, 1e-6)
    keep = (np.arange(9) != 2) & (np.arange(9) != 5)
    assert got[5][2] & 2 and got[5][5] & 2 and not got[5][keep].any()
    assert not np.isfinite(got[4][5]) and np.array_equal(got[0][:, 5], want[0][:, 5]) and np.array_equal(got[1][:, 5], want[1][:, 5])
    assert same([a[..., keep] for a in got[:5]], [a[..., keep] for a in want[:5]])
    assert same(emu_steps(L, q, p, wq, wp, DT, 2, EVERY, 1e-6, status=False)[:5], want[:5])
    one = emu_steps(L, q, p, w2, np.where(np.arange(9) == 5, 0.0, wp), DT, 1, EVERY, 1e-6)          # one interval: the -inf itself
    assert np.isneginf(one[4][5]) and one[5][5] & 2 and np.isnan(one[2][:, 5]).all()
