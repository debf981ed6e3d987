"""CPU: the symplectic fixed-step stepper (hamk_symplectic_steps; hamilton_amd/csrc/hamk_symp.hpp) -- its three entry points and
their argument checks, the companion module that carries its kernel (compiled for gfx950 here: hiprtc needs no GPU), and the kernel
itself run thread by thread on the host (tests/host_emulation/symp_driver.inc, compiled from System.symplectic_source with the flags
of test_host_emulation.py's `emulate`) against a literal numpy restatement of the scheme over the oracle's hamEqs
(below) -- values, and the properties that a wrong scheme that still "matches itself" would lose: order,
time-reversibility, symplecticity, no secular energy growth.  What this cannot see is the GPU compiler (tests/test_gpu_symplectic.py)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from hamilton_amd import examples as E

EMU = os.path.join(ROOT, "tests", "host_emulation")
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
P = lambda a: a.ctypes.data_as(_dp)
I = lambda a: a.ctypes.data_as(_ip)
LL = ctypes.c_longlong
F = ctypes.c_double


# ---------------------------------------------------------------------------------------------------------------------- reference
# A LITERAL numpy restatement of the scheme of hamilton_amd/csrc/hamk_symp.hpp over the oracle's hamEqs (the oracle itself is not
# changed); tests/test_gpu_symplectic.py imports it, and the stencil, from this module.
#   one substep of size h from y = [q; p]:   z^0 = y;  z^{k+1} = y + (h/2) f(z^k), k = 0 .. iters-1;  y <- 2 z^{iters} - y
#   order 2: one substep of dt per step.  order 4: substeps g1 dt, g2 dt, g1 dt, g1 = 1 / (2 - 2^(1/3)), g2 = 1 - 2 g1.
#   residual: max over steps, substeps and components j of |z^{iters}_j - z^{iters-1}_j| / max(1, |y_j|), y the substep's start.
#   status: OR of the status of every hamEqs evaluation (1 = singular K), plus 2 where the FINAL state is not finite.
G1 = 1.0 / (2.0 - 2.0 ** (1.0 / 3.0))
G2 = 1.0 - 2.0 * G1


def substeps(dt, order):
    assert order in (2, 4)
    return [dt] if order == 2 else [G1 * dt, G2 * dt, G1 * dt]


def restate(o, q, p, dt, nsteps, order, iters):
    """-> (q, p, residual[B], status[B]) after nsteps steps; q, p are [n, B]."""
    q, p = np.array(q, dtype=np.float64), np.array(p, dtype=np.float64)
    B = q.shape[1]
    res, st = np.zeros(B), np.zeros(B, np.int32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(nsteps):
            for h in substeps(dt, order):
                hh = 0.5 * h
                zq, zp = q.copy(), p.copy()
                last = np.zeros(B)
                for k in range(iters):
                    dq, dp, s1 = o.hameqs_batch(zq, zp, threads=1)     # (small ensembles, hundreds of calls: no thread team per call)
                    st |= s1
                    nq, npp = q + hh * dq, p + hh * dp
                    if k == iters - 1:
                        last = np.maximum((np.abs(nq - zq) / np.maximum(1.0, np.abs(q))).max(0),
                                          (np.abs(npp - zp) / np.maximum(1.0, np.abs(p))).max(0))
                    zq, zp = nq, npp
                res = np.fmax(res, last)
                q, p = 2.0 * zq - q, 2.0 * zp - p
    st[~(np.isfinite(q).all(0) & np.isfinite(p).all(0))] |= 2
    return q, p, res, st


# ---- symplecticity by finite differences over neighbouring lanes ------------------------------------------------------
# Every base point y = [q; p] (2n numbers) sits in the ensemble with its 2 * 2n central-difference neighbours y +- delta e_c: lane
# b * (1 + 4n) is base point b, then for component c the lanes +delta, -delta.  M = d(step map)/dy by central differences;
# a symplectic map has M^T J M = J, J = [[0, I], [-I, 0]].
DELTA = 1e-4


def stencil(q0, p0, delta=DELTA):
    """q0, p0: [n, nb] base points -> q, p: [n, nb * (1 + 4n)]."""
    n, nb = q0.shape
    y0 = np.concatenate([q0, p0], axis=0)
    cols = []
    for b in range(nb):
        cols.append(y0[:, b].copy())
        for c in range(2 * n):
            for sgn in (1.0, -1.0):
                y = y0[:, b].copy()
                y[c] += sgn * delta
                cols.append(y)
    y = np.stack(cols, axis=1)
    return np.ascontiguousarray(y[:n]), np.ascontiguousarray(y[n:])


def symplectic_defect(q1, p1, n, nb, delta=DELTA):
    """max over base points of ||M^T J M - J||_max from the stepped stencil."""
    y1 = np.concatenate([q1, p1], axis=0)
    J = np.block([[np.zeros((n, n)), np.eye(n)], [-np.eye(n), np.zeros((n, n))]])
    worst = 0.0
    for b in range(nb):
        at = b * (1 + 4 * n)
        M = np.stack([(y1[:, at + 1 + 2 * c] - y1[:, at + 2 + 2 * c]) / (2.0 * delta) for c in range(2 * n)], axis=1)
        worst = max(worst, float(np.abs(M.T @ J @ M - J).max()))
    return worst


# base points of the stencil tests: regular motion, well inside the systems' sampling boxes
STENCIL = {
    "pendulum": dict(dt=0.5, q0=np.array([[-2.0, -1.2, -0.6, -0.2, 0.3, 0.8, 1.5, 2.2]]),
                     p0=np.array([[0.4, -0.7, 0.9, -0.2, 0.6, -1.0, 0.3, -0.5]])),
    "doublePendulum": dict(dt=0.1, q0=np.array([[0.4, -0.9, 1.3, -0.3], [-0.6, 0.5, 0.2, 1.1]]),
                           p0=np.array([[0.3, -0.5, 0.2, 0.8], [-0.2, 0.4, -0.6, 0.1]])),
}
STENCIL_ITERS = {2: 32, 4: 48}                               # residual < 1e-14 at those steps (test_step_map_is_symplectic checks it on the restatement)


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))))


@pytest.fixture(scope="module")
def emulate(hamk_lib, tmp_path_factory):
    """(System, which) -> the kernels of `which` source ("symp": the companion module, "lane": the per-system module) on the host."""
    cache = {}
    tmp = tmp_path_factory.mktemp("symp_emu")

    def make(s, which="symp"):
        src, driver = (s.symplectic_source, "symp_driver.inc") if which == "symp" else (s.source, "driver.inc")
        key = hashlib.sha1((which + src).encode()).hexdigest()[:16]
        if key not in cache:
            cpp, so = str(tmp / f"{key}.cpp"), str(tmp / f"{key}.so")
            with open(cpp, "w") as fh:
                fh.write(src + open(os.path.join(EMU, driver)).read())
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-gnu-unique", "-Wno-unknown-pragmas", "-Wno-attributes",
                                   "-include", os.path.join(EMU, "hip_shim.hpp"), "-I" + os.path.join(ROOT, "hamilton_amd", "csrc"),
                                   "-o", so, cpp])
            cache[key] = ctypes.CDLL(so)
        return cache[key]
    return make


def emu_steps(L, q, p, dt, nsteps, order, iters):
    """hamk_symp_steps_k on the host with the arguments hamk_symplectic_steps passes it -> (q, p, residual, status)."""
    q, p = np.ascontiguousarray(q, dtype=np.float64).copy(), np.ascontiguousarray(p, dtype=np.float64).copy()
    B = q.shape[1]
    res, st = np.full(B, -1.0), np.full(B, -1, np.int32)
    hs = substeps(dt, order)
    L.emu_symp(P(q), P(p), LL(B), int(nsteps), len(hs), F(hs[0]), F(hs[1] if order == 4 else 0.0), int(iters), P(res), I(st))
    return q, p, res, st


# ---------------------------------------------------------------------------------------------------------------------- 1. ABI
def test_entry_points_are_declared_exported_and_bound(hamk_lib):
    from hamilton_amd import _abi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hamk.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "hamilton_amd", "libhamk.so")], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for name in ("hamk_symplectic_steps", "hamk_symplectic_source", "hamk_symplectic_build_info"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in exported and name in _abi.SIGNATURES and hasattr(hamk_lib, name), name
    assert len(_abi.SIGNATURES["hamk_symplectic_steps"][1]) == 11
    from hamilton_amd import api
    assert callable(api.symplecticSteps)
    for text in (open(os.path.join(ROOT, "include", "hamilton.hpp")).read(), open(os.path.join(ROOT, "bindings", "haskell", "Numeric", "Hamilton", "HIP.hs")).read()):
        assert "hamk_symplectic_steps" in text


def test_argument_checks(hamk_lib):
    """Every refusal of include/hamk.h, each with its code, before any device is looked at; nothing to do is HAMK_OK."""
    from hamilton_amd import _abi, api
    L = hamk_lib
    s = api.system_from_spec(E.get("pendulum"))
    q, p = np.array([[0.1, 0.2]]), np.array([[0.3, 0.4]])
    h, qp, pp = s._h, q.ctypes.data, p.ctypes.data
    call = lambda *a: L.hamk_symplectic_steps(*a)
    INV = _abi.HAMK_ERR_INVALID
    assert call(None, 2, qp, pp, 0.01, 1, 2, 4, None, None, 0) == INV
    assert call(h, 2, None, pp, 0.01, 1, 2, 4, None, None, 0) == INV
    assert call(h, 2, qp, None, 0.01, 1, 2, 4, None, None, 0) == INV
    assert call(h, -1, qp, pp, 0.01, 1, 2, 4, None, None, 0) == INV
    assert call(h, 2, qp, pp, 0.01, -1, 2, 4, None, None, 0) == INV
    for order in (0, 1, 3, 5, -2):
        assert call(h, 2, qp, pp, 0.01, 1, order, 4, None, None, 0) == INV and b"order" in L.hamk_last_error()
    for iters in (-1, 65, 1000):
        assert call(h, 2, qp, pp, 0.01, 1, 2, iters, None, None, 0) == INV and b"iters" in L.hamk_last_error()
    for dt in (float("nan"), float("inf"), -float("inf")):
        assert call(h, 2, qp, pp, dt, 1, 4, 4, None, None, 0) == INV and b"dt" in L.hamk_last_error()
    assert call(h, 2, qp, pp, 0.01, 1, 2, 4, None, None, 7) == INV                       # mem
    # nothing to do: HAMK_OK with nothing launched (no GPU is needed for that), the state untouched
    before = (q.copy(), p.copy())
    assert call(h, 0, qp, pp, 0.01, 5, 2, 4, None, None, 0) == _abi.HAMK_OK
    assert call(h, 2, qp, pp, 0.01, 0, 4, 0, None, None, 0) == _abi.HAMK_OK
    assert call(h, 2, qp, pp, -0.01, 0, 4, 64, None, None, 1) == _abi.HAMK_OK
    assert np.array_equal(q, before[0]) and np.array_equal(p, before[1])
    if L.hamk_device_count() == 0:                                                       # no CPU fall-back: a real call needs the GPU
        with pytest.raises(api.HamkError):
            api.symplecticSteps(0.01, 1, s, api.Phase(q, p))


@pytest.mark.parametrize("order", [2, 4])
def test_nothing_to_do_through_the_python_binding(hamk_lib, order):
    """nsteps = 0 (and an empty ensemble) is HAMK_OK with nothing launched and nothing written -- no GPU needed: the binding hands
    back the state unchanged, status 0 and residual 0, for one reference-shaped trajectory and for a batch, every time."""
    from hamilton_amd import api
    s = api.system_from_spec(E.get("doublePendulum"))
    for _ in range(3):                                       # (fresh output arrays each call: whatever the allocator hands out)
        q1, p1 = np.array([0.3, -0.2]), np.array([0.1, 0.4])
        ph, res = api.symplecticSteps(0.01, 0, s, api.Phase(q1, p1), order=order, iters=5, with_residual=True)
        assert np.array_equal(ph.positions, q1) and np.array_equal(ph.momenta, p1) and ph.positions.shape == (2,)
        assert res == 0.0 and np.array_equal(np.asarray(s.last_status), [0])
        q, p = np.arange(14.0).reshape(2, 7) / 10, np.arange(14.0).reshape(2, 7) / 7
        ph, res = api.symplecticSteps(0.01, 0, s, api.Phase(q, p), order=order, with_residual=True)
        assert np.array_equal(ph.positions, q) and np.array_equal(ph.momenta, p)
        assert res.shape == (7,) and not res.any() and np.asarray(s.last_status).shape == (7,) and not np.asarray(s.last_status).any()
        assert api.symplecticSteps(0.01, 0, s, api.Phase(q, p), order=order).positions.shape == (2, 7)
        e = np.empty((2, 0))
        ph, res = api.symplecticSteps(0.01, 3, s, api.Phase(e, e), order=order, with_residual=True)
        assert ph.positions.shape == (2, 0) and res.shape == (0,)


def test_unsupported_handles_name_the_limit(hamk_lib):
    """One trajectory per lane: n <= 16, and no handle whose options state another mapping."""
    from hamilton_amd import _abi, api
    q, p = np.zeros((17, 2)), np.zeros((17, 2))
    big = api.system_from_spec(E.chain(17))
    wave = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_WAVE})
    quad = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_QUAD})
    for s, word in ((big, "n <= 16"), (wave, "HAMK_MAP_WAVE"), (quad, "HAMK_MAP_QUAD")):
        rc = hamk_lib.hamk_symplectic_steps(s._h, 2, q.ctypes.data, p.ctypes.data, 0.01, 1, 2, 4, None, None, 0)
        msg = hamk_lib.hamk_last_error().decode()
        assert rc == _abi.HAMK_ERR_UNSUPPORTED and word in msg and "n <= 16" in msg, (rc, msg)
        assert hamk_lib.hamk_symplectic_source(s._h) is None and hamk_lib.hamk_symplectic_build_info(s._h) is None
        with pytest.raises(api.HamkError, match="n <= 16") as e:
            s.symplectic_source
        assert e.value.code == _abi.HAMK_ERR_UNSUPPORTED
    assert hamk_lib.hamk_symplectic_source(None) is None
    lane = api.system_from_spec(E.get("chain8"), {"mapping": _abi.MAP_LANE})          # the lane mapping stated: fine
    assert "HAMK_INSTANTIATE_SYMP(HamkSys)" in lane.symplectic_source


# ---------------------------------------------------------------------------------------------------------------------- 2. build
@pytest.mark.parametrize("name", ["pendulum", "doublePendulum", "opcodeZoo", "chain8", "chain16"])
def test_companion_module_compiles_for_gfx950(hamk_lib, name):
    """The kernel lives in a module of its own: the per-system module keeps its nine function symbols, its nine build_info rows and
    its source, byte for byte; the companion is that source with the final instantiation replaced."""
    from hamilton_amd import api
    s = api.system_from_spec(E.get(name))
    src, info, rows = s.source, s.build_info, s.num_device_functions
    line = s.symplectic_build_info
    assert line.count("\n") == 1 and line.endswith("\n")
    m = re.fullmatch(r"hamk_symp_steps_k build=default bytes=(\d+) sgpr_spills=(-?\d+) vgpr_spills=(-?\d+) vgprs=(\d+) functions=(\d+)\n", line)
    assert m, line
    nbytes, _, vspill, vgprs, nfunc = (int(x) for x in m.groups())
    # every device function inlined into the one kernel: what the nine-symbol rule guards in the per-system modules
    assert nfunc == 1, (name, nfunc)
    assert 0 < nbytes < 100 * 1024, (name, nbytes)
    assert 0 < vgprs <= 512 and vspill >= 0
    assert s.num_device_functions == rows == 9 and s.build_info == info and len(info.splitlines()) == 9
    assert s.source == src
    comp = s.symplectic_source
    assert src.endswith("HAMK_INSTANTIATE(HamkSys)\n") and "HAMK_INSTANTIATE_SYMP" not in src
    head = src[:src.rindex("HAMK_INSTANTIATE(HamkSys)")]
    assert comp == head + '#include "hamk_symp.hpp"\nHAMK_INSTANTIATE_SYMP(HamkSys)\n'
    assert s.kernel_bytes("hamk_symp_steps_k") == 0                                       # not a kernel of the per-system module
    assert s.symplectic_build_info == line                                                # built once


def test_auto_mapping_keeps_the_stepper_on_the_lane_module(hamk_lib):
    """chain12: AUTO serves small RK4 ensembles on the four-lane kernels; the symplectic stepper's module is the lane module's
    companion whichever specialisation the handle is describing."""
    from hamilton_amd import _abi, api
    s = api.system_from_spec(E.get("chain12"))
    assert s.options(8192)["mapping"] == _abi.MAP_QUAD
    s.describe_batch(8192)
    assert "hamk_quad.hpp" in s.source
    comp = s.symplectic_source
    assert '#include "hamk_device.hpp"' in comp and "hamk_quad.hpp" not in comp and comp.endswith("HAMK_INSTANTIATE_SYMP(HamkSys)\n")


# ---------------------------------------------------------------------------------------------------------------------- 3. values
def make_system(name, monkeypatch):
    """name, or name@jets: the jets instead of the symbolic right-hand side (HAMK_K_SYMBOLIC=0 under HAMK_TEST_OVERRIDES=1)."""
    from hamilton_amd import api
    base, _, variant = name.partition("@")
    if variant == "jets":
        monkeypatch.setenv("HAMK_K_SYMBOLIC", "0")
    spec = E.get(base)
    s = api.system_from_spec(spec)
    if base == "doublePendulum":
        assert ("HAS_SYM_K = true" in s.source) == (variant != "jets")
    return spec, s


def sample_phase(spec, o, start, B):
    q, qd = E.sample_config(spec, start, B)
    if spec.name.startswith("chain") or "~mixed" in spec.name:             # (the chains' sampling box has qd = 0)
        qd = qd + 0.4 * np.cos(1.0 + np.arange(spec.n * B, dtype=np.float64).reshape(spec.n, B))
    return q, o.to_phase_batch(q, qd)


VALUE_SYSTEMS = ["pendulum", "doublePendulum", "doublePendulum@jets", "opcodeZoo", "room", "chain8", "doublePendulum~mixed"]


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", VALUE_SYSTEMS)
def test_kernel_on_host_matches_the_restatement(emulate, oracle_lib, monkeypatch, name, order):
    """B = 5, 10 steps of 0.01, 6 iterations.  State: the bound test_fixed_step_loop_over_many_steps_on_host applies to RK4 --
    2e-11 absolute on the calm lanes, most lanes calm; status words equal; residual to a factor of 2 (it is a difference of nearly
    equal numbers: the two evaluation orders round it differently)."""
    spec, s = make_system(name, monkeypatch)
    o = oracle_lib.OracleSystem(spec)
    B = 5
    q, p = sample_phase(spec, o, 17, B)
    rq, rp, rres, rst = restate(o, q, p, 0.01, 10, order, 6)
    L = emulate(s)
    gq, gp, gres, gst = emu_steps(L, q, p, 0.01, 10, order, 6)
    err = np.maximum(np.abs(gq - rq).max(0), np.abs(gp - rp).max(0))
    calm = np.abs(rp).max(0) < 50
    print(name, order, "state err", float(err[calm].max()), "residual kernel", gres, "restatement", rres)
    assert np.array_equal(gst, rst), (gst, rst)
    assert calm.mean() > 0.8 and float(err[calm].max()) < 2e-11, (name, order, float(err[calm].max()))
    assert np.all(gres <= 2 * rres) and np.all(rres <= 2 * gres), (gres, rres)


def test_status_and_null_outputs_on_host(emulate, oracle_lib):
    """A NaN lane: costs what the others cost, ends flagged HAMK_ST_NONFINITE, its neighbours' bits are those of a run without it;
    residual and status may be null."""
    from hamilton_amd import api
    spec = E.get("doublePendulum")
    s, o = api.system_from_spec(spec), oracle_lib.OracleSystem(spec)
    L = emulate(s)
    q, p = sample_phase(spec, o, 3, 6)
    want = emu_steps(L, q, p, 0.01, 5, 4, 5)
    q2 = q.copy(); q2[0, 2] = np.nan
    got = emu_steps(L, q2, p, 0.01, 5, 4, 5)
    keep = np.arange(6) != 2
    assert got[3][2] & 2 and not got[3][keep].any() and not want[3].any()
    assert np.array_equal(got[0][:, keep], want[0][:, keep]) and np.array_equal(got[1][:, keep], want[1][:, keep])
    a, b = q.copy(), p.copy()
    L.emu_symp(P(a), P(b), LL(6), 5, 3, F(G1 * 0.01), F(G2 * 0.01), 5, None, None)
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1])


# ---------------------------------------------------------------------------------------------------------------------- 4. properties
# amplitudes at which the motion is regular (the double pendulum: small swings); dt per order such that both errors are far above
# the reference solution's own (evolve_ham at eps = 1e-13: ~1e-12) and the observed order is in its asymptotic range
ORDER_CASES = {
    "pendulum": dict(q0=STENCIL["pendulum"]["q0"], p0=STENCIL["pendulum"]["p0"], dt={2: 0.02, 4: 0.1}),
    "doublePendulum": dict(q0=np.array([[0.3, -0.2, 0.25, 0.1], [-0.2, 0.3, 0.15, -0.25]]),
                           p0=np.array([[0.1, -0.15, 0.05, 0.2], [-0.05, 0.1, -0.1, 0.05]]), dt={2: 0.02, 4: 0.05}),
}


@pytest.fixture(scope="module")
def truth_at_one(oracle_lib):
    """The state at t = 1 by the oracle's adaptive stepper at eps = 1e-13, once per system."""
    out = {}
    for name, c in ORDER_CASES.items():
        o = oracle_lib.OracleSystem(E.get(name))
        rows = [o.evolve_ham(c["q0"][:, i], c["p0"][:, i], [0.0, 1.0], eps_abs=1e-13, eps_rel=1e-13) for i in range(c["q0"].shape[1])]
        out[name] = (np.stack([r[0][1] for r in rows], 1), np.stack([r[1][1] for r in rows], 1))
    return out


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", ["pendulum", "doublePendulum"])
def test_observed_order(emulate, oracle_lib, truth_at_one, name, order):
    """Error at t = 1 for dt and dt / 2, per trajectory: log2 of the ratio within 0.15 of the order.  40 iterations: residual
    < 1e-14, i.e. the implicit equations are solved.  The restatement has to meet every condition before the kernel is asked to."""
    from hamilton_amd import api
    spec, c = E.get(name), ORDER_CASES[name]
    o, s = oracle_lib.OracleSystem(spec), api.system_from_spec(spec)
    L = emulate(s)
    tq, tp = truth_at_one[name]
    dt = c["dt"][order]

    def observed(step):
        es = []
        for d in (dt, dt / 2):
            n = int(round(1.0 / d))
            assert abs(n * d - 1.0) < 1e-12
            q1, p1, res, st = step(c["q0"], c["p0"], d, n)
            assert res.max() < 1e-14 and not st.any()
            es.append(np.maximum(np.abs(q1 - tq).max(0), np.abs(p1 - tp).max(0)))
        assert es[0].min() > 1e-9 and es[1].min() > 1e-9, es
        return np.log2(es[0] / es[1])
    ref = observed(lambda q, p, d, n: restate(o, q, p, d, n, order, 40))
    assert np.all(np.abs(ref - order) < 0.15), ("the restatement itself", ref)
    got = observed(lambda q, p, d, n: emu_steps(L, q, p, d, n, order, 40))
    print(name, order, "observed order: restatement", ref, "kernel", got)
    assert np.all(np.abs(got - order) < 0.15), got


REVERSE_CASES = [("pendulum", 0.05), ("doublePendulum", 0.02)]


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name,dt", REVERSE_CASES)
def test_time_reversibility(emulate, oracle_lib, name, dt, order):
    """100 steps of dt, then 100 of -dt: back at the start to within 10 x the restatement's own return distance + 1e-13 (the factor
    allows for the different rounding order).  24 iterations: the substeps are solved to roundoff (residual checked)."""
    from hamilton_amd import api
    spec, c = E.get(name), ORDER_CASES[name]
    o, s = oracle_lib.OracleSystem(spec), api.system_from_spec(spec)
    L = emulate(s)

    def there_and_back(step):
        q1, p1, res1, _ = step(c["q0"], c["p0"], dt)
        q2, p2, res2, _ = step(q1, p1, -dt)
        assert max(res1.max(), res2.max()) < 1e-14
        assert max(np.abs(q1 - c["q0"]).max(), np.abs(p1 - c["p0"]).max()) > 0.1            # (it did go somewhere)
        return max(np.abs(q2 - c["q0"]).max(), np.abs(p2 - c["p0"]).max())
    ref = there_and_back(lambda q, p, h: restate(o, q, p, h, 100, order, 24))
    got = there_and_back(lambda q, p, h: emu_steps(L, q, p, h, 100, order, 24))
    print(name, order, "return distance: restatement", ref, "kernel", got)
    assert ref < 1e-11, ref
    assert got <= 10 * ref + 1e-13, (got, ref)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", ["pendulum", "doublePendulum"])
def test_step_map_is_symplectic(emulate, oracle_lib, name, order):
    """One large step (pendulum 0.5, doublePendulum 0.1) of every base point and its 2 * 2n central-difference neighbours at
    delta = 1e-4: the finite-difference Jacobian M of the step map has ||M^T J M - J||_max <= 1e-6 (truncation O(delta^2) = 1e-8
    and roundoff eps / delta = 1e-12 are both far below).  Control: the same stencil through the RK4 kernel gives > 1e-5 for the
    pendulum -- the test can tell the two apart."""
    from hamilton_amd import api
    spec, c = E.get(name), STENCIL[name]
    o, s = oracle_lib.OracleSystem(spec), api.system_from_spec(spec)
    nb = c["q0"].shape[1]
    assert nb == (8 if name == "pendulum" else 4)
    q, p = stencil(c["q0"], c["p0"])
    assert q.shape[1] == nb * (1 + 4 * spec.n)
    iters = STENCIL_ITERS[order]
    rq, rp, rres, rst = restate(o, q, p, c["dt"], 1, order, iters)
    ref = symplectic_defect(rq, rp, spec.n, nb)
    assert rres.max() < 1e-14 and not rst.any() and ref <= 1e-6, (rres.max(), ref)
    gq, gp, gres, gst = emu_steps(emulate(s), q, p, c["dt"], 1, order, iters)
    got = symplectic_defect(gq, gp, spec.n, nb)
    print(name, order, "defect: restatement", ref, "kernel", got)
    assert not gst.any() and got <= 1e-6, got
    if name == "pendulum":
        Lr = emulate(s, "lane")
        kq, kp, st = q.copy(), p.copy(), np.zeros(q.shape[1], np.int32)
        Lr.emu_rk4(P(kq), P(kp), LL(q.shape[1]), F(c["dt"]), 1, I(st))
        rk4 = symplectic_defect(kq, kp, spec.n, nb)
        print("RK4 kernel, same stencil:", rk4)
        assert rk4 > 1e-5, rk4


def test_no_secular_energy_growth(emulate, oracle_lib):
    """pendulum, dt = 0.05, 20 000 steps in 20 launches of 1000, H from the oracle after each launch: the energy error of the second
    half of the run is no larger than twice that of the first half (a symplectic method's error oscillates; RK4's grows)."""
    from hamilton_amd import api
    spec, c = E.get("pendulum"), STENCIL["pendulum"]
    o, s = oracle_lib.OracleSystem(spec), api.system_from_spec(spec)
    L = emulate(s)
    q, p = c["q0"].copy(), c["p0"].copy()
    H0 = o.observe_batch(q, p)[2]
    dev = []
    for _ in range(20):
        q, p, res, st = emu_steps(L, q, p, 0.05, 1000, 2, 16)
        assert not st.any() and res.max() < 1e-14
        dev.append(np.abs(o.observe_batch(q, p)[2] - H0))
    dev = np.array(dev)
    first, second = dev[:10].max(0), dev[10:].max(0)
    print("max |H - H0| launches 1-10", first, "11-20", second)
    assert np.all(second <= 2 * first), (first, second)
