"""GPU: hamk_symplectic_steps through the C ABI of libhamk.so -- the companion module's kernel as the GPU compiler built it --
against the numpy restatement of the scheme over the oracle's hamEqs (tests/test_symplectic.py), plus what only the real launch can
show: bit-reproducibility, independence of B and of how a run is cut into calls, the symplecticity stencil on the device's own
arithmetic, the residual, a singular lane among healthy ones.  B = 257: two blocks, the second holding one lane."""
import ctypes

import numpy as np
import pytest

import test_symplectic as R                  # the numpy restatement of the scheme and the stencil live in the CPU test module
from hamilton_amd import examples as E

pytestmark = pytest.mark.gpu

B = 257
HOST, DEVICE = 0, 1


@pytest.fixture(scope="module")
def lib(hamk_lib):
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return hamk_lib


def steps(lib, s, q, p, dt, nsteps, order, iters, mem=HOST, residual=True, status=True):
    """One hamk_symplectic_steps call on copies of q, p ([n, B] host arrays) -> (q, p, residual, status); mem = DEVICE goes through
    hamk_device_malloc'ed arrays and is synchronised before the copy back."""
    from hamilton_amd import _abi
    q, p = np.ascontiguousarray(q, dtype=np.float64).copy(), np.ascontiguousarray(p, dtype=np.float64).copy()
    nb = q.shape[1]
    res = np.full(nb, -1.0) if residual else None
    st = np.full(nb, -1, np.int32) if status else None
    ptr = lambda a: None if a is None else a.ctypes.data
    if mem == HOST:
        _abi.check(lib.hamk_symplectic_steps(s._h, nb, ptr(q), ptr(p), dt, nsteps, order, iters, ptr(res), ptr(st), HOST))
        return q, p, res, st
    dev = []
    try:
        for a in (q, p, res, st):
            d = ctypes.c_void_p()
            if a is not None:
                _abi.check(lib.hamk_device_malloc(ctypes.byref(d), a.nbytes))
                _abi.check(lib.hamk_memcpy(d, a.ctypes.data, a.nbytes, 0))
            dev.append(d)
        _abi.check(lib.hamk_set_stream(s._h, None))
        _abi.check(lib.hamk_symplectic_steps(s._h, nb, dev[0], dev[1], dt, nsteps, order, iters, dev[2], dev[3], DEVICE))
        _abi.check(lib.hamk_synchronize(s._h))
        for a, d in zip((q, p, res, st), dev):
            if a is not None:
                _abi.check(lib.hamk_memcpy(a.ctypes.data, d, a.nbytes, 1))
    finally:
        for d in dev:
            lib.hamk_device_free(d)
    return q, p, res, st


def make_system(name, monkeypatch):
    from hamilton_amd import api
    base, _, variant = name.partition("@")
    if variant == "jets":
        monkeypatch.setenv("HAMK_K_SYMBOLIC", "0")
    spec = E.get(base)
    s = api.system_from_spec(spec)
    if base == "doublePendulum":
        assert ("HAS_SYM_K = true" in s.source) == (variant != "jets")
    return spec, s


def sample_phase(spec, o, start, nb):
    q, qd = E.sample_config(spec, start, nb)
    if spec.name.startswith("chain") or "~mixed" in spec.name:             # (the chains' sampling box has qd = 0)
        qd = qd + 0.4 * np.cos(1.0 + np.arange(spec.n * nb, dtype=np.float64).reshape(spec.n, nb))
    return q, o.to_phase_batch(q, qd)


# ---------------------------------------------------------------------------------------------------------------------- 1. values
VALUE_SYSTEMS = ["pendulum", "doublePendulum", "doublePendulum@jets", "opcodeZoo", "room", "chain8", "doublePendulum~mixed"]
# The state bound is the one tests/test_gpu_parity.py applies to several RK4 steps of the same system: test_rk4_vs_oracle's 1e-8
# (relative to max(1, |y|)) for the reference's systems, test_all_codegen_variants_agree's 1e-11 for opcodeZoo and for the double
# pendulum on its jets, the same for chain8 (the bound of its lane-kernel RK4 comparisons), and for the system of mixed-sign inertias
# test_indefinite_mass_matrices_are_inverted_like_the_reference's 1e-9 cond(K) on the lanes the reference itself finds regular.
STATE_BOUND = {"pendulum": 1e-8, "doublePendulum": 1e-8, "room": 1e-8, "doublePendulum@jets": 1e-11, "opcodeZoo": 1e-11, "chain8": 1e-11}
_reference = {}


def reference(oracle_lib, name, order):
    """The restatement's result for (system, order), computed once and shared by the host-array and the device-array case."""
    if (name, order) not in _reference:
        spec = E.get(name.partition("@")[0])
        o = oracle_lib.OracleSystem(spec)
        q, p = sample_phase(spec, o, 17, B)
        out = dict(q=q, p=p, want=R.restate(o, q, p, 0.01, 10, order, 6))
        if "~mixed" in name:
            K = [o.jacobian(q[:, i]).T @ np.diag(spec.inertia) @ o.jacobian(q[:, i]) for i in range(B)]
            out["scale"] = np.maximum(1.0, np.array([np.linalg.cond(k) for k in K]))
            b = R.restate(o, q * (1 + 1e-9), p * (1 - 1e-9), 0.01, 10, order, 6)
            with np.errstate(invalid="ignore", over="ignore"):
                sens = np.maximum(np.abs(out["want"][0] - b[0]).max(0), np.abs(out["want"][1] - b[1]).max(0)) / 1e-9
            out["keep"] = np.isfinite(sens) & (sens < 1e4)
        _reference[(name, order)] = out
    return _reference[(name, order)]


@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", VALUE_SYSTEMS)
def test_against_the_restatement(lib, oracle_lib, monkeypatch, name, order, mem):
    """10 steps of 0.01 at 6 iterations, host arrays and device arrays: state within the bound the RK4 parity tests apply to the
    system, status words equal."""
    spec, s = make_system(name, monkeypatch)
    ref = reference(oracle_lib, name, order)
    rq, rp, rres, rst = ref["want"]
    gq, gp, gres, gst = steps(lib, s, ref["q"], ref["p"], 0.01, 10, order, 6, mem)
    with np.errstate(invalid="ignore", over="ignore"):
        lane = np.maximum((np.abs(gq - rq) / np.maximum(1.0, np.abs(rq))).max(0), (np.abs(gp - rp) / np.maximum(1.0, np.abs(rp))).max(0))
    if "~mixed" in name:
        keep = ref["keep"]
        assert keep.mean() > 0.5, float(keep.mean())
        err = (lane / ref["scale"])[keep]
        print(name, order, mem, "state err / cond", float(err.max()))
        assert np.array_equal(gst[keep], rst[keep]) and err.max() < 1e-9, float(err.max())
    else:
        print(name, order, mem, "state err", float(lane.max()))
        assert np.array_equal(gst, rst), (gst, rst)
        assert lane.max() < STATE_BOUND[name], (name, order, float(lane.max()))
    fin = np.isfinite(rres) & np.isfinite(gres)
    print("residual: kernel max", float(gres[fin].max()), "restatement max", float(rres[fin].max()))


# ---------------------------------------------------------------------------------------------------------------------- 2. n = 16
def test_chain16_one_step(lib, oracle_lib):
    """n = 16 is where the kernel's spills live: one step at 4 iterations against the restatement (1e-11, the bound of the lane
    kernels' RK4 comparisons), both orders."""
    from hamilton_amd import api
    spec = E.get("chain16")
    s, o = api.system_from_spec(spec), oracle_lib.OracleSystem(spec)
    q, p = sample_phase(spec, o, 17, B)
    for order in (2, 4):
        rq, rp, rres, rst = R.restate(o, q, p, spec.dt, 1, order, 4)
        gq, gp, gres, gst = steps(lib, s, q, p, spec.dt, 1, order, 4)
        err = max(R.relerr(gq, rq), R.relerr(gp, rp))
        print("chain16 order", order, "state err", err, "residual kernel", float(gres.max()), "restatement", float(rres.max()))
        assert np.array_equal(gst, rst) and not gst.any()
        assert err < 1e-11, (order, err)
        assert np.all(gres <= 2 * rres) and np.all(rres <= 2 * gres)


# ---------------------------------------------------------------------------------------------------------------------- 3. bits
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_determinism_and_splitting(lib, oracle_lib, name):
    """Two runs give equal bits; the 257 trajectories stepped as 100 + 157 give the bits of the one call (a launch's result does not
    depend on B); 7 steps in one call are 3 + 4 in two, bit for bit -- host arrays and device arrays alike."""
    from hamilton_amd import api
    spec = E.get(name)
    s, o = api.system_from_spec(spec), oracle_lib.OracleSystem(spec)
    q, p = sample_phase(spec, o, 23, B)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    for order in (2, 4):
        one = steps(lib, s, q, p, spec.dt, 7, order, 5)
        assert not one[3].any() and np.all(one[2] >= 0)
        assert same(one, steps(lib, s, q, p, spec.dt, 7, order, 5))
        assert same(one, steps(lib, s, q, p, spec.dt, 7, order, 5, DEVICE))
        a = steps(lib, s, q[:, :100], p[:, :100], spec.dt, 7, order, 5)
        b = steps(lib, s, q[:, 100:], p[:, 100:], spec.dt, 7, order, 5)
        assert same(one, [np.concatenate([x, y], axis=-1) for x, y in zip(a, b)])
        h1 = steps(lib, s, q, p, spec.dt, 3, order, 5)
        h2 = steps(lib, s, h1[0], h1[1], spec.dt, 4, order, 5)
        assert np.array_equal(h2[0], one[0]) and np.array_equal(h2[1], one[1])
        assert np.array_equal(np.fmax(h1[2], h2[2]), one[2]) and np.array_equal(h1[3] | h2[3], one[3])
        # the optional outputs left out: the same state
        bare = steps(lib, s, q, p, spec.dt, 7, order, 5, residual=False, status=False)
        assert np.array_equal(bare[0], one[0]) and np.array_equal(bare[1], one[1])
    # iters = HAMK_AUTO is 8
    assert same(steps(lib, s, q, p, spec.dt, 2, 2, 0), steps(lib, s, q, p, spec.dt, 2, 2, 8))
    assert not same(steps(lib, s, q, p, 10 * spec.dt, 2, 2, 0)[:2], steps(lib, s, q, p, 10 * spec.dt, 2, 2, 3)[:2])


def test_python_binding(lib, oracle_lib):
    """api.symplecticSteps: numpy arrays, torch tensors in place, one reference-shaped trajectory."""
    import torch
    from hamilton_amd import api
    spec = E.get("doublePendulum")
    s, o = api.system_from_spec(spec), oracle_lib.OracleSystem(spec)
    q, p = sample_phase(spec, o, 5, B)
    want = steps(lib, s, q, p, 0.01, 4, 4, 6)
    ph, res = api.symplecticSteps(0.01, 4, s, api.Phase(q, p), order=4, iters=6, with_residual=True)
    assert np.array_equal(ph.positions, want[0]) and np.array_equal(ph.momenta, want[1]) and np.array_equal(res, want[2])
    assert np.array_equal(np.asarray(s.last_status), want[3])
    tq, tp = torch.from_numpy(q).cuda(), torch.from_numpy(p).cuda()
    out = api.symplecticSteps(0.01, 4, s, api.Phase(tq, tp), order=4, iters=6, inplace=True)
    assert out.positions.data_ptr() == tq.data_ptr() and np.array_equal(tq.cpu().numpy(), want[0]) and np.array_equal(tp.cpu().numpy(), want[1])
    one = api.symplecticSteps(0.01, 4, s, api.Phase(q[:, 3], p[:, 3]), order=4, iters=6)
    assert one.positions.shape == (2,) and np.array_equal(one.positions, want[0][:, 3])


# ---------------------------------------------------------------------------------------------------------------------- 4. stencil
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", ["pendulum", "doublePendulum"])
def test_step_map_is_symplectic_on_the_gpu(lib, name, order):
    """The stencil of tests/test_symplectic.py (same base points, delta, step and iteration counts -- chosen there on the
    restatement), the finite differences taken with numpy from the kernel's outputs: ||M^T J M - J||_max <= 1e-6."""
    from hamilton_amd import api
    spec, c = E.get(name), R.STENCIL[name]
    s = api.system_from_spec(spec)
    nb = c["q0"].shape[1]
    q, p = R.stencil(c["q0"], c["p0"])
    gq, gp, gres, gst = steps(lib, s, q, p, c["dt"], 1, order, R.STENCIL_ITERS[order])
    got = R.symplectic_defect(gq, gp, spec.n, nb)
    print(name, order, "defect", got, "residual", float(gres.max()))
    assert not gst.any() and gres.max() < 1e-14
    assert got <= 1e-6, got


# ---------------------------------------------------------------------------------------------------------------------- 5. residual
def test_residual_falls_with_the_iteration_count(lib, oracle_lib):
    """pendulum at dt = 0.5, positions within 0.6 rad of the bottom (there the fixed-point map contracts slowly enough that 16
    iterations leave a residual far above roundoff on EVERY lane -- checked on the restatement first): the residual falls from 2 to
    4 to 8 to 16 iterations on every lane, and at 16 it is the restatement's to a factor of 2."""
    from hamilton_amd import api
    spec = E.get("pendulum")
    s, o = api.system_from_spec(spec), oracle_lib.OracleSystem(spec)
    q = np.linspace(-0.6, 0.6, B).reshape(1, B)
    p = 0.8 * np.cos(1.0 + np.arange(B, dtype=np.float64)).reshape(1, B)
    rres = R.restate(o, q, p, 0.5, 1, 2, 16)[2]
    assert rres.min() > 1e-13, rres.min()
    got = [steps(lib, s, q, p, 0.5, 1, 2, it)[2] for it in (2, 4, 8, 16)]
    print("residual max at 2, 4, 8, 16 iterations:", [float(g.max()) for g in got], "restatement at 16:", float(rres.max()))
    for a, b in zip(got, got[1:]):
        assert np.all(b < a)
    assert np.all(got[3] <= 2 * rres) and np.all(rres <= 2 * got[3])


# ---------------------------------------------------------------------------------------------------------------------- 6. singular lane
def test_a_singular_lane_among_healthy_ones(lib, oracle_lib):
    """twoBody at r = 0 (test_gpu_parity.py test_nonfinite_is_flagged's point: K = diag(mu, mu r^2) is singular there): that lane is
    flagged SINGULAR and / or NONFINITE, the call is HAMK_OK, and the other 256 lanes hold the bits of a run in which that lane
    had an ordinary input."""
    from hamilton_amd import api
    spec = E.get("twoBody")
    s, o = api.system_from_spec(spec), oracle_lib.OracleSystem(spec)
    q, p = sample_phase(spec, o, 9, B)
    lane = 37
    bad_q, bad_p = q.copy(), p.copy()
    bad_q[:, lane] = (0.0, 0.0)
    bad_p[:, lane] = (0.0, 1.0)
    want = steps(lib, s, q, p, 0.01, 5, 2, 6)
    got = steps(lib, s, bad_q, bad_p, 0.01, 5, 2, 6)              # (steps() checks the return code: HAMK_OK)
    keep = np.arange(B) != lane
    assert got[3][lane] & 3 and not got[3][keep].any() and not want[3].any(), got[3][lane]
    for a, b in zip(got[:3], want[:3]):
        assert np.array_equal(a[..., keep], b[..., keep])
