"""GPU: hamk_lyapunov_steps through the C ABI of libhamk.so -- the companion module's kernel as the GPU compiler built it --
against the numpy restatement of the scheme over the oracle's hamEqs, the oracle's own RK4 state and the two analytic anchors
(all from tests/test_lyapunov.py), plus what only the real launch can show: bit-reproducibility, independence of B and of how a
run is cut into calls, q, p independent of the shadow, a NaN lane among healthy ones, the Python binding on device tensors.
B = 257: two blocks, the second holding one lane."""
import ctypes

import numpy as np
import pytest

import test_lyapunov as R                    # the restatement, the anchors, the inputs and the bounds live in the CPU test module
from hamilton_amd import examples as E

pytestmark = pytest.mark.gpu

B = R.B
HOST, DEVICE = 0, 1


@pytest.fixture(scope="module")
def lib(hamk_lib):
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return hamk_lib


def steps(lib, s, q, p, wq, wp, dt, nintervals, every, d0, logsum=None, mem=HOST, status=True):
    """One hamk_lyapunov_steps call on copies ([n, B] host arrays, logsum [B] or zeros) -> (q, p, wq, wp, logsum, status);
    mem = DEVICE goes through hamk_device_malloc'ed arrays and is synchronised before the copy back."""
    from hamilton_amd import _abi
    q, p, wq, wp = (np.ascontiguousarray(a, dtype=np.float64).copy() for a in (q, p, wq, wp))
    nb = q.shape[1]
    ls = np.zeros(nb) if logsum is None else np.array(logsum, dtype=np.float64)
    st = np.full(nb, -1, np.int32) if status else None
    arrays = (q, p, wq, wp, ls, st)
    ptr = lambda a: None if a is None else a.ctypes.data
    if mem == HOST:
        _abi.check(lib.hamk_lyapunov_steps(s._h, nb, ptr(q), ptr(p), ptr(wq), ptr(wp), dt, nintervals, every, d0, ptr(ls), ptr(st), HOST))
        return arrays
    dev = []
    try:
        for a in arrays:
            d = ctypes.c_void_p()
            if a is not None:
                _abi.check(lib.hamk_device_malloc(ctypes.byref(d), a.nbytes))
                _abi.check(lib.hamk_memcpy(d, a.ctypes.data, a.nbytes, 0))
            dev.append(d)
        _abi.check(lib.hamk_set_stream(s._h, None))
        _abi.check(lib.hamk_lyapunov_steps(s._h, nb, dev[0], dev[1], dev[2], dev[3], dt, nintervals, every, d0, dev[4], dev[5], DEVICE))
        _abi.check(lib.hamk_synchronize(s._h))
        for a, d in zip(arrays, dev):
            if a is not None:
                _abi.check(lib.hamk_memcpy(a.ctypes.data, d, a.nbytes, 1))
    finally:
        for d in dev:
            lib.hamk_device_free(d)
    return arrays


_systems = {}


def system(name):
    """One handle per system for the whole module: the companion module is built and loaded once."""
    from hamilton_amd import api
    if name not in _systems:
        _systems[name] = api.system_from_spec(E.get(name))
    return _systems[name]


# ---------------------------------------------------------------------------------------------------------------------- 1. values
@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("d0", R.D0S)
@pytest.mark.parametrize("name", R.SYSTEMS)
def test_against_the_restatement(lib, oracle_lib, name, d0, mem):
    """4 intervals of 5 steps of 0.01 on all 257 lanes: q, p against the oracle's rk4_steps_batch at the system's STATE_BOUND; logsum
    and w within 4 x what a 1e-12 perturbation of every hamEqs output moves them in the restatement; status words equal."""
    ref = R.reference(oracle_lib, name, d0)
    got = steps(lib, system(name), ref["q"], ref["p"], ref["wq"], ref["wp"], R.DT, R.NINT, R.EVERY, d0, mem=mem)
    R.check_against_reference(ref, name, got, "MI355X " + ("host arrays" if mem == HOST else "device arrays"))


@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("case", R.ANCHOR_CASES, ids=lambda c: "dt%g-every%d-n%d-d0%g" % c)
@pytest.mark.parametrize("start", ["zero", "random"])
@pytest.mark.parametrize("kind", R.ANCHOR_KINDS)
def test_analytic_anchors(lib, kind, start, case, mem):
    """logsum against the closed forms (saddle: N log R; oscillator: N / 2 log1p(-dt^6 / 72 + dt^8 / 576) for any unit w) within
    N (8 eps ymax / d0 + 32 eps), every lane."""
    dt, every, nint, d0 = case
    q, p, wq, wp = R.anchor_inputs(kind, start)
    R.check_anchor(kind, case, steps(lib, R.anchor_system(kind), q, p, wq, wp, dt, nint, every, d0, mem=mem), "MI355X")


# ---------------------------------------------------------------------------------------------------------------------- 2. bits
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_determinism_splitting_and_the_shadow(lib, oracle_lib, name):
    """Two identical calls agree bitwise, host arrays and device arrays alike; lanes 0..63 stepped alone (B = 64) are the same lanes
    of the B = 257 call; 4 intervals are 2 + 2 with w and logsum carried, bitwise on all five outputs; q, p are bitwise
    independent of (w, d0)."""
    ref = R.reference(oracle_lib, name, 1e-6)
    s = system(name)
    q, p, wq, wp = ref["q"], ref["p"], ref["wq"], ref["wp"]
    start = np.linspace(-1.0, 1.0, B)
    one = steps(lib, s, q, p, wq, wp, R.DT, 4, R.EVERY, 1e-6, start)
    assert not one[5].any() and all(np.isfinite(a).all() for a in one[:5]) and not np.array_equal(one[4], start)
    assert R.same(one, steps(lib, s, q, p, wq, wp, R.DT, 4, R.EVERY, 1e-6, start))
    assert R.same(one, steps(lib, s, q, p, wq, wp, R.DT, 4, R.EVERY, 1e-6, start, mem=DEVICE))
    few = steps(lib, s, q[:, :64], p[:, :64], wq[:, :64], wp[:, :64], R.DT, 4, R.EVERY, 1e-6, start[:64])
    assert R.same(few, [a[..., :64] for a in one])
    h1 = steps(lib, s, q, p, wq, wp, R.DT, 2, R.EVERY, 1e-6, start)
    h2 = steps(lib, s, *h1[:4], R.DT, 2, R.EVERY, 1e-6, h1[4])
    assert R.same(one[:5], h2[:5]) and np.array_equal(one[5], h1[5] | h2[5])
    w2q, w2p = R.unit_w(q.shape[0], B, 99)
    for other in (steps(lib, s, q, p, w2q, w2p, R.DT, 4, R.EVERY, 1e-6), steps(lib, s, q, p, wq, wp, R.DT, 4, R.EVERY, 1e-3),
                  steps(lib, s, q, p, 3.0 * w2q, -2.0 * w2p, R.DT, 4, R.EVERY, 1e-9)):
        assert np.array_equal(other[0], one[0]) and np.array_equal(other[1], one[1])
        assert not np.array_equal(other[2], one[2])
    # status left out: the same five outputs
    assert R.same(steps(lib, s, q, p, wq, wp, R.DT, 4, R.EVERY, 1e-6, start, status=False)[:5], one[:5])


def test_a_nan_lane_among_healthy_ones(lib, oracle_lib):
    """A NaN is an ordinary value to this kernel: that lane ends flagged HAMK_ST_NONFINITE, the call is HAMK_OK, and the other 256
    lanes hold the bits of a run without it."""
    ref = R.reference(oracle_lib, "doublePendulum", 1e-6)
    s = system("doublePendulum")
    q, p, wq, wp = ref["q"], ref["p"], ref["wq"], ref["wp"]
    lane = 37
    bad = q.copy()
    bad[0, lane] = np.nan
    want = steps(lib, s, q, p, wq, wp, R.DT, 2, R.EVERY, 1e-6)
    got = steps(lib, s, bad, p, wq, wp, R.DT, 2, R.EVERY, 1e-6)                      # (steps() checks the return code: HAMK_OK)
    keep = np.arange(B) != lane
    assert got[5][lane] & 2 and not got[5][keep].any() and not want[5].any(), got[5][lane]
    assert R.same([a[..., keep] for a in got[:5]], [a[..., keep] for a in want[:5]])


# ---------------------------------------------------------------------------------------------------------------------- 3. binding
def test_python_binding(lib, oracle_lib):
    """api.lyapunovSteps: torch device tensors equal the ABI call, in place and out of place; numpy arrays; the defaults
    (w = 1 / sqrt(2n) on every component, logsum = 0); one reference-shaped trajectory."""
    import torch
    from hamilton_amd import api
    ref = R.reference(oracle_lib, "doublePendulum", 1e-6)
    s = system("doublePendulum")
    q, p, wq, wp = ref["q"], ref["p"], ref["wq"], ref["wp"]
    start = np.linspace(-1.0, 1.0, B)
    want = steps(lib, s, q, p, wq, wp, R.DT, 3, R.EVERY, 1e-6, start)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tq, tp, twq, twp, tls = cu(q), cu(p), cu(wq), cu(wp), cu(start)
    ph, w, ls = api.lyapunovSteps(R.DT, 3, R.EVERY, s, api.Phase(tq, tp), w=api.Phase(twq, twp), d0=1e-6, logsum=tls)
    got = [t.cpu().numpy() for t in (ph.positions, ph.momenta, w.positions, w.momenta, ls)]
    assert R.same(got, want[:5]) and np.array_equal(s.last_status.cpu().numpy(), want[5])
    assert np.array_equal(tq.cpu().numpy(), q) and np.array_equal(tls.cpu().numpy(), start)         # out of place: inputs untouched
    ph, w, ls = api.lyapunovSteps(R.DT, 3, R.EVERY, s, api.Phase(tq, tp), w=api.Phase(twq, twp), d0=1e-6, logsum=tls, inplace=True)
    assert ph.positions.data_ptr() == tq.data_ptr() and w.momenta.data_ptr() == twp.data_ptr() and ls.data_ptr() == tls.data_ptr()
    assert R.same([t.cpu().numpy() for t in (tq, tp, twq, twp, tls)], want[:5])
    ph, w, ls = api.lyapunovSteps(R.DT, 3, R.EVERY, s, api.Phase(q, p), w=api.Phase(wq, wp), d0=1e-6, logsum=start)
    assert R.same([ph.positions, ph.momenta, w.positions, w.momenta, ls], want[:5])
    c = np.full_like(q, 1.0 / np.sqrt(2.0 * s.n))
    dflt = steps(lib, s, q, p, c, c, R.DT, 3, R.EVERY, 1e-7)
    ph, w, ls = api.lyapunovSteps(R.DT, 3, R.EVERY, s, api.Phase(q, p))
    assert R.same([ph.positions, ph.momenta, w.positions, w.momenta, ls], dflt[:5])
    ph, w, ls = api.lyapunovSteps(R.DT, 3, R.EVERY, s, api.Phase(q[:, 3], p[:, 3]), w=api.Phase(wq[:, 3], wp[:, 3]), d0=1e-6, logsum=start[3:4])
    assert ph.positions.shape == (2,) and np.array_equal(ph.positions, want[0][:, 3]) and np.array_equal(w.momenta, want[3][:, 3]) and ls == want[4][3]
