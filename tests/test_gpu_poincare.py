"""GPU: hamk_poincare_steps through the C ABI of libhamk.so -- the companion module's kernel as the GPU compiler built it --
against the numpy restatement of the scheme over the oracle's hamEqs, the oracle's own RK4 state and the two analytic anchors
(all from tests/test_poincare.py), plus what only the real launch can show: bit-reproducibility, independence of B and of how a
run is cut into calls, q, p independent of the surface, a NaN lane among healthy ones, host arrays against device arrays, the
Python binding on device tensors.  B = 257: two blocks, the second holding one lane."""
import ctypes

import numpy as np
import pytest

import test_poincare as R                    # the restatement, the anchors, the inputs and the bounds live in the CPU test module
from hamilton_amd import examples as E

pytestmark = pytest.mark.gpu

B = R.B
HOST, DEVICE = 0, 1


@pytest.fixture(scope="module")
def lib(hamk_lib):
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return hamk_lib


def steps(lib, s, q, p, dt, nsteps, coord, level=0.0, period=0.0, direction=1, max_hits=16, hits=None, step0=0, sentinel=0.0, thit=True,
          status=True, mem=HOST):
    """One hamk_poincare_steps call on copies -> a dict like test_poincare.restate's (hits: a dict q, p, t, n to continue from);
    mem = DEVICE goes through hamk_device_malloc'ed arrays and is synchronised before the copy back."""
    from hamilton_amd import _abi
    q, p = (np.ascontiguousarray(a, dtype=np.float64).copy() for a in (q, p))
    n, nb = q.shape
    h = R.new_hits(n, nb, max_hits, sentinel) if hits is None else {k: np.array(v) for k, v in hits.items()}
    st = np.full(nb, -1, np.int32) if status else None
    arrays = (q, p, h["q"], h["p"], h["t"] if thit else None, h["n"], st)
    ptr = lambda a: None if a is None else a.ctypes.data
    args = (dt, int(nsteps), int(coord), level, period, int(direction), int(max_hits))
    if mem == HOST:
        _abi.check(lib.hamk_poincare_steps(s._h, nb, ptr(q), ptr(p), *args, *(ptr(a) for a in arrays[2:6]), int(step0), ptr(st), HOST))
    else:
        dev = []
        try:
            for a in arrays:
                d = ctypes.c_void_p()
                if a is not None:
                    _abi.check(lib.hamk_device_malloc(ctypes.byref(d), a.nbytes))
                    _abi.check(lib.hamk_memcpy(d, a.ctypes.data, a.nbytes, 0))
                dev.append(d)
            _abi.check(lib.hamk_set_stream(s._h, None))
            _abi.check(lib.hamk_poincare_steps(s._h, nb, dev[0], dev[1], *args, *dev[2:6], int(step0), dev[6], DEVICE))
            _abi.check(lib.hamk_synchronize(s._h))
            for a, d in zip(arrays, dev):
                if a is not None:
                    _abi.check(lib.hamk_memcpy(a.ctypes.data, d, a.nbytes, 1))
        finally:
            for d in dev:
                lib.hamk_device_free(d)
    return dict(q=q, p=p, hq=h["q"], hp=h["p"], ht=h["t"], n=h["n"], status=st)


_systems = {}


def system(name):
    """One handle per system for the whole module: the companion module is built and loaded once."""
    from hamilton_amd import api
    if name not in _systems:
        _systems[name] = api.system_from_spec(E.get(name))
    return _systems[name]


# ---------------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("direction", [1, -1, 0])
def test_rotor_anchor(lib, direction, mem):
    """Counts from floor arithmetic, crossing times from (target - q0) / p within the rounding bound, the momentum bit for bit,
    fewer rows than the fastest lanes have crossings."""
    q, p = R.rotor_inputs()
    got = steps(lib, R.anchor_system("rotor"), q, p, R.ROTOR_DT, R.ROTOR_N, 0, 0.0, R.TWO_PI, direction, R.ROTOR_MAX_HITS, sentinel=-7.0, mem=mem)
    R.check_rotor(got, direction, "MI355X")


@pytest.mark.parametrize("direction", [1, -1, 0])
@pytest.mark.parametrize("case", R.OSC_CASES, ids=lambda c: "dt%g-n%d" % c)
def test_oscillator_anchor(lib, case, direction):
    """Count, theta and the hit state against numpy.roots on the closed-form cubic of every crossing step."""
    dt, nsteps = case
    q, p = R.osc_inputs()
    got = steps(lib, R.anchor_system("oscillator"), q, p, dt, nsteps, 0, 0.0, 0.0, direction, 8)
    R.check_oscillator(got, dt, nsteps, direction, 8, "MI355X")


# ---------------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("name", R.SYSTEMS)
def test_against_the_restatement(lib, oracle_lib, name, mem):
    """nhit equal; q, p against the oracle's rk4_steps_batch at the system's STATE_BOUND; thit and the hit states within 4 x what a
    1e-12 perturbation of every hamEqs output moves them in the restatement; every stored hit on its surface and near H0."""
    ref = R.reference(oracle_lib, name)
    got = steps(lib, system(name), ref["q"], ref["p"], R.DT, ref["nsteps"], mem=mem, **ref["kw"])
    R.check_against_reference(ref, name, got, "MI355X " + ("host arrays" if mem == HOST else "device arrays"))


# ---------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_properties(lib, oracle_lib, name):
    """test_poincare.run_properties on the real launch (cut invariance, q and p independent of the surface, the sentinel beyond
    the count, thit = NULL, counts at entry), and: two identical calls agree bitwise; lanes 0..63 stepped alone (B = 64) are the
    same lanes of the B = 257 call; host arrays equal device arrays."""
    ref = R.reference(oracle_lib, name)
    s = system(name)
    run = lambda q, p, nsteps, **kw: steps(lib, s, q, p, R.DT, nsteps, **kw)
    one = R.run_properties(run, ref, name)
    q, p, kw, N = ref["q"], ref["p"], ref["kw"], ref["nsteps"]
    assert not one["status"].any()
    assert R.same(one, run(q, p, N, sentinel=-7.0, **kw))
    assert R.same(one, run(q, p, N, sentinel=-7.0, mem=DEVICE, **kw))
    few = run(q[:, :64], p[:, :64], N, sentinel=-7.0, **kw)
    assert R.same(few, {k: v[..., :64] for k, v in one.items()})
    assert R.same(one, run(q, p, N, sentinel=-7.0, status=False, **kw))


def test_a_nan_lane_among_healthy_ones(lib, oracle_lib):
    """A NaN is an ordinary value to this kernel: that lane records nothing and ends flagged HAMK_ST_NONFINITE, the call is HAMK_OK
    (steps() checks the return code), and the other 256 lanes hold the bits of a run without it."""
    ref = R.reference(oracle_lib, "doublePendulum")
    s = system("doublePendulum")
    R.run_nan_lane(lambda q, p, nsteps, **kw: steps(lib, s, q, p, R.DT, nsteps, **kw), ref, 37)


def test_order_of_the_first_crossing_time(lib, oracle_lib):
    s = system("pendulum")
    R.check_order(oracle_lib, lambda q, p, dt, nsteps, **kw: steps(lib, s, q, p, dt, nsteps, **kw), "MI355X")


# ---------------------------------------------------------------------------------------------------------------------- binding
def test_python_binding(lib, oracle_lib):
    """api.poincareSteps: torch device tensors equal the ABI call, out of place, continued from the returned Hits, and in place;
    numpy arrays; one reference-shaped trajectory."""
    import torch
    from hamilton_amd import api
    ref = R.reference(oracle_lib, "doublePendulum")
    s = system("doublePendulum")
    q, p, kw, N = ref["q"], ref["p"], ref["kw"], ref["nsteps"]
    want = steps(lib, s, q, p, R.DT, N, **kw)
    n1 = N // 3
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    host = lambda h: dict(hq=h.positions.cpu().numpy(), hp=h.momenta.cpu().numpy(), ht=h.times.cpu().numpy(), n=h.count.cpu().numpy())
    tq, tp = cu(q), cu(p)
    ph, hits = api.poincareSteps(R.DT, N, s, api.Phase(tq, tp), **kw)
    got = dict(q=ph.positions.cpu().numpy(), p=ph.momenta.cpu().numpy(), **host(hits))
    assert R.same(got, want) and np.array_equal(s.last_status.cpu().numpy(), want["status"])
    assert np.array_equal(tq.cpu().numpy(), q)                                                   # out of place: inputs untouched
    ph1, h1 = api.poincareSteps(R.DT, n1, s, api.Phase(tq, tp), **kw)                             # N1 + N2, the Hits passed back
    before = host(h1)
    ph2, h2 = api.poincareSteps(R.DT, N - n1, s, ph1, kw["coord"], kw["level"], kw["period"], kw["direction"], hits=h1, step0=n1)
    assert R.same(dict(q=ph2.positions.cpu().numpy(), p=ph2.momenta.cpu().numpy(), **host(h2)), want)
    assert R.same(host(h1), before, ("hq", "hp", "ht", "n"))                                     # ... which were not advanced in place
    ph3, h3 = api.poincareSteps(R.DT, N - n1, s, ph1, kw["coord"], kw["level"], kw["period"], kw["direction"], hits=h1, step0=n1, inplace=True)
    assert ph3.positions.data_ptr() == ph1.positions.data_ptr() and h3.count.data_ptr() == h1.count.data_ptr()
    assert R.same(dict(q=ph1.positions.cpu().numpy(), p=ph1.momenta.cpu().numpy(), **host(h1)), want)
    ph, hits = api.poincareSteps(R.DT, N, s, api.Phase(q, p), **kw)                               # numpy arrays
    assert R.same(dict(q=ph.positions, p=ph.momenta, hq=hits.positions, hp=hits.momenta, ht=hits.times, n=hits.count), want)
    ph, hits = api.poincareSteps(R.DT, N, s, api.Phase(q[:, 3], p[:, 3]), **kw)                   # one trajectory
    assert ph.positions.shape == (2,) and np.array_equal(ph.positions, want["q"][:, 3]) and hits.positions.shape == (kw["max_hits"], 2)
    assert np.array_equal(hits.positions, want["hq"][:, :, 3]) and np.array_equal(hits.times, want["ht"][:, 3]) and hits.count == want["n"][3]
