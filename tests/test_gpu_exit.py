"""GPU: hamk_exit_steps through the C ABI of libhamk.so -- the companion module's kernel as the GPU compiler built it -- against the
numpy restatement of the scheme over the oracle's hamEqs and the three analytic anchors (all from tests/test_exit.py), plus what only
the real launch can show: the wave-wide break (ragged wavefronts, work that is dropped), bit-reproducibility, independence of B and
of how a run is cut into calls, lanes stopped at entry, a NaN lane among healthy ones, host arrays against device arrays, the Python
binding on device tensors.  B = 257: four wavefronts and one lane, so the block edge at 256 is covered."""
import ctypes
import time

import numpy as np
import pytest

import test_exit as R                        # the restatement, the anchors, the inputs and the bounds live in the CPU test module
from hamilton_amd import examples as E

pytestmark = pytest.mark.gpu

B = R.B
HOST, DEVICE = 0, 1


@pytest.fixture(scope="module")
def lib(hamk_lib):
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return hamk_lib


class DeviceArrays:
    """The arrays of one call in hamk_device_malloc'ed memory: put() copies the host arrays in, get() copies them back."""

    def __init__(self, lib, arrays):
        from hamilton_amd import _abi
        self.lib, self.arrays, self.dev = lib, arrays, []
        for a in arrays:
            d = ctypes.c_void_p()
            if a is not None:
                _abi.check(lib.hamk_device_malloc(ctypes.byref(d), a.nbytes))
            self.dev.append(d)

    def put(self):
        from hamilton_amd import _abi
        for a, d in zip(self.arrays, self.dev):
            if a is not None:
                _abi.check(self.lib.hamk_memcpy(d, a.ctypes.data, a.nbytes, 0))

    def get(self):
        from hamilton_amd import _abi
        for a, d in zip(self.arrays, self.dev):
            if a is not None:
                _abi.check(self.lib.hamk_memcpy(a.ctypes.data, d, a.nbytes, 1))

    def free(self):
        for d in self.dev:
            self.lib.hamk_device_free(d)


def steps(lib, s, q, p, dt, nsteps, gates, exits=None, step0=0, sentinel=0.0, record=True, status=True, mem=HOST):
    """One hamk_exit_steps call on copies -> a dict like test_exit.restate's (exits: a dict code, t, q, p to continue from;
    record=False: qexit = pexit = NULL); mem = DEVICE goes through hamk_device_malloc'ed arrays and is synchronised before the copy
    back."""
    from hamilton_amd import _abi
    q, p = (np.ascontiguousarray(a, dtype=np.float64).copy() for a in (q, p))
    n, nb = q.shape
    e = R.new_exits(n, nb, sentinel) if exits is None else {k: np.array(v) for k, v in exits.items()}
    st = np.full(nb, -1, np.int32) if status else None
    arrays = (q, p, e["code"], e["t"], e["q"] if record else None, e["p"] if record else None, st)
    ptr = lambda a: None if a is None else a.ctypes.data
    g = R.gate_struct(gates)
    head = (dt, int(nsteps), ctypes.addressof(g), len(gates))
    if mem == HOST:
        _abi.check(lib.hamk_exit_steps(s._h, nb, ptr(q), ptr(p), *head, *(ptr(a) for a in arrays[2:6]), int(step0), ptr(st), HOST))
    else:
        d = DeviceArrays(lib, arrays)
        try:
            d.put()
            _abi.check(lib.hamk_set_stream(s._h, None))
            _abi.check(lib.hamk_exit_steps(s._h, nb, d.dev[0], d.dev[1], *head, *d.dev[2:6], int(step0), d.dev[6], DEVICE))
            _abi.check(lib.hamk_synchronize(s._h))
            d.get()
        finally:
            d.free()
    return dict(q=q, p=p, code=e["code"], t=e["t"], eq=e["q"], ep=e["p"], status=st)


_systems = {}


def system(name):
    """One handle per system for the whole module: the companion module is built and loaded once."""
    from hamilton_amd import api
    if name not in _systems:
        _systems[name] = api.system_from_spec(E.get(name))
    return _systems[name]


# ---------------------------------------------------------------------------------------------------------------------- anchors
@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
def test_rotor_anchor(lib, mem):
    """Code and side follow the sign of p, lanes at rest keep code -1, exit times from (+-pi - q0) / p within the rounding bound."""
    q, p = R.rotor_inputs(B)
    got = steps(lib, R.anchor_system("rotor"), q, p, R.ROTOR_DT, R.ROTOR_N, R.ROTOR_GATES, sentinel=-7.0, mem=mem)
    R.check_rotor(got, "MI355X", B)


@pytest.mark.parametrize("case", R.OSC_CASES, ids=lambda c: "dt%g-n%d" % c)
def test_oscillator_anchor(lib, case):
    """Code, theta and the exit state against numpy.roots on the closed-form cubic of the exit step."""
    dt, nsteps = case
    q, p = R.osc_inputs()
    got = steps(lib, R.anchor_system("oscillator"), q, p, dt, nsteps, [(0, -R.OSC_C, R.OSC_C)])
    R.check_oscillator(got, dt, nsteps, "MI355X")


def test_free_particle_gate_order(lib):
    """The smaller theta wins, the lower index wins a tie, a start outside a gate has theta = 0 and texit = step0."""
    q, p = R.free_inputs()
    R.check_free(steps(lib, R.anchor_system("free"), q, p, R.FREE_DT, 4, R.FREE_GATES, sentinel=-7.0, step0=10), "MI355X")


# ---------------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("name", R.SYSTEMS)
def test_against_the_restatement(lib, oracle_lib, name, mem):
    """Codes equal; texit, the exit state and q, p within 4 x what a 1e-12 perturbation of every hamEqs output moves them in the
    restatement; every exit state on its bound."""
    ref = R.reference(oracle_lib, name)
    got = steps(lib, system(name), ref["q"], ref["p"], R.DT, ref["nsteps"], ref["gates"], mem=mem)
    R.check_against_reference(ref, name, got, "MI355X " + ("host arrays" if mem == HOST else "device arrays"))


# ---------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_properties(lib, oracle_lib, name):
    """test_exit.run_properties on the real launch (cut invariance, freeze, gate independence, lanes stopped at entry, qexit = pexit
    = NULL, infinite bounds), and: two identical calls agree bitwise; lanes 0..63 stepped alone (B = 64) are the same lanes of the
    B = 257 call -- the break of one wavefront does not leak into another; host arrays equal device arrays."""
    ref = R.reference(oracle_lib, name)
    s = system(name)
    run = lambda q, p, nsteps, gates, **kw: steps(lib, s, q, p, R.DT, nsteps, gates, **kw)
    one = R.run_properties(run, ref, name)
    q, p, gates, N = ref["q"], ref["p"], ref["gates"], ref["nsteps"]
    both = R.OUT + ("status",)
    assert R.same(one, run(q, p, N, gates, sentinel=-7.0), both)
    assert R.same(one, run(q, p, N, gates, sentinel=-7.0, mem=DEVICE), both)
    few = run(q[:, :64], p[:, :64], N, gates, sentinel=-7.0)
    assert R.same(few, R.lanes(one, slice(0, 64)), both)
    assert R.same(one, run(q, p, N, gates, sentinel=-7.0, status=False))


def test_a_nan_lane_among_healthy_ones(lib, oracle_lib):
    """A NaN is an ordinary value to this kernel: that lane stops with code -2 after its first step and is flagged
    HAMK_ST_NONFINITE, the call is HAMK_OK (steps() checks the return code), and the other 256 lanes hold the bits of a run
    without it."""
    ref = R.reference(oracle_lib, "doublePendulum")
    s = system("doublePendulum")
    R.run_nan_lane(lambda q, p, nsteps, gates, **kw: steps(lib, s, q, p, R.DT, nsteps, gates, **kw), ref, 37)


# ---------------------------------------------------------------------------------------------------------------------- the break
def test_ragged_wavefronts(lib, oracle_lib):
    """pendulum: lanes 64 .. 127 -- one whole wavefront -- swing over within 20 steps, every other lane librates for 400.  The launch
    returns (no barrier waits for the wavefront that left), and the survivors hold bitwise what the same lanes hold in a launch
    without the early wavefront."""
    spec = E.get("pendulum")
    o = oracle_lib.OracleSystem(spec)
    lane = np.arange(B, dtype=np.float64)
    early = (np.arange(B) >= 64) & (np.arange(B) < 128)
    q = np.where(early, 3.0, 0.5 * np.sin(1.0 + 0.37 * lane)).reshape(1, -1)
    qd = np.where(early, 5.0 + 0.01 * lane, 0.0).reshape(1, -1)
    p = o.to_phase_batch(q, qd)
    gates = [(0, -R.PI, R.PI)]
    want = R.restate(o, q, p, R.DT, 400, gates)
    assert (want["steps"][early] <= 20).all() and (want["code"][early] == 1).all() and (want["code"][~early] == R.ALIVE).all()
    s = system("pendulum")
    got = steps(lib, s, q, p, R.DT, 400, gates, sentinel=-7.0)
    assert np.array_equal(got["code"], want["code"]) and not got["status"].any()
    assert np.abs(got["t"] - want["t"])[early].max() < 1e-9 and (got["t"][~early] == -7.0).all()
    alone = steps(lib, s, q[:, ~early], p[:, ~early], R.DT, 400, gates, sentinel=-7.0)
    assert R.same(alone, R.lanes(got, ~early), R.OUT + ("status",))
    assert (np.abs(alone["q"]) < 0.6).all()                                                             # ... and have kept librating


def test_work_is_dropped(lib):
    """rotor, B = 257.  Call A: every lane leaves within 20 steps, nsteps = 200 000.  Call B: no lane leaves, nsteps = 2 000.  Without
    the wavefront break A does 100 x B's work, with it 1 / 100: t(A) < t(B), no measured constant needed.  Both on device arrays,
    timed by device synchronisation after one warm-up each."""
    from hamilton_amd import _abi
    s = R.anchor_system("rotor")
    lane = np.arange(B)
    gates = R.gate_struct(R.ROTOR_GATES)
    cases = {"A": (np.where(lane % 2 == 0, 4.0, -4.0), 200000), "B": (np.zeros(B), 2000)}
    seconds, codes = {}, {}
    for name, (p0, nsteps) in cases.items():
        q, p = (2.0 * np.sign(p0)).reshape(1, -1).copy(), p0.reshape(1, -1).copy()                     # A: 1.14 from the bound at speed 4: 15 steps of 0.02
        e = R.new_exits(1, B)
        st = np.zeros(B, np.int32)
        d = DeviceArrays(lib, (q, p, e["code"], e["t"], e["q"], e["p"], st))
        try:
            _abi.check(lib.hamk_set_stream(s._h, None))
            for _ in ("warm-up", "timed"):
                d.put()                                                                                 # a fresh run each time
                _abi.check(lib.hamk_synchronize(s._h))
                t0 = time.perf_counter()
                _abi.check(lib.hamk_exit_steps(s._h, B, d.dev[0], d.dev[1], R.ROTOR_DT, nsteps, ctypes.addressof(gates), 1, *d.dev[2:6], 0, d.dev[6], DEVICE))
                _abi.check(lib.hamk_synchronize(s._h))
                seconds[name] = time.perf_counter() - t0
            d.get()
            codes[name] = e["code"].copy()
            if name == "A":
                assert (e["t"] < 20.0).all() and (e["t"] > 10.0).all()
        finally:
            d.free()
    print("work is dropped: t(A) =", seconds["A"], "s for 200000 steps asked, t(B) =", seconds["B"], "s for 2000 steps run")
    assert np.array_equal(codes["A"], np.where(lane % 2 == 0, 1, 0)) and (codes["B"] == R.ALIVE).all()
    assert seconds["A"] < seconds["B"], seconds


# ---------------------------------------------------------------------------------------------------------------------- binding
def test_python_binding(lib, oracle_lib):
    """api.exitSteps: torch device tensors equal the ABI call, out of place, continued from the returned Exits, and in place; numpy
    arrays; one reference-shaped trajectory."""
    import torch
    from hamilton_amd import api
    ref = R.reference(oracle_lib, "doublePendulum")
    s = system("doublePendulum")
    q, p, gates, N = ref["q"], ref["p"], ref["gates"], ref["nsteps"]
    want = steps(lib, s, q, p, R.DT, N, gates)
    n1 = N // 3
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    host = lambda x: dict(code=x.code.cpu().numpy(), t=x.t.cpu().numpy(), eq=x.q.cpu().numpy(), ep=x.p.cpu().numpy())
    tq, tp = cu(q), cu(p)
    ph, ex = api.exitSteps(R.DT, N, s, api.Phase(tq, tp), gates)
    got = dict(q=ph.positions.cpu().numpy(), p=ph.momenta.cpu().numpy(), **host(ex))
    assert R.same(got, want) and np.array_equal(s.last_status.cpu().numpy(), want["status"])
    assert ex.code.dtype == torch.int32 and np.array_equal(tq.cpu().numpy(), q)                   # out of place: inputs untouched
    ph1, x1 = api.exitSteps(R.DT, n1, s, api.Phase(tq, tp), gates)                                # N1 + N2, the Exits passed back
    before = host(x1)
    ph2, x2 = api.exitSteps(R.DT, N - n1, s, ph1, gates, exits=x1, step0=n1)
    assert R.same(dict(q=ph2.positions.cpu().numpy(), p=ph2.momenta.cpu().numpy(), **host(x2)), want)
    assert R.same(host(x1), before, ("code", "t", "eq", "ep"))                                    # ... which were not advanced in place
    ph3, x3 = api.exitSteps(R.DT, N - n1, s, ph1, gates, exits=x1, step0=n1, inplace=True)
    assert ph3.positions.data_ptr() == ph1.positions.data_ptr() and x3.code.data_ptr() == x1.code.data_ptr()
    assert R.same(dict(q=ph1.positions.cpu().numpy(), p=ph1.momenta.cpu().numpy(), **host(x1)), want)
    ph, ex = api.exitSteps(R.DT, N, s, api.Phase(q, p), gates)                                    # numpy arrays
    assert R.same(dict(q=ph.positions, p=ph.momenta, code=ex.code, t=ex.t, eq=ex.q, ep=ex.p), want)
    i = int(np.nonzero(want["code"] >= 0)[0][0])
    ph, ex = api.exitSteps(R.DT, N, s, api.Phase(q[:, i], p[:, i]), gates)                        # one trajectory
    assert ph.positions.shape == (2,) and np.array_equal(ph.positions, want["q"][:, i]) and ex.q.shape == (2,)
    assert np.array_equal(ex.q, want["eq"][:, i]) and ex.t == want["t"][i] and ex.code == want["code"][i]
