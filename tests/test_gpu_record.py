"""GPU: hamk_record_steps through the C ABI of libhamk.so -- the companion module's kernel as the GPU compiler built it -- against the
oracle's RK4 and hamiltonian, the numpy restatement of the scheme and the oscillator's closed form (all from tests/test_record.py),
plus what only the real launch can show: bit-reproducibility, independence of B and of how a run is cut into calls, the host's
staging of exactly the rows a call fills, host arrays against device arrays, hamk_observe_batch on the recorded rows, the Python
binding on device tensors.  B = 257: four wavefronts and one lane, so the block edge at 256 is covered; at most 400 steps."""
import ctypes

import numpy as np
import pytest

import test_record as R                      # the restatement, the anchor, the inputs, the bounds and the properties live in the CPU test module
from hamilton_amd import examples as E
from test_gpu_exit import DeviceArrays

pytestmark = pytest.mark.gpu

B = R.B
HOST, DEVICE = 0, 1


@pytest.fixture(scope="module")
def lib(hamk_lib):
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return hamk_lib


def steps(lib, s, q, p, dt, nsteps, every, max_rows, step0=0, bufs=None, fill=0.0, states=True, energy=True, status=True, rows=None, mem=HOST):
    """One hamk_record_steps call on copies -> a dict like test_record.restate's (the arguments of test_record.emu_steps); mem = DEVICE
    goes through hamk_device_malloc'ed arrays and is synchronised before the copy back."""
    from hamilton_amd import _abi
    q, p = (np.ascontiguousarray(a, dtype=np.float64).copy() for a in (q, p))
    n, nb = q.shape
    b = R.new_bufs(n, nb, max_rows if rows is None else rows, fill, states, energy) if bufs is None else \
        {k: None if v is None else np.array(v) for k, v in bufs.items()}
    st = np.full(nb, -1, np.int32) if status else None
    arrays = (q, p, b["qout"], b["pout"], b["hout"], st)
    ptr = lambda a: None if a is None else a.ctypes.data
    if mem == HOST:
        _abi.check(lib.hamk_record_steps(s._h, nb, ptr(q), ptr(p), dt, int(nsteps), int(every), int(max_rows), ptr(b["qout"]), ptr(b["pout"]),
                                         ptr(b["hout"]), int(step0), ptr(st), HOST))
    else:
        d = DeviceArrays(lib, arrays)
        try:
            d.put()
            _abi.check(lib.hamk_set_stream(s._h, None))
            _abi.check(lib.hamk_record_steps(s._h, nb, d.dev[0], d.dev[1], dt, int(nsteps), int(every), int(max_rows), *d.dev[2:5], int(step0), d.dev[5], DEVICE))
            _abi.check(lib.hamk_synchronize(s._h))
            d.get()
        finally:
            d.free()
    return dict(q=q, p=p, status=st, **b)


_systems = {}


def system(name):
    """One handle per system for the whole module: the companion module is built and loaded once."""
    from hamilton_amd import api
    if name not in _systems:
        _systems[name] = api.system_from_spec(E.get(name))
    return _systems[name]


# ---------------------------------------------------------------------------------------------------------------------- anchor
@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("case", R.ANCHOR_CASES, ids=lambda c: "dt%g-n%d-every%d-rows%d" % c)
def test_oscillator_anchor(lib, case, mem):
    """Row k is the (k every)-th power of the RK4 matrix applied to the start; H of row k is H0 (a^2 + b^2)^(k every)."""
    dt, nsteps, every, max_rows = case
    q, p = R.osc_inputs(B)
    got = steps(lib, R.anchor_system("oscillator"), q, p, dt, nsteps, every, max_rows, fill=R.PAYLOAD, mem=mem)
    R.check_oscillator(got, case, "MI355X", B)


# ---------------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("name", R.SYSTEMS)
def test_against_the_oracle(lib, oracle_lib, name, mem):
    """Every state row within STATE_BOUND of the oracle's rk4_steps_batch at that row's step count, row 0 the input bit for bit,
    every hout row within 1e-11 of the oracle's hamiltonian of the recorded row, all 257 lanes; row 7 untouched.  Measured on an
    MI355X: DESIGN.md section 15."""
    ref = R.reference(oracle_lib, name)
    got = steps(lib, system(name), ref["q"], ref["p"], R.DT, R.NSTEPS, R.EVERY, R.MAX_ROWS, fill=R.PAYLOAD, mem=mem)
    R.check_against_reference(ref, name, got, "MI355X " + ("host arrays" if mem == HOST else "device arrays"))


@pytest.mark.parametrize("name", R.SYSTEMS)
def test_hout_against_observe_batch(lib, oracle_lib, name):
    """hout's rows against hamk_observe_batch applied to the recorded rows: the same formula through different device code (another
    kernel of another module), so the bound is the 1e-11 relative to max(1, |H|) of the oracle comparison, not equality."""
    from hamilton_amd import api
    ref = R.reference(oracle_lib, name)
    s = system(name)
    got = steps(lib, s, ref["q"], ref["p"], R.DT, R.NSTEPS, R.EVERY, R.MAX_ROWS)
    worst = max(R.relerr(got["hout"][k], api.hamiltonian(s, api.Phase(got["qout"][k], got["pout"][k]))) for k in range(R.FILLED))
    print("MI355X", name, "hout vs hamk_observe_batch on the recorded rows", worst, "bound", R.H_BOUND)
    assert worst <= R.H_BOUND, (name, worst)


# ---------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize("mem", [HOST, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("name", ["doublePendulum", "chain8"])
def test_properties(lib, oracle_lib, name, mem):
    """test_record.run_properties on the real launch (prefix, cut invariance, independence of every / max_rows / the outputs given,
    guard rows, rows of an earlier call, status = NULL) -- through host arrays it is also the staging's rule that rows outside the
    call's range keep their bits -- and: two identical calls agree bitwise; lanes 0 .. 63 stepped alone (B = 64) are the same lanes
    of the B = 257 call; host arrays equal device arrays."""
    ref = R.reference(oracle_lib, name)
    s = system(name)
    run = lambda q, p, nsteps, every, max_rows, **kw: steps(lib, s, q, p, R.DT, nsteps, every, max_rows, mem=mem, **kw)
    one = R.run_properties(run, ref, name)
    q, p = ref["q"], ref["p"]
    both = R.OUT + ("status",)
    assert R.same(one, run(q, p, R.NSTEPS, R.EVERY, R.MAX_ROWS, fill=R.PAYLOAD), both)
    other = steps(lib, s, q, p, R.DT, R.NSTEPS, R.EVERY, R.MAX_ROWS, fill=R.PAYLOAD, mem=DEVICE if mem == HOST else HOST)
    assert R.same(one, other, both)
    few = run(q[:, :64], p[:, :64], R.NSTEPS, R.EVERY, R.MAX_ROWS, fill=R.PAYLOAD)
    assert R.same(few, R.lanes(one, slice(0, 64)), both)


def test_long_run_in_pieces(lib, oracle_lib):
    """400 steps, every = 7, 30 rows of room (58 would be filled): one call against calls of 1, 6, 7, 8, 93 and 285 steps, buffers and
    step0 carried, on host arrays whose unfilled rows hold a payload: bitwise equal, rows 30 .. dropped."""
    ref = R.reference(oracle_lib, "doublePendulum")
    s = system("doublePendulum")
    q, p = ref["q"], ref["p"]
    one = steps(lib, s, q, p, R.DT, 400, 7, 30, fill=R.PAYLOAD, rows=31)
    assert not np.isnan(one["hout"][:30]).any() and np.isnan(one["hout"][30]).all() and np.isnan(one["qout"][30]).all()
    cur, done = dict(q=q, p=p, **R.new_bufs(2, B, 31, R.PAYLOAD)), 0
    for n in (1, 6, 7, 8, 93, 285):
        cur = steps(lib, s, cur["q"], cur["p"], R.DT, n, 7, 30, step0=done, bufs=R.carry(cur))
        done += n
    assert done == 400 and R.same(one, cur)


def test_a_nan_lane_and_a_singular_lane(lib, oracle_lib):
    """A NaN is an ordinary value to this kernel: that lane is flagged HAMK_ST_NONFINITE, the call is HAMK_OK (steps() checks the
    return code), the other 256 lanes hold the bits of a run without it; twoBody at r = 0 is flagged HAMK_ST_SINGULAR."""
    ref = R.reference(oracle_lib, "doublePendulum")
    s = system("doublePendulum")
    R.run_nan_lane(lambda q, p, nsteps, every, max_rows, **kw: steps(lib, s, q, p, R.DT, nsteps, every, max_rows, **kw), ref, 37)
    s2 = system("twoBody")
    R.run_singular_lane(lambda q, p, nsteps, every, max_rows, **kw: steps(lib, s2, q, p, R.DT, nsteps, every, max_rows, **kw), oracle_lib)


# ---------------------------------------------------------------------------------------------------------------------- binding
def test_python_binding(lib, oracle_lib):
    """api.recordSteps: torch device tensors equal the ABI call, out of place, continued from the returned Record, and in place; numpy
    arrays; max_rows = None; one reference-shaped trajectory."""
    import torch
    from hamilton_amd import api
    ref = R.reference(oracle_lib, "doublePendulum")
    s = system("doublePendulum")
    q, p = ref["q"], ref["p"]
    N, every, rows = R.NSTEPS, R.EVERY, R.MAX_ROWS
    want = steps(lib, s, q, p, R.DT, N, every, rows)
    n1 = 7
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    host = lambda x: dict(qout=x.positions.cpu().numpy(), pout=x.momenta.cpu().numpy(), hout=x.energy.cpu().numpy())
    tq, tp = cu(q), cu(p)
    ph, rec = api.recordSteps(R.DT, N, every, s, api.Phase(tq, tp), max_rows=rows, energy=True)
    got = dict(q=ph.positions.cpu().numpy(), p=ph.momenta.cpu().numpy(), **host(rec))
    assert R.same(got, want) and np.array_equal(s.last_status.cpu().numpy(), want["status"]) and rec.rows == R.FILLED
    assert rec.positions.shape == (rows, 2, B) and rec.energy.shape == (rows, B) and np.array_equal(tq.cpu().numpy(), q)      # out of place
    ph1, r1 = api.recordSteps(R.DT, n1, every, s, api.Phase(tq, tp), max_rows=rows, energy=True)                              # N1 + N2, the Record passed back
    before = host(r1)
    assert r1.rows == 3
    ph2, r2 = api.recordSteps(R.DT, N - n1, every, s, ph1, record=r1, step0=n1)
    assert R.same(dict(q=ph2.positions.cpu().numpy(), p=ph2.momenta.cpu().numpy(), **host(r2)), want) and r2.rows == R.FILLED
    assert R.same(host(r1), before, ("qout", "pout", "hout"))                                     # ... which was not advanced in place
    ph3, r3 = api.recordSteps(R.DT, N - n1, every, s, ph1, record=r1, step0=n1, inplace=True)
    assert ph3.positions.data_ptr() == ph1.positions.data_ptr() and r3.positions.data_ptr() == r1.positions.data_ptr()
    assert r3.energy.data_ptr() == r1.energy.data_ptr() and r3.rows == R.FILLED
    assert R.same(dict(q=ph1.positions.cpu().numpy(), p=ph1.momenta.cpu().numpy(), **host(r1)), want)
    ph, rec = api.recordSteps(R.DT, N, every, s, api.Phase(q, p), energy=True)                    # numpy arrays; exactly the rows the run fills
    assert rec.positions.shape == (R.FILLED, 2, B) and rec.rows == R.FILLED
    assert R.same(dict(q=ph.positions, p=ph.momenta, qout=rec.positions, pout=rec.momenta, hout=rec.energy),
                  dict(want, **{k: want[k][:R.FILLED] for k in ("qout", "pout", "hout")}))
    ph, rec = api.recordSteps(R.DT, N, every, s, api.Phase(tq, tp), states=False, energy=True)    # the energy curve alone
    assert rec.positions is None and rec.momenta is None and np.array_equal(R.bits(rec.energy.cpu().numpy()), R.bits(want["hout"][:R.FILLED]))
    ph, rec = api.recordSteps(R.DT, N, every, s, api.Phase(q[:, 5], p[:, 5]), energy=True)        # one trajectory
    assert ph.positions.shape == (2,) and np.array_equal(ph.positions, want["q"][:, 5])
    assert rec.positions.shape == (R.FILLED, 2) and rec.energy.shape == (R.FILLED,)
    assert np.array_equal(rec.positions, want["qout"][:R.FILLED, :, 5]) and np.array_equal(rec.energy, want["hout"][:R.FILLED, 5])
