"""The stepping loop's constants in vector registers (HAMK_STEP_CONST_VGPR, hamk_device.hpp StepK; hamk_options::step_const_vgpr) move
no bit: every system that rotates its sincos pairs is built with the define on and off, steps the same ensemble, and positions, momenta
and status must be EQUAL as integers on every lane -- healthy lanes, lanes beyond each rotation range (they re-evaluate through the
table), an angle beyond the table's range (library path), a NaN lane, and for the double pendulum of mixed inertias the lanes whose K is
not positive definite (LU fallback)."""
import numpy as np
import pytest

from hamilton_amd import examples as E

pytestmark = pytest.mark.gpu

B = 193            # no multiple of 64 or 256: the last wavefront and the last block are partial
STEPS = 25
# dt per system, so that the sampled ensemble straddles the stage-3 rotation range by itself: dt^2 / 4 |qdd| crosses 1/32 inside the
# sample's range of accelerations (checked below with the oracle); the stage-2 / stage-4 range is crossed by lanes placed at 1/8
DT = {"doublePendulum": 0.25, "doublePendulum~mixed": 0.25, "pendulum": 0.5, "threeBodyPolar": 0.25, "chain4": 0.05}
SYSTEMS = list(DT)


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    return _api


def ensemble(api, oracle_lib, name):
    """(q, p) with the lanes that take each guard placed next to lanes that do not; checked with the CPU oracle's right-hand side."""
    spec = E.get(name)
    o = oracle_lib.OracleSystem(spec)
    n, dt = spec.n, DT[name]
    q, qd = E.sample_config(spec, 11, B)
    q, qd = np.ascontiguousarray(q), np.ascontiguousarray(qd)
    # stage 2 / stage 4 rotation range: |qd_0| dt / 2 just under and just over 1/8, neighbours of ordinary lanes
    qd[0, 7], qd[0, 8] = (0.125 - 1e-6) * 2 / dt, (0.125 + 1e-6) * 2 / dt
    qd[0, 70], qd[0, 71] = -(0.125 - 1e-9) * 2 / dt, -(0.125 + 1e-9) * 2 / dt
    qd[:, 100] = 0.0                                           # a lane that starts at rest: inside every range
    qd[:, 130] = 8.0 / dt                                      # far beyond every range, stage 3 included
    p = np.ascontiguousarray(o.to_phase_batch(q, qd))
    # what the first step's stages see (oracle): delta_2 = dt/2 |dq(y)|, delta_3 = dt/2 |dq(y + dt/2 k1) - dq(y)|
    dq0, dp0, _ = o.hameqs_batch(q, p)
    dq1, _, _ = o.hameqs_batch(q + 0.5 * dt * dq0, p + 0.5 * dt * dp0)
    d2 = 0.5 * dt * np.abs(dq0).max(0)
    d3 = 0.5 * dt * np.abs(dq1 - dq0).max(0)
    assert (d2 < 0.125).any() and (d2 > 0.125).any(), name
    assert (d3 < 0.03125).any() and (d3 > 0.03125).any(), name
    q[0, 33] = 1.7e6                                           # beyond the table's range: library sincos
    q[n - 1, 150] = -2.5e6
    q[0, 55] = np.nan                                          # a NaN lane between healthy ones
    p[n - 1, 160] = np.inf
    return spec, dt, q, p


@pytest.mark.parametrize("name", SYSTEMS)
def test_parked_constants_do_not_move_a_bit(api, oracle_lib, name):
    from hamilton_amd import _abi
    spec, dt, q, p = ensemble(api, oracle_lib, name)
    if name.endswith("~mixed"):                                # some lanes must meet a K that is not positive definite
        o = oracle_lib.OracleSystem(spec)
        ok = [i for i in range(B) if np.isfinite(q[:, i]).all()]
        eig = [np.linalg.eigvalsh(o.jacobian(q[:, i]).T @ np.diag(spec.inertia) @ o.jacobian(q[:, i])).min() for i in ok]
        assert min(eig) < 0.0
    out = {}
    for tag, opt in (("on", _abi.ON), ("off", _abi.OFF)):
        # (chain4 takes every sincos through the table by the library's rule and has nothing to park: here with one table evaluation per
        # step and rotations, the configuration in which it runs rotate_pair -- in both builds)
        trig = _abi.TRIG_TABLE_ROTATE if name == "chain4" else _abi.AUTO
        s = api.system_from_spec(spec, _abi.HamkOptions(step_const_vgpr=opt, mapping=_abi.MAP_LANE, trig=trig))
        assert ("#define HAMK_STEP_CONST_VGPR 1" in s.source) == (tag == "on"), (name, tag)   # the two builds differ in the define
        assert s.options(B)["step_const_vgpr"] == opt
        ph = api.rk4Steps(dt, STEPS, s, api.Phase(q.copy(), p.copy()), drift_tol=1e-3)
        out[tag] = (np.ascontiguousarray(np.asarray(ph.positions)), np.ascontiguousarray(np.asarray(ph.momenta)),
                    np.ascontiguousarray(np.asarray(s.last_status)))
    assert out["on"][0].shape == (spec.n, B)
    np.testing.assert_array_equal(out["on"][0].view(np.int64), out["off"][0].view(np.int64))
    np.testing.assert_array_equal(out["on"][1].view(np.int64), out["off"][1].view(np.int64))
    np.testing.assert_array_equal(out["on"][2].astype(np.int32), out["off"][2].astype(np.int32))
    assert (out["on"][2][[55, 160]] != 0).all(), name         # the NaN and the Inf lane are flagged
