"""GPU: the symbolic right-hand side and the jets it replaces, side by side.  Every member of tests/symbolic_family.py and the four
headline systems are built twice -- the default and HAMK_K_SYMBOLIC=0, flags asserted from the source -- and both builds go against
the 50-digit fixtures (tests/golden/symbolic_family.json; the named systems: their by-hand fixtures, threeBodyPolar its derived
ones), against the oracle on an ensemble of 257 (three RK4 steps, stepHam with the oracle's sub-step counts) and against each
other.  No trajectory and no fixture point is left out (the family was selected by the reference's cond K < 1e4) and no status bit
may be set."""
import json
import os

import numpy as np
import pytest

import symbolic_family as F
from conftest import GOLDEN, fvec, load_golden
from hamilton_amd import examples as E
from symbolic_text import flags
from test_gpu_parity import T1, check_golden_points, relerr

pytestmark = pytest.mark.gpu

NAMED = {"doublePendulum": "byhand:doublePendulum", "twoBody": "byhand:twoBody", "spring": "byhand:spring", "threeBodyPolar": "threeBodyPolar"}
NAMED_FLAGS = {"doublePendulum": "111", "twoBody": "110", "spring": "110", "threeBodyPolar": "110"}


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _api


@pytest.fixture(scope="module")
def family():
    with open(os.path.join(GOLDEN, "symbolic_family.json")) as fh:
        return json.load(fh)["blocks"]


def both_builds(api, monkeypatch, spec, promised):
    out = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("HAMK_K_SYMBOLIC", "0")
        else:
            monkeypatch.delenv("HAMK_K_SYMBOLIC", raising=False)
        s = api.system_from_spec(spec)
        assert flags(s.source) == ("000" if off else promised), (spec.name, off, flags(s.source))
        out.append(s)
    monkeypatch.delenv("HAMK_K_SYMBOLIC", raising=False)
    return out


def run_both(api, oracle_lib, monkeypatch, spec, promised, pts, golden_name, dt_ham):
    o = oracle_lib.OracleSystem(spec)
    builds = both_builds(api, monkeypatch, spec, promised)
    # fixtures: hamEqs, momenta, hamiltonian (and the rest of the surface) at test_gpu_parity's golden rule T1 max(1, cond / 1e3)
    gq = np.stack([fvec(p["q"]) for p in pts], axis=1)
    gp = np.stack([fvec(p["p"]) for p in pts], axis=1)
    tol = T1 * np.maximum(1.0, np.array([max(1.0, float(pt["cond_hint"])) for pt in pts]) / 1e3)
    at_fixture = []
    for s in builds:
        check_golden_points(api, s, golden_name, pts=pts)
        dq, dp = api.hamEqs(s, api.Phase(gq, gp))
        assert not np.any(s.last_status)
        at_fixture.append((np.asarray(dq), np.asarray(dp)))
    for x, y in zip(*at_fixture):                          # both within tol of one truth: within 2 tol of each other
        scale = np.maximum(1.0, np.maximum(np.abs(x).max(0), np.abs(y).max(0)))
        assert np.all(np.abs(x - y).max(0) / scale <= 2 * tol), (spec.name, float(np.max(np.abs(x - y).max(0) / scale / tol)))
    # ensemble against the oracle
    B = 257
    q, qd = E.sample_config(spec, 2024, B)
    p = o.to_phase_batch(q, qd)
    odq, odp, ost = o.hameqs_batch(q, p)
    assert not ost.any()
    oq, op = o.rk4_steps_batch(q, p, spec.dt, 3)
    sq, sp, sns = o.step_ham_batch(q, p, dt_ham)
    ens = []
    for s in builds:
        dq, dp = api.hamEqs(s, api.Phase(q, p))
        assert not np.any(s.last_status)
        assert relerr(dq, odq) < 1e-11 and relerr(dp, odp) < 1e-11, (spec.name, relerr(dq, odq), relerr(dp, odp))
        ens.append((np.asarray(dq), np.asarray(dp)))
        ph = api.rk4Steps(spec.dt, 3, s, api.Phase(q, p))
        assert not np.any(s.last_status)
        assert relerr(ph.positions, oq) < 1e-11 and relerr(ph.momenta, op) < 1e-11, spec.name
        st = api.stepHam(dt_ham, s, api.Phase(q, p))
        assert not np.any(s.last_status)
        same = np.asarray(s.last_nsub) == sns               # identical accept / reject sequence wherever the oracle's decision is unambiguous
        assert same.mean() >= 0.99, (spec.name, same.mean())
        assert relerr(np.asarray(st.positions)[:, same], sq[:, same]) < 1e-10 and relerr(np.asarray(st.momenta)[:, same], sp[:, same]) < 1e-10, spec.name
    assert relerr(ens[0][0], ens[1][0]) < 2e-11 and relerr(ens[0][1], ens[1][1]) < 2e-11, spec.name


@pytest.mark.parametrize("seed", F.SEEDS)
def test_family_symbolic_and_jet_builds(api, oracle_lib, monkeypatch, family, seed):
    spec = F.spec(seed)
    run_both(api, oracle_lib, monkeypatch, spec, F.PROMISE[seed], family[str(seed)]["points"], spec.name, 0.02)


@pytest.mark.parametrize("name", sorted(NAMED))
def test_headline_systems_symbolic_and_jet_builds(api, oracle_lib, monkeypatch, name):
    """BASELINE configs 1-4: the jets under HAMK_K_SYMBOLIC=0 are what these systems ran on before the symbolic right-hand side; no
    default build runs them any more."""
    spec = E.get(name)
    run_both(api, oracle_lib, monkeypatch, spec, NAMED_FLAGS[name], load_golden(NAMED[name])["points"], NAMED[name], 0.01)
