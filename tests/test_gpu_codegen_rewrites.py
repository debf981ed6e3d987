"""GPU: the generator's per-node rewrites -- shared exponentials, the fused 1 / sqrt, the sincos slots -- through the C ABI.  Every member
of tests/rewrite_family.py (one per branch; see there) runs on the default build, on the reverse sweep (AD_R) and on the four-lane and
wave mappings forced through the ABI's options: against the 50-digit fixtures of tests/golden/rewrite_family.json at the golden rule
T1 max(1, cond / 1e3), and on an ensemble of 257 against the oracle, which evaluates the tape as written (hamEqs and three RK4 steps
to 1e-11, stepHam to 1e-10 with the oracle's sub-step counts on at least 0.99 of the trajectories: the tolerances of
tests/test_gpu_symbolic_rhs.py).  No point and no trajectory is left out, and no status bit may be set: the range members hold
exponentials at the edge of fp64's range whose VALUES are in range as the tape writes them."""
import json
import os

import numpy as np
import pytest

import rewrite_family as F
from conftest import GOLDEN
from hamilton_amd import examples as E
from test_codegen_rewrites import check_promise
from test_gpu_parity import check_golden_points, relerr

pytestmark = pytest.mark.gpu

B = 257
DT_HAM = 0.02
MARKER = {"default": "HAMK_INSTANTIATE(HamkSys)", "R": "MODE_R = true", "quad": "HAMK_INSTANTIATE_QUAD", "wave": "HAMK_INSTANTIATE_WAVE"}


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _api


@pytest.fixture(scope="module")
def family():
    with open(os.path.join(GOLDEN, "rewrite_family.json")) as fh:
        return json.load(fh)["blocks"]


@pytest.fixture(scope="module")
def truth(oracle_lib):
    """The oracle's side of one member, computed once and shared by its four builds (read only)."""
    cache = {}

    def get(key):
        if key not in cache:
            spec = F.spec(key)
            o = oracle_lib.OracleSystem(spec)
            q, qd = E.sample_config(spec, 2024, B)
            p = o.to_phase_batch(q, qd)
            odq, odp, ost = o.hameqs_batch(q, p)
            assert not ost.any()
            cache[key] = dict(q=q, p=p, dq=odq, dp=odp, rk4=o.rk4_steps_batch(q, p, spec.dt, 3), ham=o.step_ham_batch(q, p, DT_HAM))
            for v in (q, p, odq, odp) + tuple(cache[key]["rk4"]) + tuple(cache[key]["ham"]):
                v.setflags(write=False)
        return cache[key]
    return get


@pytest.mark.parametrize("variant", F.GPU_VARIANTS)
@pytest.mark.parametrize("key", F.KEYS)
def test_family_through_the_abi(api, truth, family, key, variant):
    spec = F.spec(key)
    s = api.system_from_spec(spec, F.gpu_options(variant))
    assert MARKER[variant] in s.source, (key, variant)
    check_promise(key, s.source)
    check_golden_points(api, s, spec.name, pts=family[key]["points"])
    t = truth(key)
    q, p = t["q"], t["p"]
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    assert not np.any(s.last_status)
    print(f"{key} {variant}: hamEqs {relerr(dq, t['dq']):.2e} {relerr(dp, t['dp']):.2e}", end="")
    assert relerr(dq, t["dq"]) < 1e-11 and relerr(dp, t["dp"]) < 1e-11, (key, variant, relerr(dq, t["dq"]), relerr(dp, t["dp"]))
    ph = api.rk4Steps(spec.dt, 3, s, api.Phase(q, p))
    assert not np.any(s.last_status)
    oq, op = t["rk4"]
    print(f" rk4 {relerr(ph.positions, oq):.2e} {relerr(ph.momenta, op):.2e}", end="")
    assert relerr(ph.positions, oq) < 1e-11 and relerr(ph.momenta, op) < 1e-11, (key, variant)
    st = api.stepHam(DT_HAM, s, api.Phase(q, p))
    assert not np.any(s.last_status)
    sq, sp, sns = t["ham"]
    same = np.asarray(s.last_nsub) == sns
    print(f" stepHam same {same.mean():.3f} {relerr(np.asarray(st.positions)[:, same], sq[:, same]):.2e}")
    assert same.mean() >= 0.99, (key, variant, same.mean())
    assert relerr(np.asarray(st.positions)[:, same], sq[:, same]) < 1e-10 and relerr(np.asarray(st.momenta)[:, same], sp[:, same]) < 1e-10, (key, variant)
