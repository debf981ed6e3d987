"""GPU: rectangular coordinate maps (m != n) through the C ABI -- every member of tests/rect_family.py (one per branch a kernel takes on
m against a size derived from n; the table is in that module) with the mapping its table asks for, at B = 193: no multiple of 64, 16, 4
or 2, so the last wavefront, the last group of quads and the last pair of wave trajectories are partial.

Against the 50-digit fixtures of tests/golden/rect_family.json (1e-12 max(1, cond_hint / 1e3), as tests/test_gpu_parity.py T1) and, on
every one of the 193 trajectories, against the oracle: hamEqs, velocities, the energies, three RK4 steps at the member's dt and one
stepHam(0.1) with the oracle's sub-step counts; no status bit set anywhere.  The bound against the oracle is the one of
tests/test_rect_family.py: 1e-11 (lane kernels) or 1e-10 (the cooperative mappings) times max(1, cond K / 100) per trajectory, ten times
that after the RK4 steps, a hundred times after stepHam.

qd_eq, qd_first_gu and qd_last -- the members on the V / GU boundary of the dense four-lane path -- also run with MAP_WAVE: both mappings
agree with the oracle within that bound and with each other within the same bound."""
import json
import os

import numpy as np
import pytest

import rect_family as F
from conftest import GOLDEN, fvec
from hamilton_amd import examples as E

pytestmark = pytest.mark.gpu

B = 193
DT_HAM = 0.1
MARKER = {"lane": "HAMK_INSTANTIATE(HamkSys)", "quad": "HAMK_INSTANTIATE_QUAD", "wave": "HAMK_INSTANTIATE_WAVE"}
RUN_IDS = [f"{key}-{ask or 'auto'}" for key, ask in F.GPU_RUNS]


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _api


@pytest.fixture(scope="module")
def family():
    with open(os.path.join(GOLDEN, "rect_family.json")) as fh:
        return json.load(fh)["blocks"]


@pytest.fixture(scope="module")
def truth(oracle_lib):
    """The oracle's side of one member, computed once and shared by its builds (read only)."""
    cache = {}

    def get(key):
        if key not in cache:
            spec = F.spec(key)
            o = oracle_lib.OracleSystem(spec)
            q, qd = E.sample_config(spec, 2024, B)
            p = o.to_phase_batch(q, qd)
            odq, odp, ost = o.hameqs_batch(q, p)
            assert not ost.any()
            cond = np.array([np.linalg.cond(o.jacobian(q[:, i]).T @ np.diag(spec.inertia) @ o.jacobian(q[:, i])) for i in range(B)])
            assert cond.max() < F.COND_LIMIT, (key, cond.max())
            t = dict(q=q, p=p, dq=odq, dp=odp, vel=o.from_phase_batch(q, p)[0], obs=o.observe_batch(q, p),
                     rk4=o.rk4_steps_batch(q, p, spec.dt, 3), ham=o.step_ham_batch(q, p, DT_HAM), scale=np.maximum(1.0, cond / 100.0))
            for v in (q, p, odq, odp, t["vel"], t["scale"]) + tuple(t["obs"]) + tuple(t["rk4"]) + tuple(t["ham"]):
                v.setflags(write=False)
            cache[key] = t
        return cache[key]
    return get


def golden_points(api, s, key, pts):
    q = np.stack([fvec(pt["q"]) for pt in pts], axis=1)
    qd = np.stack([fvec(pt["vel"]) for pt in pts], axis=1)         # (`vel` is also the qd of toPhase and the dq of hamEqs: rect_family.json)
    p = np.stack([fvec(pt["p"]) for pt in pts], axis=1)
    tol = 1e-12 * np.maximum(1.0, np.array([float(pt["cond_hint"]) for pt in pts]) / 1e3)

    def close(got, name):
        want = np.stack([fvec(pt[name]) for pt in pts], axis=-1) if isinstance(pts[0][name], list) else np.array([float(pt[name]) for pt in pts])
        err = np.abs(np.asarray(got) - want) / np.maximum(1.0, np.abs(want))
        print(f" {name} {float(np.max(err / tol)):.2f}", end="")
        assert np.all(err <= tol), (key, name, float(np.max(err / tol)))

    close(api.momenta(s, api.Config(q, qd)), "p")
    close(api.velocities(s, api.Phase(q, p)), "vel")
    close(api.keP(s, api.Phase(q, p)), "keP")
    close(api.pe(s, q), "pe")
    close(api.hamiltonian(s, api.Phase(q, p)), "hamiltonian")
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    assert not np.any(s.last_status)
    close(dq, "vel")
    close(dp, "dp")


def per_lane(got, want, ref=None):
    """max over the components of |got - want| / max(1, max |ref|), trajectory by trajectory."""
    ref = want if ref is None else ref
    return np.abs(np.asarray(got) - want).max(0) / np.maximum(1.0, np.abs(ref).max(0))


RESULTS = {}                                               # (key, mapping that ran) -> what the kernels gave, for the quad / wave comparison


@pytest.mark.parametrize("key,ask", F.GPU_RUNS, ids=RUN_IDS)
def test_member_through_the_abi(api, truth, family, key, ask):
    spec = F.spec(key)
    want = ask or F.runs_on(key)
    s = api.system_from_spec(spec, F.options(ask))
    assert s.options(B)["mapping"] == F.mapping_code(want) and MARKER[want] in s.describe_batch(B).source, (key, ask)
    assert ("QUAD_DENSE = true" in s.source) == (F.quad_dense(key) and want == "quad"), (key, ask)
    print(f"{key} {want}: golden", end="")
    golden_points(api, s, key, family[key]["points"])
    t = truth(key)
    q, p = t["q"], t["p"]
    tol = (1e-11 if want == "lane" else 1e-10) * t["scale"]
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    assert not np.any(s.last_status)
    e = np.maximum(per_lane(dq, t["dq"]), per_lane(dp, t["dp"]))
    print(f" | oracle hamEqs {float(np.max(e / tol)):.3f}", end="")
    assert np.all(e <= tol), (key, ask, float(np.max(e / tol)))
    v = api.velocities(s, api.Phase(q, p))
    assert not np.any(s.last_status) and np.all(per_lane(v, t["vel"]) <= tol), (key, ask)
    oke, ope, oh = t["obs"]
    h = np.asarray(api.hamiltonian(s, api.Phase(q, p)))
    assert np.all(np.abs(h - oh) / np.maximum(1.0, np.abs(oh)) <= tol), (key, ask)
    assert np.all(np.abs(np.asarray(api.pe(s, q)) - ope) / np.maximum(1.0, np.abs(ope)) <= tol), (key, ask)
    assert np.all(np.abs(np.asarray(api.keP(s, api.Phase(q, p))) - oke) / np.maximum(1.0, np.abs(oke)) <= tol), (key, ask)
    ph = api.rk4Steps(spec.dt, 3, s, api.Phase(q, p))
    assert not np.any(s.last_status)
    oq, op = t["rk4"]
    e = np.maximum(per_lane(ph.positions, oq, op), per_lane(ph.momenta, op))
    print(f" rk4 {float(np.max(e / (10 * tol))):.3f}", end="")
    assert np.all(e <= 10 * tol), (key, ask, float(np.max(e / (10 * tol))))
    st = api.stepHam(DT_HAM, s, api.Phase(q, p))
    assert not np.any(s.last_status)
    sq, sp, sns = t["ham"]
    assert np.array_equal(np.asarray(s.last_nsub), sns), (key, ask, np.asarray(s.last_nsub)[:8], sns[:8])
    e = np.maximum(per_lane(st.positions, sq, sp), per_lane(st.momenta, sp))
    print(f" stepHam {float(np.max(e / (100 * tol))):.3f}")
    assert np.all(e <= 100 * tol), (key, ask, float(np.max(e / (100 * tol))))
    RESULTS[(key, want)] = dict(dq=np.asarray(dq).copy(), dp=np.asarray(dp).copy(), q3=np.asarray(ph.positions).copy(), p3=np.asarray(ph.momenta).copy(),
                                qh=np.asarray(st.positions).copy(), ph=np.asarray(st.momenta).copy())


@pytest.mark.parametrize("key", F.QUAD_AND_WAVE)
def test_quad_and_wave_mappings_agree(truth, key):
    """The two mappings of the members on the V / GU boundary against each other, within the bound each holds against the oracle (the
    results of test_member_through_the_abi above, which has run both: a missing result is a failure, not a skip)."""
    assert (key, "quad") in RESULTS and (key, "wave") in RESULTS, f"{key}: test_member_through_the_abi must have passed on both mappings first"
    a, b, t = RESULTS[(key, "quad")], RESULTS[(key, "wave")], truth(key)
    tol = 1e-10 * t["scale"]
    assert np.all(np.maximum(per_lane(a["dq"], b["dq"]), per_lane(a["dp"], b["dp"])) <= tol), key
    assert np.all(np.maximum(per_lane(a["q3"], b["q3"], b["p3"]), per_lane(a["p3"], b["p3"])) <= 10 * tol), key
    assert np.all(np.maximum(per_lane(a["qh"], b["qh"], b["ph"]), per_lane(a["ph"], b["ph"])) <= 100 * tol), key
