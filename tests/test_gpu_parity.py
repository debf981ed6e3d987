"""GPU: the HIP path (through the C ABI of libhamk.so) against the CPU oracle and the
golden fixtures.  Tolerance ladder of SURVEY.md section 8c:
  T1  state functions / hamEqs        <= 1e-12 * max(1,|y|) (scaled by cond(K) when ill-conditioned)
  T2  one RK4 step, GPU vs oracle     <= 1e-13 relative
  T3  N RK4 steps                     reported; bounded loosely (chaotic growth of roundoff)
  T4  RK4 vs stepHam (RKF45)          truncation level, 1-step <= 1e-8
The product path evaluates an algebraically equivalent form of Hamilton.hs:375-387 (solve
instead of inverse, contraction instead of the Hessian tensor, FMA contraction), so fp64
results agree to roundoff, not bitwise.
"""
import numpy as np
import pytest

from conftest import ALL_GOLDEN_SYSTEMS, BYHAND_SYSTEMS, CHAIN_GOLDEN_SYSTEMS, REFERENCE_SYSTEMS, fvec, load_golden
from hamilton_amd import examples as E

pytestmark = pytest.mark.gpu

T1 = 1e-12


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    if hamk_lib.hamk_device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests need a real MI355X")
    return _api


@pytest.fixture(scope="module")
def systems(api, oracle_lib):
    out = {}
    for name in ALL_GOLDEN_SYSTEMS:
        spec = E.get(name)
        out[name] = (spec, api.system_from_spec(spec), oracle_lib.OracleSystem(spec))
    return out


def relerr(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(1.0, np.abs(np.asarray(b)))))


# ---------------------------------------------------------------- T1: golden fixtures
def check_golden_points(api, s, name, pts=None):
    """`pts`: the points of one block of a fixture file that holds several systems (symbolic_family.json)."""
    pts = load_golden(name)["points"] if pts is None else pts
    q = np.stack([fvec(p["q"]) for p in pts], axis=1)
    qd = np.stack([fvec(p["qd"]) for p in pts], axis=1)
    p = np.stack([fvec(pt["p"]) for pt in pts], axis=1)
    cond = np.array([max(1.0, float(pt["cond_hint"])) for pt in pts])
    tol = T1 * np.maximum(1.0, cond / 1e3)

    def close(got, key, scale_rows=True):
        want = np.stack([fvec(pt[key]) for pt in pts], axis=-1) if isinstance(pts[0][key], list) \
            else np.array([float(pt[key]) for pt in pts])
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        assert np.all(err <= tol), (name, key, float(np.max(err / tol)))

    close(api.underlyingPos(s, q), "x")
    close(api.momenta(s, api.Config(q, qd)), "p")
    close(api.velocities(s, api.Phase(q, p)), "vel")
    close(api.keC(s, api.Config(q, qd)), "keC")
    close(api.keP(s, api.Phase(q, p)), "keP")
    close(api.pe(s, q), "pe")
    close(api.lagrangian(s, api.Config(q, qd)), "lagrangian")
    close(api.hamiltonian(s, api.Phase(q, p)), "hamiltonian")
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    close(dq, "dq")
    close(dp, "dp")
    assert not np.any(s.last_status)


@pytest.mark.parametrize("name", ALL_GOLDEN_SYSTEMS)
def test_golden_points(api, systems, name):
    spec, s, _ = systems[name]
    check_golden_points(api, s, name)


@pytest.mark.parametrize("name", BYHAND_SYSTEMS)
def test_by_hand_golden_points(api, name):
    """The reference's own systems against fixtures that share nothing with hamilton_amd/examples.py (hand-written mass matrix,
    potential and Hamilton's equations from app/Examples.hs / README.md at 50 digits, oracle/gen_golden_byhand.py) -- incl. the
    README's worked double pendulum (masses 1 1 2 2) at its config0."""
    check_golden_points(api, api.system_from_spec(E.get(name)), "byhand:" + name)


@pytest.mark.parametrize("mapping", ["default", "large-ensemble", "lane", "quad", "wave"])
@pytest.mark.parametrize("name", CHAIN_GOLDEN_SYSTEMS)
def test_chain_golden_points(api, name, mapping):
    """BASELINE config 5 (N = 8, 16, 32) against 50-digit fixtures that share NOTHING with the product or the oracle: the
    chain's closed-form mass matrix K[a][b] = l^2 (N - max(a, b)) cos(th_a - th_b) and Hamilton's equations written out by
    hand (oracle/gen_golden.py evaluate_chain_point; round 3 checked these sizes against the C oracle only, which reads the
    same tape).  On the mapping the library picks for a 13-point call, on the one it picks for the config's 65 536, and on
    every mapping forced through the ABI's options."""
    from hamilton_amd import _abi
    spec = E.get(name)
    if mapping == "lane" and spec.n > 16:
        pytest.skip("one trajectory per lane stops at n = 16")
    if mapping == "default":
        s = api.system_from_spec(spec)
    elif mapping == "large-ensemble":
        s = api.system_from_spec(spec, {"mapping": api.system_from_spec(spec).options(65536)["mapping"]})
    else:
        s = api.system_from_spec(spec, {"mapping": {"lane": _abi.MAP_LANE, "quad": _abi.MAP_QUAD, "wave": _abi.MAP_WAVE}[mapping]})
    check_golden_points(api, s, name)


# ---------------------------------------------------------------- T1: against the oracle on seeded ensembles
@pytest.mark.parametrize("name", ALL_GOLDEN_SYSTEMS)
def test_hameqs_vs_oracle_ensemble(api, systems, name):
    spec, s, o = systems[name]
    B = 1000                                   # deliberately not a multiple of the 256-lane block
    q, qd = E.sample_config(spec, 12345, B)
    p = api.momenta(s, api.Config(q, qd))
    assert relerr(p, o.to_phase_batch(q, qd)) < T1
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    odq, odp, ost = o.hameqs_batch(q, p)
    assert not ost.any() and not np.any(s.last_status)
    assert relerr(dq, odq) < 1e-11 and relerr(dp, odp) < 1e-11, (relerr(dq, odq), relerr(dp, odp))
    ke, pe_, h = o.observe_batch(q, p)
    assert relerr(api.keP(s, api.Phase(q, p)), ke) < 1e-11
    assert relerr(api.pe(s, q), pe_) < T1
    assert relerr(api.hamiltonian(s, api.Phase(q, p)), h) < 1e-11
    v, _ = o.from_phase_batch(q, p)
    assert relerr(api.velocities(s, api.Phase(q, p)), v) < 1e-11
    assert relerr(api.underlyingPos(s, q), o.coords_batch(q)) < T1


def test_abs_and_signum_opcodes(api, oracle_lib):
    """Opcodes 27 / 28 (Num.abs, Num.signum; no reference system uses them) on the GPU vs the oracle."""
    spec = E.get("absZoo")
    s, o = api.system_from_spec(spec), oracle_lib.OracleSystem(spec)
    q, qd = E.sample_config(spec, 7, 777)
    p = api.momenta(s, api.Config(q, qd))
    assert relerr(p, o.to_phase_batch(q, qd)) < T1
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    odq, odp, _ = o.hameqs_batch(q, p)
    assert relerr(dq, odq) < 1e-11 and relerr(dp, odp) < 1e-11 and not np.any(s.last_status)
    ph = api.rk4Steps(spec.dt, 5, s, api.Phase(q, p))
    oq, op = o.rk4_steps_batch(q, p, spec.dt, 5)
    assert relerr(ph.positions, oq) < 1e-12 and relerr(ph.momenta, op) < 1e-12
    st = api.stepHam(0.02, s, api.Phase(q, p))
    sq, sp, sns = o.step_ham_batch(q, p, 0.02)
    assert np.array_equal(np.asarray(s.last_nsub), sns) and relerr(st.positions, sq) < 1e-11


# ---------------------------------------------------------------- T2/T3: RK4
@pytest.mark.parametrize("name", REFERENCE_SYSTEMS + ["threeBodyPolar"])
def test_rk4_vs_oracle(api, systems, name):
    spec, s, o = systems[name]
    B = 300
    q, qd = E.sample_config(spec, 777, B)
    p = o.to_phase_batch(q, qd)
    one = api.rk4Steps(spec.dt, 1, s, api.Phase(q, p))
    oq, op = o.rk4_steps_batch(q, p, spec.dt, 1)
    assert relerr(one.positions, oq) < 1e-13 and relerr(one.momenta, op) < 1e-13            # T2
    many = api.rk4Steps(spec.dt, 100, s, api.Phase(q, p))
    oq, op = o.rk4_steps_batch(q, p, spec.dt, 100)
    err = max(relerr(many.positions, oq), relerr(many.momenta, op))
    assert err < 1e-8, (name, err)                                                            # T3 (bounded loosely)
    assert not np.any(s.last_status)


def test_rk4_matches_taylor_truth(api, systems):
    spec, s, _ = systems["doublePendulum"]
    tr = load_golden("doublePendulum")["trajectory"]
    q0, p0 = fvec(tr["q0"]), fvec(tr["p0"])
    for st in tr["states"]:
        n = int(round(float(st["t"]) / spec.dt))
        ph = api.rk4Steps(spec.dt, n, s, api.Phase(q0, p0))
        err = max(np.max(np.abs(ph.positions - fvec(st["q"]))), np.max(np.abs(ph.momenta - fvec(st["p"]))))
        assert err < 5e-6, (st["t"], err)


# ---------------------------------------------------------------- stepHam / evolveHam (GSL RKF45 semantics)
@pytest.mark.parametrize("name", REFERENCE_SYSTEMS)
def test_stepham_vs_oracle(api, systems, name):
    spec, s, o = systems[name]
    B = 200
    q, qd = E.sample_config(spec, 4242, B)
    p = o.to_phase_batch(q, qd)
    dt = 1.0 / 12.0                                    # the demo app's frame step (Examples.hs:415,429)
    ph = api.stepHam(dt, s, api.Phase(q, p))
    oq, op, ons = o.step_ham_batch(q, p, dt)
    nsub = np.asarray(s.last_nsub)
    same = nsub == ons                                  # identical accept/reject sequence
    # measured on MI355X: 100 % (profiles/r01_parity_report.jsonl); a controller threshold can flip on a roundoff tie
    assert same.mean() >= 0.99, (name, same.mean())
    assert np.abs(np.bincount(nsub, minlength=64) - np.bincount(ons, minlength=64)).sum() <= 2 * int((~same).sum())
    assert relerr(ph.positions[:, same], oq[:, same]) < 1e-10
    assert relerr(ph.momenta[:, same], op[:, same]) < 1e-10
    # lanes whose step sequence differs still agree to the integrator's tolerance
    assert relerr(ph.positions, oq) < 1e-6 and relerr(ph.momenta, op) < 1e-6
    assert not np.any(s.last_status)


def test_stepham_reference_initial_state(api, systems):
    """C1: doublePendulum 1 1 from seInit, one trajectory, stepHam 0.01: 4 sub-steps like the CPU path."""
    spec, s, o = systems["doublePendulum"]
    q0, p0 = np.array(spec.q0), np.zeros(2)
    ph = api.stepHam(0.01, s, api.Phase(q0, p0))
    oq, op = o.step_ham(0.01, q0, p0)
    assert int(np.asarray(s.last_nsub)[0]) == 4
    assert relerr(ph.positions, oq) < 1e-13 and relerr(ph.momenta, op) < 1e-13
    # 1000 x stepHam 0.01 (BASELINE config 1), GPU lane vs CPU oracle: chaotic growth of roundoff only
    q, p, oq, op = q0, p0, q0, p0
    for _ in range(100):
        ph = api.stepHam(0.01, s, api.Phase(q, p)); q, p = ph.positions, ph.momenta
        oq, op = o.step_ham(0.01, oq, op)
    assert relerr(q, oq) < 1e-9 and relerr(p, op) < 1e-9


def test_evolveham_rows(api, systems):
    spec, s, o = systems["spring"]
    B = 64
    q, qd = E.sample_config(spec, 99, B)
    p = o.to_phase_batch(q, qd)
    ts = np.array([0.0, 0.05, 0.1, 0.3, 0.31])
    rows = api.evolveHam(s, api.Phase(q, p), ts)
    assert len(rows) == len(ts)
    np.testing.assert_array_equal(rows[0].positions, q)      # row 0 = initial state (Hamilton.hs:443-462)
    np.testing.assert_array_equal(rows[0].momenta, p)
    oq, op, _ = o.evolve_ham_batch(q, p, ts)
    for r in range(1, len(ts)):
        assert relerr(rows[r].positions, oq[r]) < 1e-7 and relerr(rows[r].momenta, op[r]) < 1e-7
    # evolveHam' list front-end (Hamilton.hs:409-429)
    assert api.evolveHam_(s, api.Phase(q, p), []) == []
    one = api.evolveHam_(s, api.Phase(q, p), [0.05])
    assert len(one) == 1 and relerr(one[0].positions, oq[1]) < 1e-7
    # config-space wrappers (Hamilton.hs:470-515)
    c1 = api.stepHamC(0.05, s, api.Config(q, qd))
    v, _ = o.from_phase_batch(oq[1], op[1])
    assert relerr(c1.velocities, v) < 1e-7


# ---------------------------------------------------------------- edge cases
def test_edge_sizes(api, systems):
    spec, s, o = systems["doublePendulum"]
    for B in (1, 63, 64, 65, 255, 256, 257, 1025):
        q, qd = E.sample_config(spec, 5, B)
        p = o.to_phase_batch(q, qd)
        dq, dp = api.hamEqs(s, api.Phase(q, p))
        odq, odp, _ = o.hameqs_batch(q, p)
        assert dq.shape == (2, B) and relerr(dq, odq) < 1e-11 and relerr(dp, odp) < 1e-11
    # empty ensemble
    e = np.empty((2, 0))
    dq, dp = api.hamEqs(s, api.Phase(e, e))
    assert dq.shape == (2, 0)
    ph = api.rk4Steps(0.01, 3, s, api.Phase(e, e))
    assert ph.positions.shape == (2, 0)
    # single trajectory, reference-shaped [n] arrays
    dq1, dp1 = api.hamEqs(s, api.Phase(np.array(spec.q0), np.zeros(2)))
    np.testing.assert_allclose(dq1, [0, 0], atol=1e-15)
    np.testing.assert_allclose(dp1, [-10, 0], atol=1e-14)
    # zero steps is the identity
    q, qd = E.sample_config(spec, 5, 10)
    ph = api.rk4Steps(0.01, 0, s, api.Phase(q, qd))
    np.testing.assert_array_equal(ph.positions, q)


def test_singular_mass_matrix_is_flagged(api, oracle_lib):
    """Zero inertias make K singular: the reference's `inv` throws (Hamilton.hs:321,381);
    the ensemble path flags the lane, the single-trajectory call raises."""
    from hamilton_amd import tracer as T
    s = api.mkSystem_([0.0, 0.0], lambda q: [T.sin(q[0]), 0.5 - T.cos(q[0])], lambda x: x[1], n=1)
    q = np.array([[0.1, 0.2, 0.3]]); p = np.array([[1.0, 1.0, 1.0]])
    api.hamEqs(s, api.Phase(q, p))
    st = np.asarray(s.last_status)
    assert np.all(st & 1), st
    with pytest.raises(api.SingularSystem):
        api.velocities(s, api.Phase(np.array([0.1]), np.array([1.0])))


@pytest.mark.parametrize("B", [1000, 8192])
@pytest.mark.parametrize("name", ["doublePendulum~mixed", "spring~mixed", "threeBodyPolar~mixed", "chain6~mixed", "chain12~mixed",
                                  "chain20~mixed"])
def test_indefinite_mass_matrices_are_inverted_like_the_reference(api, oracle_lib, name, B):
    """The reference inverts every K = J^T M J by LU with partial pivoting (hmatrix `inv` = LAPACK dgesv against the
    identity, Hamilton.hs:321, :381), so inertias of mixed sign -- K symmetric, indefinite, invertible -- are a legal
    input there.  VALUES, not flags, against the oracle's literal restatement (lu_inverse), per trajectory within
    1e-10 cond(K): velocities, hamEqs, hamiltonian, 5 RK4 steps, stepHam -- on the kernels the library dispatches for
    (n, B): lane kernels for n <= 16 at EITHER ensemble size (the four-lane kernels do not pivot and are never chosen
    for such a system), the wave-cooperative kernels' solve_pivoted for n = 20.  Round 3 flagged every trajectory
    HAMK_ST_SINGULAR on the quad / wave mappings."""
    from hamilton_amd import _abi
    spec = E.get(name)
    s = api.system_from_spec(spec)
    o = oracle_lib.OracleSystem(spec)
    assert s.options(B)["mapping"] == (_abi.MAP_LANE if spec.n <= 16 else _abi.MAP_WAVE)
    nb = min(B, 256)                                         # the oracle's share (the launch covers all B)
    q, qd = E.sample_config(spec, 77, B)
    qd = qd + 0.4 * np.cos(1.0 + np.arange(spec.n * B, dtype=np.float64).reshape(spec.n, B))
    p = np.ascontiguousarray(o.to_phase_batch(q[:, :nb], qd[:, :nb]))
    pg = api.momenta(s, api.Config(q, qd))
    assert relerr(pg[:, :nb], p) < 1e-11
    ph = api.Phase(q, pg)
    K = [o.jacobian(q[:, i]).T @ np.diag(spec.inertia) @ o.jacobian(q[:, i]) for i in range(nb)]
    assert min(np.linalg.eigvalsh(k).min() for k in K) < 0.0, "the sample must contain indefinite mass matrices"
    scale = np.maximum(1.0, np.array([np.linalg.cond(k) for k in K]))
    def lane_err(a, b):
        a, b = np.asarray(a)[..., :nb], np.asarray(b)
        return (np.abs(a - b) / np.maximum(1.0, np.abs(b))).reshape(-1, nb).max(0)
    v = api.velocities(s, ph)
    st = np.asarray(s.last_status)
    assert not st.any(), (name, B, int(np.count_nonzero(st)))
    ov, ost = o.from_phase_batch(q[:, :nb], pg[:, :nb])
    assert not ost.any()
    ev = lane_err(v, ov) / scale
    dq, dp = api.hamEqs(s, ph)
    assert not np.asarray(s.last_status).any()
    odq, odp, _ = o.hameqs_batch(q[:, :nb], pg[:, :nb])
    eh = np.maximum(lane_err(dq, odq), lane_err(dp, odp)) / scale
    eH = lane_err(api.hamiltonian(s, ph), o.observe_batch(q[:, :nb], pg[:, :nb])[2]) / scale
    assert ev.max() < 1e-10 and eh.max() < 1e-10 and eH.max() < 1e-10, (name, B, ev.max(), eh.max(), eH.max())
    # Stepping: an indefinite "kinetic energy" does not confine the motion -- a trajectory can run into a surface det K = 0
    # within a few steps, where both implementations produce garbage (the first GPU run of this test: NaN on a few lanes,
    # 1e3 on others, with velocities / hamEqs / hamiltonian above exact on all of them).  The comparison is made on the lanes
    # the ORACLE ITSELF finds well-behaved over the span: its result moves by less than 1e4 x a 1e-9 relative perturbation
    # of the start.  Most lanes must qualify (measured: 76 % of the 20-link chain's, 91-100 % of the others').
    def regular(step):
        a = step(q[:, :nb], pg[:, :nb])
        b = step(q[:, :nb] * (1 + 1e-9), pg[:, :nb] * (1 - 1e-9))
        with np.errstate(invalid="ignore", over="ignore"):
            sens = np.maximum(np.abs(a[0] - b[0]).max(0), np.abs(a[1] - b[1]).max(0)) / 1e-9
        return a, np.isfinite(sens) & (sens < 1e4)
    (oq, op), keep = regular(lambda x, y: o.rk4_steps_batch(x, y, spec.dt, 5))
    assert keep.mean() > 0.5, (name, B, float(keep.mean()))
    r = api.rk4Steps(spec.dt, 5, s, ph)
    with np.errstate(invalid="ignore", over="ignore"):
        er = (np.maximum(lane_err(r.positions, oq), lane_err(r.momenta, op)) / scale)[keep]
    assert er.max() < 1e-9, (name, B, er.max())
    (sq, sp, sns), keep = regular(lambda x, y: o.step_ham_batch(x, y, 2 * spec.dt))
    assert keep.mean() > 0.5, (name, B, float(keep.mean()))
    sh = api.stepHam(2 * spec.dt, s, ph)
    same = (np.asarray(s.last_nsub)[:nb] == sns) & keep
    assert same[keep].mean() >= 0.97, (name, B, float(same[keep].mean()))
    with np.errstate(invalid="ignore", over="ignore"):
        es = (np.maximum(lane_err(sh.positions, sq), lane_err(sh.momenta, sp)) / scale)[same]
    assert es.max() < 1e-8, (name, B, es.max())


def test_the_quad_mapping_refuses_a_system_it_cannot_pivot_for(api):
    from hamilton_amd import _abi
    with pytest.raises(api.HamkError) as e:
        api.system_from_spec(E.get("chain20~mixed"), {"mapping": _abi.MAP_QUAD})
    assert e.value.code == _abi.HAMK_ERR_UNSUPPORTED


def test_nonfinite_is_flagged(api, systems):
    spec, s, _ = systems["twoBody"]
    q = np.array([[2.0, 0.0, np.nan], [0.0, 0.0, 0.0]])     # r = 0 -> division by zero; NaN input
    p = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    ph = api.rk4Steps(0.01, 2, s, api.Phase(q, p))
    st = np.asarray(s.last_status)
    assert st[0] == 0 and (st[1] & 3) and (st[2] & 2), st
    assert np.all(np.isfinite(ph.positions[:, 0]))


def test_negative_base_constant_power(api, systems):
    """spring's `x ** 2` must stay valid for x < 0 (Examples.hs:154; SURVEY.md hard parts)."""
    spec, s, o = systems["spring"]
    q = np.array([[0.1], [-0.15], [0.2]]); p = np.array([[0.3], [-0.2], [0.1]])
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    odq, odp, _ = o.hameqs_batch(q, p)
    assert np.all(np.isfinite(dp)) and relerr(dp, odp) < 1e-12 and relerr(dq, odq) < 1e-12


def test_device_pointers_equal_host_staging(api, systems):
    """HAMK_MEM_DEVICE (torch CUDA tensors, in place) and HAMK_MEM_HOST staging give identical bits."""
    import torch
    spec, s, o = systems["doublePendulum"]
    B = 5000
    q, qd = E.sample_config(spec, 31337, B)
    p = o.to_phase_batch(q, qd)
    host = api.rk4Steps(0.01, 20, s, api.Phase(q, p))
    tq, tp = torch.from_numpy(q).cuda(), torch.from_numpy(p).cuda()
    dev = api.rk4Steps(0.01, 20, s, api.Phase(tq, tp))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.positions.cpu().numpy(), host.positions)
    np.testing.assert_array_equal(dev.momenta.cpu().numpy(), host.momenta)
    # in-place variant advances the caller's tensors
    api.rk4Steps(0.01, 20, s, api.Phase(tq, tp), inplace=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tq.cpu().numpy(), host.positions)
    sq, sp = torch.from_numpy(q).cuda(), torch.from_numpy(p).cuda()
    pure = api.stepHam(0.03, s, api.Phase(sq, sp))
    np.testing.assert_array_equal(sq.cpu().numpy(), q)                      # the pure form leaves its argument alone
    api.stepHam(0.03, s, api.Phase(sq, sp), inplace=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(sq.cpu().numpy(), pure.positions.cpu().numpy())
    np.testing.assert_array_equal(sp.cpu().numpy(), pure.momenta.cpu().numpy())


@pytest.mark.parametrize("B", [1, 7, 300, 20000])
def test_host_pointer_paths_equal_device_path(api, systems, B):
    """Host-pointer calls take the pinned, device-mapped arena when the arrays are small (B = 1, 7,
    300: the kernel reads/writes host memory directly) and staged copies when large (B = 20000),
    mixed in between; every entry point must give the bits of the HAMK_MEM_DEVICE path."""
    import torch
    spec, s, o = systems["spring"]
    q, qd = E.sample_config(spec, 4242, B)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    eq = lambda d, h: np.testing.assert_array_equal(d.cpu().numpy(), h)
    ph_h = api.toPhase(s, api.Config(q, qd)); ph_d = api.toPhase(s, api.Config(T(q), T(qd)))
    eq(ph_d.momenta, ph_h.momenta)
    p = ph_h.momenta
    eq(api.fromPhase(s, api.Phase(T(q), T(p))).velocities, api.fromPhase(s, api.Phase(q, p)).velocities)
    eq(api.underlyingPos(s, T(q)), api.underlyingPos(s, q))
    eq(api.hamiltonian(s, api.Phase(T(q), T(p))), api.hamiltonian(s, api.Phase(q, p)))
    eq(api.lagrangian(s, api.Config(T(q), T(qd))), api.lagrangian(s, api.Config(q, qd)))
    dq_h, dp_h = api.hamEqs(s, api.Phase(q, p)); dq_d, dp_d = api.hamEqs(s, api.Phase(T(q), T(p)))
    eq(dq_d, dq_h); eq(dp_d, dp_h)
    r_h = api.rk4Steps(0.01, 7, s, api.Phase(q, p)); r_d = api.rk4Steps(0.01, 7, s, api.Phase(T(q), T(p)))
    eq(r_d.positions, r_h.positions); eq(r_d.momenta, r_h.momenta)
    s_h = api.stepHam(0.05, s, api.Phase(q, p)); n_h = np.asarray(s.last_nsub).copy()
    s_d = api.stepHam(0.05, s, api.Phase(T(q), T(p))); eq(s.last_nsub, n_h)
    eq(s_d.positions, s_h.positions); eq(s_d.momenta, s_h.momenta)
    # a 3-point grid (pinned side input for small host calls) and a 6000-point one (48 KB: device scratch)
    for ts in (np.array([0.0, 0.02, 0.05]), np.linspace(0.0, 0.03, 6000)):
        if B > 300 and len(ts) > 3:
            continue
        e_h = api.evolveHam(s, api.Phase(q, p), ts); e_d = api.evolveHam(s, api.Phase(T(q), T(p)), ts)
        for r in (0, 1, len(ts) - 1):
            eq(e_d[r].positions, e_h[r].positions); eq(e_d[r].momenta, e_h[r].momenta)
    torch.cuda.synchronize()


def test_large_host_arrays(api, systems):
    """Host arrays far beyond the pinned arena (67 MB per array, a ragged size; staged through device memory with
    hipMemcpyAsync -- 50 GB/s both ways from touched pageable memory on the MI355X boxes, scripts/pcie_rate.py) against the
    device-pointer path, bitwise; then the same handle on small arrays again (the pinned arena) and a mid-size one."""
    import torch
    spec, s, o = systems["doublePendulum"]
    B = (1 << 22) + 7
    q, qd = E.sample_config(spec, 4242, B)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ph_h = api.toPhase(s, api.Config(q, qd))
    ph_d = api.toPhase(s, api.Config(T(q), T(qd)))
    assert np.array_equal(ph_h.momenta, ph_d.momenta.cpu().numpy())
    r_h = api.rk4Steps(0.01, 3, s, ph_h)
    r_d = api.rk4Steps(0.01, 3, s, ph_d)
    assert np.array_equal(r_h.positions, r_d.positions.cpu().numpy()) and np.array_equal(r_h.momenta, r_d.momenta.cpu().numpy())
    assert not np.shares_memory(r_h.positions, ph_h.positions) and np.array_equal(ph_h.positions, q)       # inputs untouched
    for Bs in (130, 100000):
        qs, ps = q[:, :Bs].copy(), ph_h.momenta[:, :Bs].copy()
        a = api.rk4Steps(0.01, 3, s, api.Phase(qs, ps))
        assert np.array_equal(a.positions, r_h.positions[:, :Bs]) and np.array_equal(a.momenta, r_h.momenta[:, :Bs])
    torch.cuda.synchronize()


def test_small_host_calls_see_fresh_inputs(api, systems):
    """The pinned arena of small host-pointer calls is rewritten by the CPU before every call and
    reused at the same offsets by every entry point: alternate different inputs through one handle,
    many times, and check every result (a previous call's bytes must never be served again)."""
    spec, s, o = systems["doublePendulum"]
    B = 130
    ins = []
    for k in range(4):
        q, qd = E.sample_config(spec, 1000 * k, B)
        p = o.to_phase_batch(q, qd)
        oq, op, ons = o.step_ham_batch(q, p, 0.02)
        rq, rp = o.rk4_steps_batch(q, p, 0.01, 3)
        ins.append((q, p, oq, op, ons, rq, rp))
    for it in range(40):
        q, p, oq, op, ons, rq, rp = ins[(it * 7 + it // 3) % 4]
        st = api.stepHam(0.02, s, api.Phase(q, p))
        same = np.asarray(s.last_nsub) == ons
        assert same.mean() >= 0.99, (it, float(same.mean()))
        assert relerr(st.positions[:, same], oq[:, same]) < 1e-9 and relerr(st.momenta[:, same], op[:, same]) < 1e-9, it
        r4 = api.rk4Steps(0.01, 3, s, api.Phase(q, p))
        assert relerr(r4.positions, rq) < 1e-11 and relerr(r4.momenta, rp) < 1e-11, it


@pytest.mark.parametrize("name", ["doublePendulum", "spring", "threeBodyPolar", "opcodeZoo", "room"])
def test_steppers_are_deterministic(api, systems, name):
    """Every lane is independent, so two runs on the same input must agree bit for bit -- for both
    steppers, after other kernels have run (they leave other register contents behind).  An unrolled
    RKF45 body that spilled 101 SGPRs once failed exactly this."""
    import torch
    spec, s, o = systems[name]
    B = 1 << 16
    q, qd = E.sample_config(spec, 777, B)
    ph = api.toPhase(s, api.Config(torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda()))
    api.hamEqs(s, ph); api.hamiltonian(s, ph)
    runs = []
    for _ in range(3):
        a = api.stepHam(4 * spec.dt, s, ph); na = s.last_nsub.clone()
        b = api.rk4Steps(spec.dt, 5, s, ph)
        api.hamEqs(s, ph)
        runs.append((a.positions.clone(), a.momenta.clone(), na, b.positions.clone(), b.momenta.clone()))
    torch.cuda.synchronize()
    for r in runs[1:]:
        for x, y in zip(r, runs[0]):
            assert torch.equal(x, y), name


def test_device_memory_and_gather_through_the_abi(api, systems, hamk_lib):
    """A host without HIP or torch: hamk_device_malloc / hamk_memcpy keep the ensemble in HBM across
    calls, hamk_gather_batch reassembles SoA shards (here three unequal ones on the one device) in
    part order -- into host memory and into device memory."""
    import ctypes
    L = hamk_lib
    spec, s, o = systems["spring"]
    n = spec.n
    sizes = [257, 1, 1000]
    dev = ctypes.c_int32(-1)
    assert L.hamk_get_device(ctypes.byref(dev)) == 0 and dev.value >= 0
    assert L.hamk_set_device(dev.value) == 0
    parts_q, parts_p, want_q, want_p, ptrs = [], [], [], [], []
    start = 0
    for Bg in sizes:
        q, qd = E.sample_config(spec, start, Bg)
        p = o.to_phase_batch(q, qd)
        start += Bg
        dq, dp, dst = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        for ptr, nbytes in ((dq, q.nbytes), (dp, p.nbytes), (dst, 4 * Bg)):
            assert L.hamk_device_malloc(ctypes.byref(ptr), nbytes) == 0 and ptr.value
            ptrs.append(ptr)
        assert L.hamk_memcpy(dq, q.ctypes.data, q.nbytes, 0) == 0
        assert L.hamk_memcpy(dp, p.ctypes.data, p.nbytes, 0) == 0
        assert L.hamk_rk4_steps(s._h, Bg, dq, dp, ctypes.c_double(0.01), 5, dst, 1) == 0      # HAMK_MEM_DEVICE
        ref = api.rk4Steps(0.01, 5, s, api.Phase(q, p))
        want_q.append(ref.positions); want_p.append(ref.momenta)
        parts_q.append(dq); parts_p.append(dp)
    assert L.hamk_synchronize(s._h) == 0
    total = sum(sizes)
    Bs = (ctypes.c_int64 * 3)(*sizes)
    for parts, want in ((parts_q, want_q), (parts_p, want_p)):
        arr = (ctypes.c_void_p * 3)(*[p.value for p in parts])
        out = np.empty((n, total))
        assert L.hamk_gather_batch(3, n, Bs, arr, out.ctypes.data, 0) == 0                       # to host
        np.testing.assert_array_equal(out, np.concatenate(want, axis=1))
        dout = ctypes.c_void_p()
        assert L.hamk_device_malloc(ctypes.byref(dout), out.nbytes) == 0
        assert L.hamk_gather_batch(3, n, Bs, arr, dout, 1) == 0                                  # to the current device
        back = np.empty_like(out)
        assert L.hamk_memcpy(back.ctypes.data, dout, out.nbytes, 1) == 0
        np.testing.assert_array_equal(back, out)
        d2 = ctypes.c_void_p()
        assert L.hamk_device_malloc(ctypes.byref(d2), out.nbytes) == 0
        assert L.hamk_memcpy(d2, dout, out.nbytes, 2) == 0                                       # D2D
        assert L.hamk_memcpy(back.ctypes.data, d2, out.nbytes, 1) == 0
        np.testing.assert_array_equal(back, out)
        ptrs += [dout, d2]
    for ptr in ptrs:
        assert L.hamk_device_free(ptr) == 0


# ---------------------------------------------------------------- BASELINE.json full size: properties
def test_full_size_properties(api, systems):
    """Config 2 at full size (1,048,576 double-pendulum trajectories): size-independent properties.
    (a) shard invariance: any sub-range computed alone is bit-identical to the same lanes of the full run;
    (b) time reversal and (c) energy drift converge at RK4's order when dt is halved;
    (d) the oracle agrees on a strided sample."""
    import torch
    spec, s, o = systems["doublePendulum"]
    B = 1 << 20
    q, qd = E.sample_config(spec, 0, B)
    tq, tqd = torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda()
    ph0 = api.toPhase(s, api.Config(tq, tqd))
    h0 = api.hamiltonian(s, ph0)
    ph1 = api.rk4Steps(0.01, 100, s, ph0)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(s.last_status)) == 0
    # (a)
    lo, hi = 300_001, 300_001 + 70_000
    sub = api.rk4Steps(0.01, 100, s, api.Phase(ph0.positions[:, lo:hi], ph0.momenta[:, lo:hi]))
    assert torch.equal(sub.positions, ph1.positions[:, lo:hi]) and torch.equal(sub.momenta, ph1.momenta[:, lo:hi])
    # (b) + (c): RK4 is a 4th-order method -- halving dt must shrink the ensemble-mean time-reversal
    # error ~2^5 and the ensemble-mean energy drift ~2^4..2^5 (measured on MI355X: 31.8 and 24);
    # absolute levels bound loosely (fast-swinging members have |theta'| dt ~ 0.1).
    def rev_and_drift(dt, n):
        fwd = api.rk4Steps(dt, n, s, ph0)
        back = api.rk4Steps(-dt, n, s, fwd)
        err = torch.maximum((back.positions - ph0.positions).abs().amax(0), (back.momenta - ph0.momenta).abs().amax(0))
        drift = (api.hamiltonian(s, fwd) - h0).abs() / h0.abs().clamp(min=1.0)
        return err, drift
    e1, d1 = rev_and_drift(0.01, 100)
    e2, d2 = rev_and_drift(0.005, 200)
    assert float(e1.median()) < 2e-6 and float(e1.max()) < 1e-2, (float(e1.median()), float(e1.max()))
    assert float(d1.median()) < 1e-6 and float(d1.max()) < 1e-3, (float(d1.median()), float(d1.max()))
    r_rev, r_drift = float(e1.mean() / e2.mean()), float(d1.mean() / d2.mean())
    assert 16.0 < r_rev < 64.0, r_rev
    assert 8.0 < r_drift < 64.0, r_drift
    # (d)
    idx = np.arange(0, B, 4099)
    qs, ps = ph0.positions[:, idx].cpu().numpy(), ph0.momenta[:, idx].cpu().numpy()
    oq, op = o.rk4_steps_batch(qs, ps, 0.01, 100)
    assert relerr(ph1.positions[:, idx].cpu().numpy(), oq) < 1e-8
    assert relerr(ph1.momenta[:, idx].cpu().numpy(), op) < 1e-8


# ---------------------------------------------------------------- every code-generation variant
@pytest.mark.parametrize("name", ["opcodeZoo", "doublePendulum", "spring", "threeBodyPolar"])
def test_all_codegen_variants_agree(api, oracle_lib, name, monkeypatch):
    """MODE_H (full second-order jets), MODE_D (two sweeps, directional jets, trig cache) and MODE_R
    (second sweep in reverse mode: generated adjoint code), each with the unrolled and the
    stage-loop RK4 body, against the oracle: every derivative rule of every jet type and of the
    reverse sweep is exercised by opcodeZoo (tape opcodes 0-26; abs / signum: test_abs_and_signum_opcodes)."""
    spec = E.get(name)
    o = oracle_lib.OracleSystem(spec)
    B = 257
    q, qd = E.sample_config(spec, 2024, B)
    p = o.to_phase_batch(q, qd)
    odq, odp, _ = o.hameqs_batch(q, p)
    oq, op = o.rk4_steps_batch(q, p, spec.dt, 3)
    sq, sp, sns = o.step_ham_batch(q, p, 0.01)
    # the symbolic right-hand side (hamk_codegen.cpp symbolic_mass_matrix) is taken BEFORE MODE_H / MODE_R are looked at: the matrix runs
    # with HAMK_K_SYMBOLIC=0, so that the jets the mode names are what computes; the default build is one more variant
    for mode in ("H", "D", "R", "default"):
        # RK4 body: the library's own choice (unrolled for small kernels, stage loop above the
        # 64 KiB code-size guard -- e.g. opcodeZoo) and the stage loop forced.  The unrolled body is
        # deliberately NOT forced on kernels the guard would reject: hipcc/ROCm 7.2 miscompiles the
        # 98 KiB unrolled opcodeZoo kernel (1e-4 off after one step on every lane, status clean).
        for loop in (None, "1"):
            if mode == "default":
                monkeypatch.delenv("HAMK_AD_MODE", raising=False)
                monkeypatch.delenv("HAMK_K_SYMBOLIC", raising=False)
            else:
                monkeypatch.setenv("HAMK_AD_MODE", mode)
                monkeypatch.setenv("HAMK_K_SYMBOLIC", "0")
            if loop is None:
                monkeypatch.delenv("HAMK_RK4_LOOP", raising=False)
            else:
                monkeypatch.setenv("HAMK_RK4_LOOP", loop)
            s = api.system_from_spec(spec)
            assert s.kernel_bytes("hamk_rk4_steps_k") < 96 * 1024
            if mode == "default":
                assert ("HAS_SYM_K = true" in s.source) == (name != "opcodeZoo") and ("HAS_SYM_DT = true" in s.source) == (name != "opcodeZoo")
            else:
                assert f"MODE_H = {'true' if mode == 'H' else 'false'}" in s.source
                assert f"MODE_R = {'true' if mode == 'R' else 'false'}" in s.source
                assert "HAS_SYM_K = false" in s.source and "HAS_SYM_DT = false" in s.source and "HAS_SYM_GU = false" in s.source
            dq, dp = api.hamEqs(s, api.Phase(q, p))
            assert relerr(dq, odq) < 1e-11 and relerr(dp, odp) < 1e-11, (name, mode, loop, relerr(dp, odp))
            ph = api.rk4Steps(spec.dt, 3, s, api.Phase(q, p))
            assert relerr(ph.positions, oq) < 1e-11 and relerr(ph.momenta, op) < 1e-11, (name, mode, loop)
            st = api.stepHam(0.01, s, api.Phase(q, p))
            same = np.asarray(s.last_nsub) == sns          # identical accept/reject sequence as the oracle
            assert same.mean() >= 0.99, (name, mode, loop, same.mean())
            assert relerr(st.positions[:, same], sq[:, same]) < 1e-10, (name, mode, loop)
            assert relerr(st.momenta[:, same], sp[:, same]) < 1e-10, (name, mode, loop)


def test_evolveham_time_grid_edge_cases(api, systems):
    """Old gsl_odeiv binding (hamk_system_set_gsl_api(1)): hmatrix-gsl's loop is `for each ti: while
    (t < ti) step` (SURVEY.md section 8c box): a repeated or decreasing time does no stepping and
    returns the current state; a negative step does nothing.  (The default gsl_odeiv2 binding's
    rules are in tests/test_gpu_configs.py::test_odeiv2_direction_rules.)"""
    spec, s, o = systems["doublePendulum"]
    q, qd = E.sample_config(spec, 3, 9)
    p = o.to_phase_batch(q, qd)
    ts = np.array([0.0, 0.1, 0.1, 0.05, 0.2])
    s.gsl_api = 1
    o.gsl_api = 1
    try:
        rows = api.evolveHam(s, api.Phase(q, p), ts)
        oq, op, _ = o.evolve_ham_batch(q, p, ts)
        np.testing.assert_array_equal(rows[2].positions, rows[1].positions)
        np.testing.assert_array_equal(rows[3].positions, rows[1].positions)
        for r in range(1, 5):
            assert relerr(rows[r].positions, oq[r]) < 1e-9 and relerr(rows[r].momenta, op[r]) < 1e-9
        back = api.stepHam(-0.01, s, api.Phase(q, p))                 # t = 0 >= ti = -0.01: no steps
        np.testing.assert_array_equal(back.positions, q)
        np.testing.assert_array_equal(back.momenta, p)
    finally:
        s.gsl_api = 2
        o.gsl_api = 2


def test_single_trajectory_frame_loop(api, systems):
    """BASELINE config 1 shape: one trajectory, repeated stepHam calls through the host-staged path
    (persistent staging buffers in the handle); results equal the CPU oracle's to roundoff growth."""
    spec, s, o = systems["doublePendulum"]
    q, p = np.array(spec.q0), np.zeros(2)
    oq, op = q, p
    for _ in range(50):
        ph = api.stepHam(1.0 / 12.0, s, api.Phase(q, p))          # Examples.hs:415,429
        q, p = ph.positions, ph.momenta
        oq, op = o.step_ham(1.0 / 12.0, oq, op)
    assert relerr(q, oq) < 1e-7 and relerr(p, op) < 1e-7


def test_rank_deficient_jacobian_is_flagged(api):
    """Positive inertias but dependent coordinates: K = J^T M J is singular (det = 0).  With all
    inertias positive the pivoting fallback is compiled out and the lane is flagged by a select."""
    s = api.mkSystem([1.0, 2.0], lambda q: [q[0] + q[1], q[0] + q[1]], lambda q: q[0] * q[0], n=2)
    assert "INERTIA_POS = true" in s.source
    q = np.array([[0.1, 0.2], [0.3, 0.4]]); p = np.ones((2, 2))
    api.hamEqs(s, api.Phase(q, p))
    assert np.all(np.asarray(s.last_status) & 1)
    with pytest.raises(api.SingularSystem):
        api.velocities(s, api.Phase(np.array([0.1, 0.3]), np.array([1.0, 1.0])))
    # three coordinates, the generic LDL^T path
    s3 = api.mkSystem([1.0, 1.0, 1.0], lambda q: [q[0] + q[1], q[1] + q[2], q[0] + 2 * q[1] + q[2]], lambda q: q[0], n=3)
    api.hamEqs(s3, api.Phase(np.ones((3, 4)), np.ones((3, 4))))
    assert np.all(np.asarray(s3.last_status) & 3)


def test_first_use_self_check_and_recovery(api, oracle_lib, monkeypatch):
    """At first use the fused RK4 / RKF45 kernels are checked against the hamEqs kernel (four resp.
    six launches combined on the host).  With the test hook pretending the unrolled bodies are
    wrong, the module is rebuilt with the stage-loop bodies and still gives the oracle's numbers."""
    spec = E.get("doublePendulum")
    o = oracle_lib.OracleSystem(spec)
    q, qd = E.sample_config(spec, 8, 100)
    p = o.to_phase_batch(q, qd)
    monkeypatch.setenv("HAMK_SELFCHECK_FAULT", "rk4,rkf")
    s = api.system_from_spec(spec)
    assert "RK4_STAGE_LOOP = false" in s.source
    ph = api.rk4Steps(0.01, 5, s, api.Phase(q, p))               # first use: self-check -> rebuild
    assert "RK4_STAGE_LOOP = true" in s.source and "RKF_STAGE_LOOP = true" in s.source
    oq, op = o.rk4_steps_batch(q, p, 0.01, 5)
    assert relerr(ph.positions, oq) < 1e-12 and relerr(ph.momenta, op) < 1e-12
    st = api.stepHam(0.01, s, api.Phase(q, p))
    sq, sp, _ = o.step_ham_batch(q, p, 0.01)
    assert relerr(st.positions, sq) < 1e-12


def test_initial_conditions_are_drawn_on_the_device_from_the_global_index(api):
    """hamk_sample_batch (SURVEY.md 8e "inputs generated on-device from the global index -> no scatter needed"): the numpy
    sampler's bits (examples.sample_config) at BASELINE config 2's 2^20, for a shard that starts anywhere, through device
    and host pointers -- and G shards drawn separately are the slices of one draw."""
    import torch
    from hamilton_amd import ensemble
    for name, B in (("doublePendulum", 1 << 20), ("threeBodyPolar", 70001), ("chain32", 4099)):
        spec = E.get(name)
        s = api.system_from_spec(spec)
        want_q, want_qd = E.sample_config(spec, 0, B)
        c = api.sampleConfig(s, spec.q_box, spec.qd_box, 0, B, E.SEED, "cuda")
        assert np.array_equal(c.positions.cpu().numpy(), want_q) and np.array_equal(c.velocities.cpu().numpy(), want_qd), name
        for g in range(3):
            lo, hi = ensemble.shard_bounds(B, 3, g)
            part = api.sampleConfig(s, spec.q_box, spec.qd_box, lo, hi - lo, E.SEED, "cuda")
            assert torch.equal(part.positions, c.positions[:, lo:hi]) and torch.equal(part.velocities, c.velocities[:, lo:hi])
        far = api.sampleConfig(s, spec.q_box, spec.qd_box, 3 << 40, 1000, 12345)          # host arrays, a huge global index, another seed
        wq, wqd = E.sample_config(spec, 3 << 40, 1000, 12345)
        assert np.array_equal(far.positions, wq) and np.array_equal(far.velocities, wqd)
    with pytest.raises(ValueError):
        api.sampleConfig(s, spec.q_box[:-1], spec.qd_box, 0, 4, 1)


def test_cold_path_compiles_on_the_gpu_box(api, oracle_lib):
    """Every other GPU test loads code objects that were cross-compiled ahead and travelled with the snapshot (`.hamk_cache/`).
    This one switches the cache OFF (hamk_options::cache): tape -> source -> hiprtc for gfx950 happens HERE, on the box, and the
    freshly compiled module goes through the first-use self-check and the oracle like any other -- the path a host without a
    warm cache takes (a system of its own so that no earlier test has left a handle to the same module around)."""
    import time
    from hamilton_amd import _abi
    spec = E.double_pendulum(m1=1.5, m2=0.7)               # a small tape no other test builds (other masses): a few seconds of hiprtc
    t0 = time.time()
    s = api.system_from_spec(spec, {"cache": _abi.OFF})
    t_compile = time.time() - t0
    assert s.options()["cache"] == _abi.OFF and s.code_size > 0
    o = oracle_lib.OracleSystem(spec)
    q, qd = E.sample_config(spec, 3, 200)
    p = o.to_phase_batch(q, qd)
    assert relerr(api.momenta(s, api.Config(q, qd)), p) < 1e-12
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    odq, odp, _ = o.hameqs_batch(q, p)
    assert relerr(dq, odq) < 1e-10 and relerr(dp, odp) < 1e-10
    ph = api.rk4Steps(spec.dt, 10, s, api.Phase(q, p))
    oq, op = o.rk4_steps_batch(q, p, spec.dt, 10)
    assert relerr(ph.positions, oq) < 1e-10 and relerr(ph.momenta, op) < 1e-10
    st = api.stepHam(spec.dt, s, api.Phase(q, p))
    sq, sp, sns = o.step_ham_batch(q, p, spec.dt)
    assert np.array_equal(np.asarray(s.last_nsub), sns) and relerr(st.positions, sq) < 1e-9
    assert t_compile > 0.2, "served from a cache after all?"


@pytest.mark.parametrize("name,mapping", [("chain19", "quad"), ("chain34", "wave")])
def test_cold_path_of_the_cooperative_mappings(api, oracle_lib, name, mapping):
    """The same on the two cooperative mappings (round 6): a four-lane module (chain19) and a wave-cooperative one (chain34: one
    trajectory per wavefront, matrix cores) that no other test builds, compiled on the box with the cache off -- 20-60 s of hiprtc
    each -- then self-check, hamEqs and five RK4 steps against the oracle."""
    import time
    from hamilton_amd import _abi
    spec = E.get(name)
    t0 = time.time()
    s = api.system_from_spec(spec, {"cache": _abi.OFF})
    t_compile = time.time() - t0
    want = {"quad": _abi.MAP_QUAD, "wave": _abi.MAP_WAVE}[mapping]
    assert s.options()["cache"] == _abi.OFF and s.options()["mapping"] == want and t_compile > 2.0
    o = oracle_lib.OracleSystem(spec)
    q, _ = E.sample_config(spec, 3, 40)
    qd = 0.3 * np.cos(np.arange(spec.n * 40).reshape(spec.n, 40) * 0.7)
    p = o.to_phase_batch(q, qd)
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    odq, odp, _ = o.hameqs_batch(q, p)
    assert relerr(dq, odq) < 1e-10 and relerr(dp, odp) < 1e-10 and not np.any(s.last_status)
    ph = api.rk4Steps(spec.dt, 5, s, api.Phase(q, p))
    oq, op = o.rk4_steps_batch(q, p, spec.dt, 5)
    assert relerr(ph.positions, oq) < 1e-10 and relerr(ph.momenta, op) < 1e-10


def test_derivative_rules_at_the_edge_of_their_domain(api):
    """sqrt at 0: the reference's `ad` yields Infinity for the derivative, the device rules take their reciprocals from frcp
    (hamk_device.hpp) and yield NaN there -- both non-finite; the trajectory is flagged HAMK_ST_NONFINITE, its neighbours are not
    touched.  (stated and tested instead of guarded: the guard would be paid by every evaluation.)"""
    from hamilton_amd import tracer as T
    spec = E.SystemSpec(name="sqrtEdge", m=2, n=1, inertia=(1.0, 1.0), f=lambda q, o: [q[0], o.sqrt(q[0])], u=lambda q, o: q[0] * q[0],
                        u_space=E.U_GENERALIZED, q0=(1.0,), qd0=(0.0,), q_box=((0.5, 2.0),), qd_box=((-1.0, 1.0),), cite="build-defined (domain edge of sqrt)")
    s = api.system_from_spec(spec)
    q = np.array([[1.0, 0.0, 2.0, 0.25]])
    p = np.array([[0.3, 0.3, 0.3, 0.3]])
    dq, dp = api.hamEqs(s, api.Phase(q, p))
    st = np.asarray(s.last_status)
    assert st[1] != 0 and not st[[0, 2, 3]].any()
    assert not np.isfinite(np.asarray(dp)[0, 1]) or not np.isfinite(np.asarray(dq)[0, 1])
    # K = 1 + 1 / (4 q): dq = p / K at the regular points
    assert np.allclose(np.asarray(dq)[0, [0, 2, 3]], 0.3 / (1.0 + 1.0 / (4.0 * q[0, [0, 2, 3]])), rtol=1e-13)
