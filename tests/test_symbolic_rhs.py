"""CPU: the generator's symbolic right-hand side (hamk_codegen.cpp symbolic_mass_matrix, poly_sweep, poly_reduce, poly_prune: K, dT/dq and
grad U as polynomials) against 50-digit fixtures, and the jets it replaces (HAMK_K_SYMBOLIC=0) against the same truth.

The yardsticks the suite had share the algebra under test -- the first-use self-check compares kernels that all call mass_matrix_sym /
dT_sym / gU_sym -- or its precision (central differences of the emitted K, the oracle's first-order AD in fp64).  Here:
  * TEXT: the emitted expressions of every member of tests/symbolic_family.py are evaluated in fp64 at the points of
    tests/golden/symbolic_family.json (oracle/gen_golden_symbolic.py: sympy differentiates, mpmath evaluates at 50 digits) and must
    agree to a DERIVED bound: the running error of the sum that was emitted.  A wrong sign, a lost term, a wrong slot or an over-eager
    prune is orders of magnitude outside it;
  * KERNELS: the lane kernels on the host (tests/test_host_emulation.py), built twice per system -- the default and HAMK_K_SYMBOLIC=0,
    flags asserted from the source -- against the fixtures, against the oracle, and against each other;
  * the example systems with HAMK_K_SYMBOLIC=0 under every HAMK_AD_MODE: the Hessian, directional and reverse jets on the systems
    whose default build never runs them.
No trajectory and no fixture point is left out: the family was selected by the reference's cond K < 1e4 (symbolic_family.SEEDS).

Size rules of the generator and the members that sit on them: dT/dq at most 12 n operations (111 / 112: 24 and 26 at n = 2), grad U
at most 64 monomials per component (113 / 114: 64 and 65).  NOT forced: (a) a dT/dq component of more than 64 monomials -- every
monomial of dT/dq carries two velocities, hence at least three operations, so 65 of them are 195 operations and the 12 n <= 84 rule
has refused long before; (b) a K entry of more than 24 monomials -- an entry that long costs about 110 operations, and K is symbolic
only where that is cheaper than the numerical sum (2 per output and entry): the rule is reachable only by padding the map with some 60
dummy outputs, which was not built."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import symbolic_family as F
from conftest import GOLDEN, fvec
from hamilton_amd import examples as E
from symbolic_text import emitted, eval_with_bound, flags, slot_sincos, sym_functions
from test_host_emulation import I, LL, P, check_against_golden, check_against_oracle, emulate  # noqa: F401  (emulate: a fixture)

OFF = {"HAMK_K_SYMBOLIC": "0"}
FIXTURE_DIGITS = 1e-29            # the fixtures carry 30 significant digits ...
FIXTURE_FLOOR = 1e-45             # ... of sums evaluated at 50 digits: where terms of order one cancel analytically (a polar K01) the
#                                   reference leaves 1e-50 times their magnitude, not zero; five digits of guard on that


@pytest.fixture(scope="module")
def family():
    with open(os.path.join(GOLDEN, "symbolic_family.json")) as fh:
        return json.load(fh)["blocks"]


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    return _api


@pytest.fixture(scope="module")
def sources(api):
    return {seed: api.system_from_spec(F.spec(seed)).source for seed in F.SEEDS}


# ---------------------------------------------------------------------------------------------------------------------------------
# what the family covers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_family_keeps_its_promises(sources, family):
    """Every member has the HAS_SYM_K / DT / GU flags it promises; every fixture point has cond K < 1e4 by the 50-digit reference; SEEDS
    covers all four flag combinations three times, 111 with cartesian and with generalized U three times each, n = 1 .. 7."""
    assert sorted(family) == sorted(str(s) for s in F.SEEDS) and sorted(F.PROMISE) == sorted(F.SEEDS)
    combos, spaces, ns = {}, {E.U_CARTESIAN: 0, E.U_GENERALIZED: 0}, set()
    for seed in F.SEEDS:
        spec = F.spec(seed)
        assert flags(sources[seed]) == F.PROMISE[seed], (seed, flags(sources[seed]))
        assert all(float(pt["cond_hint"]) < 1e4 for pt in family[str(seed)]["points"]), seed
        assert all(all(float(x) != 0.0 for x in pt["qd"]) for pt in family[str(seed)]["points"]), seed
        combos[F.PROMISE[seed]] = combos.get(F.PROMISE[seed], 0) + 1
        if F.PROMISE[seed] == "111":
            spaces[spec.u_space] += 1
        ns.add(spec.n)
    assert sorted(combos) == ["000", "100", "110", "111"] and min(combos.values()) >= 3, combos
    assert min(spaces.values()) >= 3, spaces
    assert ns == set(range(1, 8)), ns


def test_n_beyond_seven_is_refused(api):
    spec = F.refused_spec()
    assert spec.n == 8 and flags(api.system_from_spec(spec).source) == "000"


def test_u_side_fallbacks_and_u_shapes(sources):
    """110 by a failure on U's side: a sincos site of U whose operand no slot of f has, and a non-polynomial opcode in U -- with the SAME
    f as member 103, which gets 111: only U differs.  Neither emits a gU_sym.  And the two shapes of U that 111 must reach: a cartesian U
    of degree three in f's outputs (poly_reduce runs on U . f: the emitted gradient has terms of degree >= 3), a generalized U whose
    sincos sites read slots of f."""
    assert F.PROMISE[F.SLOT_MATCHING_U] == "111"
    for why, seed in F.U_FALLBACK.items():
        assert flags(sources[seed]) == "110" and emitted(sources[seed], "gU_sym") is None, (why, seed)
        assert emitted(sources[seed], "mass_matrix_sym") == emitted(sources[F.SLOT_MATCHING_U], "mass_matrix_sym")
    _, tu = F.spec(F.U_FALLBACK["no matching slot"]).trace()
    from hamilton_amd import tracer as T
    assert any(op in (T.OP_SIN, T.OP_COS) for op, _, _, _ in tu.ops)
    _, tu = F.spec(F.U_FALLBACK["non-polynomial opcode"]).trace()
    assert any(op == T.OP_EXP for op, _, _, _ in tu.ops)
    g = sym_functions(sources[F.SLOT_MATCHING_U])["gU"]
    _, tu = F.spec(F.SLOT_MATCHING_U).trace()
    assert F.spec(F.SLOT_MATCHING_U).u_space == E.U_GENERALIZED and any(op in (T.OP_SIN, T.OP_COS) for op, _, _, _ in tu.ops)
    assert any("s[" in e or "c[" in e for e in g.values())
    g = sym_functions(sources[F.CUBIC_CARTESIAN_U])["gU"]
    assert F.spec(F.CUBIC_CARTESIAN_U).u_space == E.U_CARTESIAN
    assert max(len(re.findall(r"\b[qsc]\[\d+\]", t)) for e in g.values() for t in e.split(" + ")) >= 3


def test_every_polynomial_opcode_is_on_a_symbolic_tape(sources):
    """Member 108 gets 111 with ADD, SUB, MUL, NEG, POWI 0 / 1 / 2 / 3, a division by a constant, and sincos of q_i, 2 q_i, q_i - q_j,
    q_i + q_j on its coordinate map's tape (operands read from the tape), q0's pair shared by several sites."""
    from hamilton_amd import tracer as T
    tf, _ = F.spec(108).trace()
    ops = tf.ops
    have = {op for op, _, _, _ in ops}
    assert {T.OP_ADD, T.OP_SUB, T.OP_MUL, T.OP_NEG, T.OP_DIV, T.OP_POWI, T.OP_SIN, T.OP_COS} <= have
    assert {b for op, _, b, _ in ops if op == T.OP_POWI} >= {0, 1, 2, 3}
    assert all(ops[b][0] == T.OP_CONST for op, _, b, _ in ops if op == T.OP_DIV)
    kinds = set()
    for op, a, _, _ in ops:
        if op in (T.OP_SIN, T.OP_COS):
            o2, x, y, _ = ops[a]
            kinds.add("input" if o2 == T.OP_INPUT else "sum" if o2 == T.OP_ADD else "difference" if o2 == T.OP_SUB else "multiple" if o2 == T.OP_MUL else "?")
    assert kinds == {"input", "sum", "difference", "multiple"}, kinds
    operand_of_q0 = [a for op, a, _, _ in ops if op in (T.OP_SIN, T.OP_COS) and ops[a][0] == T.OP_INPUT and ops[a][1] == 0]
    assert len(operand_of_q0) == 2 and len(set(operand_of_q0)) == 1
    assert flags(sources[108]) == "111"


def test_exact_cancellation_and_small_true_terms(sources):
    """poly_prune drops what cancelled and nothing else.  Polar coordinates (100, 101, 102): every off-diagonal entry of K is the text
    0.0, the diagonal is m and m r^2 -- one monomial.  A body hanging from a body (103): K01 is one product of cosines plus one of sines
    (cos(q0 - q1)), the diagonal constants.  Member 104, inertias 1, 1.3 and 1e-9: K01 = 1e-9 * 0.49 driven by the small body alone, and
    the monomial 1e-9 q0^2 in K00 next to a constant of order one -- both are there."""
    for seed, npart in ((100, 2), (101, 3), (102, 3)):
        k = sym_functions(sources[seed])["K"]
        n = F.spec(seed).n
        assert all(k[(a, b)] == "0.0" for a in range(n) for b in range(a + 1, n)), seed
        for i in range(npart):
            m = 1.0 + 0.5 * i
            assert eval(k[(2 * i, 2 * i)]) == m
            assert k[(2 * i + 1, 2 * i + 1)] == (f"q[{2 * i}] * q[{2 * i}]" if m == 1.0 else f"{m!r} * q[{2 * i}] * q[{2 * i}]")
    k = sym_functions(sources[103])["K"]
    assert abs(eval(k[(0, 0)]) - 2.5 * 0.64) < 1e-15 and abs(eval(k[(1, 1)]) - 1.5 * 1.21) < 1e-15
    assert sorted(re.sub(r"[-0-9.e]+ \* ", "", t) for t in k[(0, 1)].split(" + ")) == ["c[0] * c[1]", "s[0] * s[1]"]
    k = sym_functions(sources[104])["K"]
    assert abs(eval(k[(0, 1)]) / (1e-9 * 0.49) - 1) < 1e-15
    small = [t for t in k[(0, 0)].split(" + ") if t.endswith("q[0] * q[0]")]
    assert len(small) == 1 and abs(float(small[0].split(" * ")[0]) / 1e-9 - 1) < 1e-15, k[(0, 0)]


def test_size_rules_flip_the_flags(sources):
    """dT/dq: 24 operations at n = 2 is inside 12 n (111), 26 is outside (100: K stays symbolic).  grad U: 64 monomials in one component
    inside (111), 65 outside (110).  Both sides of both rules go through every value test below."""
    assert re.search(r"\((\d+) operations\): no second-order", sources[111]).group(1) == "24" and flags(sources[111]) == "111"
    assert flags(sources[112]) == "100"
    # ... for THAT reason: K of both members is a polynomial in q alone (the polar terms cancelled), so dT/dq = -1/2 v^T (dK/dq) v can be
    # counted from the emitted K -- one monomial of (degree - 1) + 2 factors, that many operations plus one, per power of q_i in an entry
    counts = {}
    for seed in (111, 112):
        ops = 0
        for e in sym_functions(sources[seed])["K"].values():
            assert "s[" not in e and "c[" not in e
            for t in ([] if e == "0.0" else e.split(" + ")):
                qs = re.findall(r"q\[(\d+)\]", t)
                ops += sum(len(qs) - 1 + 2 + 1 for i in set(qs))
        counts[seed] = ops
    assert counts == {111: 24, 112: 26}, counts
    g = sym_functions(sources[113])["gU"]
    assert max(len(e.split(" + ")) for e in g.values()) == 64 and flags(sources[113]) == "111"
    assert flags(sources[114]) == "110"


# ---------------------------------------------------------------------------------------------------------------------------------
# TEXT against the 50-digit fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [s for s in F.SEEDS if F.PROMISE[s] != "000"])
def test_emitted_text_against_the_fixtures(sources, family, seed):
    """mass_matrix_sym, dT_sym and gU_sym of every member that has them, evaluated in fp64 at every fixture point, against the fixture's
    K = J^T M J, dT = -(M J v) . ((dJ/dq_i) v) and grad U.  The tolerance is DERIVED, not measured: a sum of T monomials of degree at most
    d over sincos values correct to one ulp obeys |error| <= (T + d + 4) 2^-52 sum |coefficient * monomial|, the sum taken from the
    emitted text at that point (plus the 30 digits the fixture carries).  The sincos pairs come from each slot's operand polynomial on
    the tape, correctly rounded (symbolic_text.slot_sincos)."""
    spec = F.spec(seed)
    src = sources[seed]
    f = sym_functions(src)
    assert (f["K"] is not None) and (f["dT"] is not None) == (F.PROMISE[seed][1] == "1") and (f["gU"] is not None) == (F.PROMISE[seed][2] == "1")
    n = spec.n
    assert sorted(f["K"]) == [(a, b) for a in range(n) for b in range(a, n)]
    worst = 0.0
    for pt in family[str(seed)]["points"]:
        q, v = [float(x) for x in pt["q"]], [float(x) for x in pt["qd"]]
        s, c = slot_sincos(spec, q, src)
        env = {"q": q, "v": v, "s": s, "c": c}
        checks = [(("K", a, b), e, float(pt["K"][a][b])) for (a, b), e in f["K"].items()]
        checks += [(("dT", i), e, float(pt["dT"][i])) for i, e in (f["dT"] or {}).items()]
        checks += [(("gU", i), e, float(pt["gU"][i])) for i, e in (f["gU"] or {}).items()]
        assert len(checks) == n * (n + 1) // 2 + (n if f["dT"] else 0) + (n if f["gU"] else 0)
        size = max([1.0] + [abs(float(x)) for row in pt["K"] for x in row] + [abs(float(x)) for x in pt["dT"] + pt["gU"]])
        for what, e, want in checks:
            got, bound = eval_with_bound(e, env)
            bound += FIXTURE_DIGITS * abs(want) + FIXTURE_FLOOR * size + 2.0 ** -53 * abs(want)      # (the fixture's own error; `want` rounded to fp64)
            assert abs(got - want) <= bound, (seed, what, got, want, abs(got - want), bound)
            worst = max(worst, abs(got - want) / bound if bound else 0.0)
    print(f"symfam{seed}: worst |error| / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# KERNELS on the host: symbolic and jet builds against the fixtures, the oracle and each other
# ---------------------------------------------------------------------------------------------------------------------------------
def hameqs_at(L, pts):
    q = np.ascontiguousarray(np.stack([fvec(p["q"]) for p in pts], axis=1))
    p = np.ascontiguousarray(np.stack([fvec(pt["p"]) for pt in pts], axis=1))
    dq, dp, st = np.zeros_like(q), np.zeros_like(q), np.zeros(len(pts), np.int32)
    L.emu_hameqs(P(q), P(p), P(dq), P(dp), LL(len(pts)), I(st))
    assert not st.any()
    return dq, dp


def agree_within_twice_the_tolerance(a, b, tol):
    """Two builds within `tol` of the same truth (relative to max(1, |truth|)) are within 2 tol of each other."""
    for x, y in zip(a, b):
        scale = np.maximum(1.0, np.maximum(np.abs(x).max(0), np.abs(y).max(0)))
        assert np.all(np.abs(x - y).max(0) / scale <= 2 * tol), float(np.max(np.abs(x - y).max(0) / scale / tol))


@pytest.mark.parametrize("seed", F.SEEDS)
def test_symbolic_and_jet_kernels_on_host(emulate, oracle_lib, family, seed):
    """Both builds of the lane kernels of every member -- flags asserted from the source -- through toPhase, hamEqs, velocities and H
    against the 50-digit fixture (tol0 = 1e-12 max(1, cond / 1e3)), through RK4 steps and stepHam against the oracle, every trajectory
    (all_lanes); then hamEqs of the two builds against each other: twice the fixture tolerance."""
    spec = F.spec(seed)
    o = oracle_lib.OracleSystem(spec)
    pts = family[str(seed)]["points"]
    got = []
    for env, want in ((None, F.PROMISE[seed]), (OFF, "000")):
        L, src = emulate(spec, env)
        assert flags(src) == want, (seed, env, flags(src))
        dq, dp, tol = check_against_golden(L, spec.name, pts=pts)
        check_against_oracle(L, spec, o, B=16, start=99, dt_ham=0.02, all_lanes=True)
        got.append((dq, dp))
    agree_within_twice_the_tolerance(got[0], got[1], tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# the example systems without the symbolic right-hand side
# ---------------------------------------------------------------------------------------------------------------------------------
EXAMPLES = ["doublePendulum", "doublePendulumReadme", "pendulum", "twoBody", "spring", "threeBodyPolar", "room", "chain4", "chain6"]
GOLDEN_OF = {"doublePendulum": "byhand:doublePendulum", "doublePendulumReadme": "byhand:doublePendulumReadme", "pendulum": "byhand:pendulum",
             "twoBody": "byhand:twoBody", "spring": "byhand:spring", "room": "byhand:room", "threeBodyPolar": "threeBodyPolar", "chain4": "chain4"}


@pytest.mark.parametrize("name", EXAMPLES)
def test_example_systems_with_symbolic_off_on_host(emulate, oracle_lib, name):
    """HAMK_K_SYMBOLIC=0: the jets these systems ran on before the symbolic right-hand side, and that no default build runs any more --
    against the by-hand 50-digit fixtures where there are some, the derived ones otherwise (chain6 has none: oracle only), and the oracle."""
    spec = E.get(name)
    L, src = emulate(spec, OFF)
    assert flags(src) == "000"
    Ld, srcd = emulate(spec)
    assert flags(srcd)[0] == "1"                                    # (what the default build takes: the switch is what turned it off)
    if name in GOLDEN_OF:
        dq, dp, tol = check_against_golden(L, GOLDEN_OF[name])
        from conftest import load_golden
        agree_within_twice_the_tolerance((dq, dp), hameqs_at(Ld, load_golden(GOLDEN_OF[name])["points"]), tol)
    check_against_oracle(L, spec, oracle_lib.OracleSystem(spec), qd_kick=0.4 if name.startswith("chain") else 0.0)


@pytest.mark.parametrize("mode", ["H", "D", "R"])
@pytest.mark.parametrize("name", EXAMPLES[:6])
def test_ad_modes_of_the_example_systems_with_symbolic_off_on_host(emulate, oracle_lib, name, mode):
    """HAMK_AD_MODE = H, D, R with HAMK_K_SYMBOLIC=0: the MODE_* lines name what runs only where no HAS_SYM_* flag overrides them
    (hamk_device.hpp ham_eqs takes the symbolic branch first) -- asserted, then values against the fixtures and the oracle."""
    spec = E.get(name)
    L, src = emulate(spec, {"HAMK_K_SYMBOLIC": "0", "HAMK_AD_MODE": mode})
    assert flags(src) == "000"
    assert ("MODE_H = true" in src) == (mode == "H") and ("MODE_R = true" in src) == (mode == "R")
    check_against_golden(L, GOLDEN_OF[name])
    check_against_oracle(L, spec, oracle_lib.OracleSystem(spec), B=24)
