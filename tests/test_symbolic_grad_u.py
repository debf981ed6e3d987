"""The generator's symbolic grad U (hamk_codegen.cpp symbolic_mass_matrix, gU_sym): where U . f is a polynomial over q and the sincos
pairs of f -- and the system takes K and dT/dq symbolically -- dU/dq is emitted as polynomials and the right-hand side needs no
first-order sweep.  CPU checks: which systems get it, its VALUES against the oracle's grad U, the format of the emitted text, and that K
and dT/dq keep the text they had (their roundings, and with them the headline kernel's results, do not move)."""
import re

import numpy as np
import pytest

from hamilton_amd import examples as E
from symbolic_text import HEX, as_python, emitted, trig_input_table

SYMBOLIC = ["pendulum", "doublePendulum", "doublePendulumReadme", "room", "twoBody", "spring", "threeBodyPolar", "chain4", "chain6"]
# polynomial U AND symbolic dT/dq.  room, spring: exponentials; twoBody: 1 / r; threeBodyPolar: square roots; chain4, chain6: the
# pendulums' polynomial U, but their dT/dq keeps the second-order sweep and grad U rides on its first-order part (the generator's rule)
WITH_GRAD_U = ["pendulum", "doublePendulum", "doublePendulumReadme"]


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    return _api


@pytest.mark.parametrize("name", SYMBOLIC)
def test_symbolic_grad_u_against_the_oracle(api, oracle_lib, name):
    """gU_sym at random points against the oracle's grad U (first-order forward AD of U . f), every component to 1e-13 RELATIVE
    (T1): a component is one rounded product of a literal and a sincos value here, so it has no cancellation to excuse."""
    spec = E.get(name)
    src = api.system_from_spec(spec).source
    g = emitted(src, "gU_sym")
    assert (g is not None) == (name in WITH_GRAD_U) == ("HAS_SYM_GU = true" in src)
    if g is None:
        return
    assert sorted(g) == ["gU[%d]" % i for i in range(spec.n)]
    o = oracle_lib.OracleSystem(spec)
    slots = trig_input_table(src)
    qs, _ = E.sample_config(spec, 31, 64)
    for k in range(qs.shape[1]):
        q = [float(x) for x in qs[:, k]]
        s, c = [float(np.sin(q[j])) for j in slots], [float(np.cos(q[j])) for j in slots]
        ref = np.asarray(o.grad_pe(np.array(q)), dtype=float)
        got = np.array([eval(as_python(g["gU[%d]" % i]), {"q": q, "s": s, "c": c}) for i in range(spec.n)])
        print(name, "grad U relative differences", np.abs(got - ref) / np.abs(ref))
        assert np.all(np.abs(got - ref) <= 1e-13 * np.abs(ref)), (name, q, got, ref)


@pytest.mark.parametrize("name", WITH_GRAD_U)
def test_the_emitted_format(api, name):
    """One self-contained expression per component over q[], tc.s[], tc.c[] with + * ( ) and hex-float literals only; a literal touches a
    parenthesis only where it is parenthesised alone (what tests/test_symbolic_k.py's substitution relies on)."""
    g = emitted(api.system_from_spec(E.get(name)).source, "gU_sym")
    for target, e in g.items():
        rest = re.sub(r"\b(q|tc\.s|tc\.c)\[\d+\]", "X", re.sub(HEX, "L", e))
        assert re.fullmatch(r"[LX+*() ]+|0\.0", rest), (name, target, e)
        for m in re.finditer(HEX, e):
            assert e[:m.start()].endswith("(") == e[m.end():].startswith(")"), (name, target, e)
        eval(as_python(e), {"q": [0.5] * 8, "s": [0.6] * 8, "c": [0.8] * 8})


def test_the_double_pendulum_text(api):
    """grad U folds to one literal per component (the Jet1 sweep left 5 (s + s) and 5 (-1/2 -s) to the compiler); K and dT/dq are the sums
    of monomials they were."""
    src = api.system_from_spec(E.get("doublePendulum")).source
    assert emitted(src, "gU_sym") == {"gU[0]": "0x1.4p+3 * tc.s[0]", "gU[1]": "0x1.4p+1 * tc.s[1]"}
    assert emitted(src, "mass_matrix_sym")["K[0][1]"] == "0x1p-1 * tc.s[0] * tc.s[1] + 0x1p-1 * tc.c[0] * tc.c[1]"
    dT = emitted(src, "dT_sym")
    assert dT["dT[0]"] == "0x1p-1 * tc.s[0] * tc.c[1] * v[0] * v[1] + (-0x1p-1) * tc.c[0] * tc.s[1] * v[0] * v[1]"
    assert dT["dT[1]"] == "(-0x1p-1) * tc.s[0] * tc.c[1] * v[0] * v[1] + 0x1p-1 * tc.c[0] * tc.s[1] * v[0] * v[1]"
