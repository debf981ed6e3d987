"""CPU: rectangular coordinate maps (m != n) on every kernel mapping -- the family of tests/rect_family.py, one member per branch a
kernel takes on m against a size derived from n (the table is in that module).

  * SOURCE: the mapping each member resolves to (`options()["mapping"]`) and whether its module is the four-lane DENSE path
    (`QUAD_DENSE = true`) are asserted from the build the table asks for; the module the host emulation compiles is that build's text.
  * CAPACITY: the dense four-lane path keeps dU/dx of a cartesian potential in 2 NP4 rows of LDS (hamk_quad.hpp assemble_dense).  `qd_last`
    (m = 2 NP4) is the last size it holds; `qd_over` (one more output) is created on the wave kernels when the mapping is left to the
    library and REFUSED with HAMK_ERR_UNSUPPORTED, in a sentence that names the limit, when the host states HAMK_MAP_QUAD.  Before the
    capacity condition hamk_system_create failed on both with HAMK_ERR_COMPILE (a static assertion inside hiprtc's log).
  * VALUES on the host emulation (tests/test_host_emulation.py: one OS thread per lane, real barriers -- where the order of dU/dx and
    dU/dq in the rows of GU is checked without a GPU): every member on its kernel at B = 5 against the 50-digit fixtures of
    tests/golden/rect_family.json and against the oracle on every trajectory: hamEqs, toPhase / fromPhase, the energy observables, three
    RK4 steps, one stepHam(0.1) with the oracle's sub-step counts; every status word any entry point writes is zero.

tests/golden/rect_family.json is written by oracle/gen_golden_rect.py; re-running it reproduces the file byte for byte.

Tolerances are the rule of tests/test_codegen_rewrites.py and tests/test_symbolic_rhs.py, unchanged: 1e-12 max(1, cond_hint / 1e3) against
the fixtures; against the oracle 1e-11 (lane kernels) and 1e-10 (the cooperative mappings, whose K = J^T M J is summed in another order)
times max(1, cond K / 100), ten times that after the RK4 steps and a hundred times after stepHam.  No member needed more."""
import ctypes
import json
import os

import numpy as np
import pytest

import rect_family as F
from conftest import GOLDEN
from test_host_emulation import check_against_golden, check_against_oracle, emulate, emulate_quad, emulate_wave  # noqa: F401  (fixtures)

B_HOST = 5
DT_HAM = 0.1
MARKER = {"lane": "HAMK_INSTANTIATE(HamkSys)", "quad": "HAMK_INSTANTIATE_QUAD", "wave": "HAMK_INSTANTIATE_WAVE"}
RUN_IDS = [f"{key}-{ask or 'auto'}" for key, ask in F.RUNS]


def points(block):
    """The fixture points of one member in the layout check_against_golden reads: `vel` is stored once and is also the qd the momenta
    were made from and the dq of hamEqs (oracle/gen_golden_rect.py asserts the three equal at 30 digits)."""
    return [dict(pt, qd=pt["vel"], dq=pt["vel"]) for pt in block["points"]]


@pytest.fixture(scope="module")
def family():
    with open(os.path.join(GOLDEN, "rect_family.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    return _api


class StatusWatch:
    """A driver library whose every call's status array (the first int32 pointer argument of each emu_* entry point) is kept."""

    def __init__(self, lib):
        self._lib, self.seen = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*args):
            r = fn(*args)
            count = next(int(a.value) for a in args if isinstance(a, ctypes.c_longlong))
            st = next((a for a in args if isinstance(a, ctypes.POINTER(ctypes.c_int32))), None)
            if st is not None:
                self.seen.append((name, np.ctypeslib.as_array(st, (count,)).copy()))
            return r
        return call


# ---------------------------------------------------------------------------------------------------------------------------------
# the family and its fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fixture_header_lists_the_family(family):
    """The member list in the header of rect_family.json is the family's, block by block: n, m, inertias, four points, each with
    cond K < 1e4 by the 50-digit reference and a non-zero velocity.  The shapes are the table's: m != n except the control."""
    assert family["members"] == F.KEYS and sorted(family["blocks"]) == sorted(F.KEYS)
    assert family["generator"].startswith("oracle/gen_golden_rect.py")
    for key in F.KEYS:
        spec, blk = F.spec(key), family["blocks"][key]
        assert (blk["system"], blk["n"], blk["m"], blk["inertia"]) == (spec.name, spec.n, spec.m, list(spec.inertia)), key
        assert len(blk["points"]) == F.NPOINTS == 4 and all(w > 0.0 for w in spec.inertia), key
        assert sorted(blk["points"][0]) == sorted(["q", "p", "vel", "dp", "pe", "keP", "hamiltonian", "cond_hint"]), key
        assert all(float(pt["cond_hint"]) < F.COND_LIMIT for pt in blk["points"]), key
        assert all(all(float(x) != 0.0 for x in pt["vel"]) for pt in blk["points"]), key
        assert (spec.m != spec.n) == (key != "ln_thin") and spec.m <= 128 and spec.n <= 33, key
    n4 = F.np4
    shape = lambda key: (F.spec(key).n, F.spec(key).m)
    n, m = shape("qd_eq")
    assert m == n4(n) and n4(n) != n
    n, m = shape("qd_first_gu")
    assert m == n4(n) + 1
    n, m = shape("qd_last")
    assert m == 2 * n4(n) and n4(n) == n
    n, m = shape("qd_over")
    assert m == 2 * n4(n) + 1
    assert shape("qd_gen")[1] == 3 * shape("qd_gen")[0] and shape("qb_wide")[1] == 3 * shape("qb_wide")[0]
    assert shape("qb_max")[1] == shape("wv_max")[1] == shape("ln_wide_c")[1] == 128
    assert shape("wv_odd")[0] > 32 and shape("wv_odd")[1] % 4 != 0 and shape("ln_wide_g") == (16, 33)


# ---------------------------------------------------------------------------------------------------------------------------------
# SOURCE
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,ask", F.RUNS, ids=RUN_IDS)
def test_source_promises(api, key, ask):
    """The build the table asks for resolves to the table's mapping, is (or is not) the dense four-lane module, and is the text the host
    emulation compiles (the emulate* fixtures state the mapping; stating it changes nothing in the generated source)."""
    spec = F.spec(key)
    s = api.system_from_spec(spec, F.options(ask))
    want = F.runs_on(key)
    assert s.options()["mapping"] == F.mapping_code(want), (key, ask, s.options()["mapping"])
    assert MARKER[want] in s.source and sum(mk in s.source for mk in MARKER.values()) == 1, (key, ask)
    assert ("QUAD_DENSE = true" in s.source) == F.quad_dense(key), (key, ask)
    if want == "quad":
        assert ("QUAD_DENSE = false" in s.source) != F.quad_dense(key), (key, ask)
    assert s.source == api.system_from_spec(spec, F.options(want)).source, (key, ask)
    assert (s.m, s.n) == (spec.m, spec.n) and f"M = {spec.m}" in s.source and f"N = {spec.n}" in s.source


def test_dense_quad_capacity_under_auto_and_forced(api):
    """Both halves of the capacity condition (hamk_dispatch.cpp quad_dense_holds, check_options).  qd_over -- 41 outputs over 20
    coordinates, one more than the 2 NP4 = 40 rows of LDS that hold dU/dx -- under AUTO: created, on the wave kernels.  With
    HAMK_MAP_QUAD stated: refused with HAMK_ERR_UNSUPPORTED and a sentence naming the limit, not with a compiler's log.  On either
    side of it nothing changes: qd_last (m = 40) is built on the dense quad path under AUTO and stated, qd_gen (m = 54, generalized U:
    no dU/dx to store) likewise, and the wide BANDED map of qb_max (m = 128) is no business of the dense path's limit."""
    from hamilton_amd import _abi
    spec = F.spec("qd_over")
    s = api.system_from_spec(spec)
    assert s.options()["mapping"] == _abi.MAP_WAVE and s.options(193)["mapping"] == _abi.MAP_WAVE
    assert MARKER["wave"] in s.source and s.code_size > 0
    with pytest.raises(_abi.HamkError) as e:
        api.system_from_spec(spec, {"mapping": _abi.MAP_QUAD})
    msg = str(e.value)
    assert e.value.code == _abi.HAMK_ERR_UNSUPPORTED, msg
    assert "HAMK_MAP_QUAD" in msg and "2 * NP4 = 40" in msg and "m = 41" in msg and "n = 20" in msg, msg
    assert "hiprtc" not in msg and "static assertion" not in msg and "error:" not in msg, msg
    assert api.system_from_spec(spec, {"mapping": _abi.MAP_WAVE}).source == s.source
    for key in ("qd_last", "qd_gen", "qb_max"):
        for opt in (None, {"mapping": _abi.MAP_QUAD}):
            t = api.system_from_spec(F.spec(key), opt)
            assert t.options()["mapping"] == _abi.MAP_QUAD and ("QUAD_DENSE = true" in t.source) == F.quad_dense(key), (key, opt)


# ---------------------------------------------------------------------------------------------------------------------------------
# VALUES on the host emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def run_member(lib, spec, o, pts, tol):
    """Fixtures, then the oracle on every one of B_HOST trajectories (all_lanes: hamEqs status zero, identical sub-step counts), then every
    status word any of those calls wrote -- the steppers' and the observables' included -- is zero."""
    L = StatusWatch(lib)
    q, _ = __import__("hamilton_amd.examples", fromlist=["examples"]).sample_config(spec, 99, B_HOST)
    cond = [np.linalg.cond(o.jacobian(q[:, i]).T @ np.diag(spec.inertia) @ o.jacobian(q[:, i])) for i in range(B_HOST)]
    assert max(cond) < F.COND_LIMIT, (spec.name, cond)
    check_against_golden(L, spec.name, pts=pts)
    check_against_oracle(L, spec, o, B=B_HOST, start=99, steps=3, dt_ham=DT_HAM, all_lanes=True, tol=tol)
    called = {name for name, _ in L.seen}
    assert {"emu_hameqs", "emu_from_phase", "emu_observe", "emu_rk4", "emu_step_ham"} <= called, called
    for name, st in L.seen:
        assert not st.any(), (spec.name, name, st)


@pytest.mark.parametrize("key,ask", F.RUNS, ids=RUN_IDS)
def test_member_on_host_emulation(emulate, emulate_quad, emulate_wave, oracle_lib, api, family, key, ask):
    spec = F.spec(key)
    want = F.runs_on(key)
    asked_src = api.system_from_spec(spec, F.options(ask)).source
    if want == "lane":
        lib, src = emulate(spec)
        assert src == asked_src
    elif want == "quad":
        lib = emulate_quad(spec)
    else:
        lib = emulate_wave(spec, True)
    assert MARKER[want] in asked_src
    run_member(lib, spec, oracle_lib.OracleSystem(spec), points(family["blocks"][key]), 1e-11 if want == "lane" else 1e-10)
