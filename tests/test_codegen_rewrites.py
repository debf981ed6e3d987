"""CPU: the three rewrites the tape -> C++ generator applies node by node (hamk_codegen.cpp emit_body) -- shared exponentials, the fused
1 / sqrt, the sincos slots -- on the family of tests/rewrite_family.py, one member per branch.

  * SOURCE: what each member promises (rewrite_family.PROMISE: how many hamk::exp( and hamk::rsqrt_of( calls each generated function
    keeps, how many sincos slots, which of f's slots the potential reuses) is asserted on the generated C++ of the default build, of
    AD modes R, H and D, and of the four-lane and wave mappings forced through the ABI's options.
  * VALUES: the lane, four-lane and wave kernels of every member on the host (tests/test_host_emulation.py) against the 50-digit
    fixtures of tests/golden/rewrite_family.json (oracle/gen_golden_rewrites.py) and against the oracle, which evaluates the tape as
    written: hamEqs, momenta, energies, three RK4 steps and one stepHam with identical sub-step counts on every trajectory.  No point
    and no trajectory is left out (cond K < 1e3 everywhere by the 50-digit reference) and no status bit may be set.

Tolerances are the project's ladder (tests/test_gpu_parity.py T1 max(1, cond / 1e3) against the fixtures, the helpers' own arguments
against the oracle).  They hold for a shared exponential because an exponential's relative sensitivity to its argument is |argument|,
and an argument built by k fp64 operations carries at most k 2^-53 |argument|: 8e-14 at |argument| <= 135 and k <= 5.

The RANGE members are the reason the generator evaluates the member with the LARGEST offset of a group and derives the others with a
factor <= 1.  Before that rule the first member on the tape was evaluated: in `range_low_small_first` that was exp(q0 - 735), a subnormal
number of some twelve significant bits, and exp(q0 - 135) -- the term of order one -- was that times e^600: wrong from the fifth digit,
with no status bit set (measured against the fixtures: see test_range_members_evaluate_the_largest_offset)."""
import json
import os
import re

import pytest

import rewrite_family as F
from conftest import GOLDEN
from test_host_emulation import check_against_golden, check_against_oracle, emulate, emulate_quad, emulate_wave  # noqa: F401  (fixtures)


@pytest.fixture(scope="module")
def family():
    with open(os.path.join(GOLDEN, "rewrite_family.json")) as fh:
        return json.load(fh)["blocks"]


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    return _api


def variants():
    from hamilton_amd import _abi
    return {"default": None, "R": {"ad_mode": _abi.AD_R}, "H": {"ad_mode": _abi.AD_H}, "D": {"ad_mode": _abi.AD_D},
            "quad": {"mapping": _abi.MAP_QUAD}, "wave": {"mapping": _abi.MAP_WAVE}}


MARKER = {"default": "HAMK_INSTANTIATE(HamkSys)", "R": "MODE_R = true", "H": "MODE_H = true", "D": "MODE_H = false",
          "quad": "HAMK_INSTANTIATE_QUAD", "wave": "HAMK_INSTANTIATE_WAVE"}


def check_promise(key, src):
    got, want = F.found(src), F.PROMISE[key]
    assert {k: got[k] for k in want} == want, (key, got)
    # the same two tapes in their other places: f with a sink (the same rewrites: a sink output is an output), f followed by U
    assert got["exp_sink"] == (want["exp"][0], sum(want["exp"])), (key, got)
    assert got["rsqrt_sink"] == (want["rsqrt"][0], sum(want["rsqrt"])), (key, got)
    assert got["shares_f_trig"] == bool(want["trig"][2]) and got["exp_after_f"] == (want["exp"][1] if want["trig"][2] else 0), (key, got)


# ---------------------------------------------------------------------------------------------------------------------------------
# SOURCE
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_family_is_complete(family):
    """One fixture block per member, every point with cond K < 1e3 and a non-zero velocity; n <= 3, m <= 4; the range members carry the
    four corners of their box; every counter of PROMISE is non-zero somewhere and zero somewhere."""
    assert sorted(family) == sorted(F.KEYS) and sorted(F.PROMISE) == sorted(F.KEYS)
    for key in F.KEYS:
        spec, pts = F.spec(key), family[key]["points"]
        assert spec.n <= 3 and spec.m <= 4 and len(pts) == (10 if key in F.RANGE_KEYS else 6), key
        assert all(float(pt["cond_hint"]) < 1e3 for pt in pts), key
        assert all(all(float(x) != 0.0 for x in pt["qd"]) for pt in pts), key
        if key in F.RANGE_KEYS:
            assert sorted((float(pt["q"][0]), float(pt["qd"][0])) for pt in pts[6:]) == [(-1.0, -1.0), (-1.0, 1.0), (1.0, -1.0), (1.0, 1.0)]
    for pick in (lambda p: p["exp"][0], lambda p: p["exp"][1], lambda p: p["rsqrt"][0], lambda p: p["rsqrt"][1], lambda p: p["trig"][0],
                 lambda p: p["trig"][1], lambda p: len(p["trig"][2])):
        vals = {pick(F.PROMISE[k]) for k in F.KEYS}
        assert 0 in vals and len(vals) >= 2


@pytest.mark.parametrize("key", F.KEYS)
def test_source_keeps_its_promise_in_every_build(api, key):
    """The default build, AD modes R, H and D, the four-lane and the wave mapping (both put f's outputs through a sink), every member."""
    spec = F.spec(key)
    for name, opt in variants().items():
        src = api.system_from_spec(spec, opt).source
        assert MARKER[name] in src and ("MODE_R = true" in src) == (name == "R"), (key, name)
        check_promise(key, src)


def test_what_the_tapes_hold():
    """The members reach the branch they are named after: the opcode and the side of the constant, read from the recorded tape."""
    from hamilton_amd import tracer as T

    def exp_args(key):
        _, tu = F.spec(key).trace()
        return tu.ops, [tu.ops[a] for op, a, _, _ in tu.ops if op == T.OP_EXP]
    const = lambda ops, i: ops[i][0] == T.OP_CONST
    ops, args = exp_args("exp_add")
    assert sorted((const(ops, a), const(ops, b)) for op, a, b, _ in args) == [(False, True), (True, False)] and all(op == T.OP_ADD for op, *_ in args)
    ops, args = exp_args("exp_sub_right")
    assert all(op == T.OP_SUB and const(ops, b) for op, a, b, _ in args)
    ops, args = exp_args("exp_sub_left")
    assert sorted(op for op, *_ in args) == sorted([T.OP_SUB, T.OP_ADD]) and all(const(ops, a) for op, a, b, _ in args if op == T.OP_SUB)
    ops, args = exp_args("exp_mul")
    muls = [o for o in ops if o[0] == T.OP_MUL and (const(ops, o[1]) != const(ops, o[2])) and 0.7 in (ops[o[1]][3], ops[o[2]][3])]
    assert sorted(const(ops, o[1]) for o in muls) == [False, True]
    ops, args = exp_args("exp_div")
    assert sorted(op for op, *_ in args) == sorted([T.OP_DIV, T.OP_ADD]) and all(const(ops, b) for op, a, b, _ in args if op == T.OP_DIV)
    ops, args = exp_args("exp_neg")
    assert all(op == T.OP_NEG for op, *_ in args)
    ops, args = exp_args("exp_logistic")
    assert all(op == T.OP_NEG and ops[a][0] == T.OP_MUL for op, a, _, _ in args) and len(args) == 2
    assert len(exp_args("exp_three")[1]) == 3 and len(exp_args("exp_four")[1]) == 4 and len(exp_args("range_chain")[1]) == 3
    for key in ("rsqrt_u",):
        ops, _ = exp_args(key)
        assert any(op == T.OP_RECIP and ops[a][0] == T.OP_SQRT for op, a, _, _ in ops)
    _, tu = F.spec("rsqrt_div").trace()
    assert any(op == T.OP_DIV and tu.ops[b][0] == T.OP_SQRT for op, a, b, _ in tu.ops) and not any(op == T.OP_RECIP for op, *_ in tu.ops)
    tf, _ = F.spec("rsqrt_sqrt_output").trace()
    sq = [i for i, o in enumerate(tf.ops) if o[0] == T.OP_SQRT]
    assert len(sq) == 1 and sq[0] in tf.outs and sum(1 for o in tf.ops if o[0] == T.OP_RECIP and o[1] == sq[0]) == 1
    assert sum(1 for o in tf.ops if o[0] not in (T.OP_CONST, T.OP_INPUT) and sq[0] in (o[1:3] if o[0] in (T.OP_ADD, T.OP_SUB, T.OP_MUL, T.OP_DIV) else o[1:2])) == 1


def evaluated_offsets(src):
    """The constant offsets of the arguments `in[0] + c` of the exponentials that `potential` evaluates."""
    body = F.functions(src)["potential"]
    out = []
    for arg in re.findall(r"= hamk::exp\((u\d+)\);", body):
        c = re.search(rf"const auto {arg} = in\[0\] \+ (u\d+);", body).group(1)
        out.append(float.fromhex(re.search(rf"const double {c} = \(?(-?0x[0-9a-fp.+-]+)\)?;", body).group(1)))
    return out


def test_range_members_evaluate_the_largest_offset(api):
    """Whichever order U writes its two exponentials in, the ONE that is evaluated is the one with the larger offset (exp(q0 - 135), not
    the subnormal exp(q0 - 735); exp(q0 + 705), not exp(q0 + 105)): the derived one is never larger than the evaluated one.  Offsets 601
    apart do not share; of three members at 0, -350 and -700 the last is evaluated itself, not derived from the derived one.

    With the first member on the tape evaluated instead (the rule before this family existed), range_low_small_first has
    max |dp - fixture| / max(1, |fixture|) between 3.0e-9 and 3.5e-5 (at q0 = -0.385) over its ten fixture points on the host
    emulation -- lane, four-lane and wave kernels alike -- against a tolerance of 1e-12, and status 0 everywhere; the other range
    members are within 7e-14 under either rule."""
    for key, want in F.RANGE_EVALUATED_OFFSET.items():
        for opt in variants().values():
            assert evaluated_offsets(api.system_from_spec(F.spec(key), opt).source) == [want], key
    assert sorted(evaluated_offsets(api.system_from_spec(F.spec("range_beyond_limit")).source)) == [-650.0, -49.0]
    src = api.system_from_spec(F.spec("range_chain")).source
    body = F.functions(src)["potential"]
    derived = re.findall(r"const auto u\d+ = (u\d+) \* (0x[0-9a-fp.+-]+);", body)
    evaluated = re.findall(r"const auto (u\d+) = hamk::exp\(", body)
    assert len(evaluated) == 2 and len(derived) == 1 and derived[0][0] in evaluated and 0.0 < float.fromhex(derived[0][1]) <= 1.0


def test_every_derived_exponential_is_scaled_down(api):
    """In every member and build: a derived exponential is an EVALUATED one times a constant in [e^-600, 1]."""
    for key in F.KEYS:
        src = api.system_from_spec(F.spec(key)).source
        for name, body in F.functions(src).items():
            if name not in ("coords", "potential", "potential_after_f", "coords_sink", "coords_sink_u"):
                continue
            evaluated = set(re.findall(r"const auto ([fu]\d+) = hamk::exp\(", body))
            for base, factor in re.findall(r"const auto [fu]\d+ = ([fu]\d+) \* (0x[0-9a-fp.+-]+);", body):
                assert base in evaluated and 2.6e-261 < float.fromhex(factor) <= 1.0, (key, name, base, factor)


def test_spring_and_room_keep_their_sharing(api):
    """The systems the sharing was made for: spring's two walls are one evaluation, room's four are two (one per coordinate) -- in
    `potential` and in `potential_after_f` alike; the headline system has no exponential at all."""
    from hamilton_amd import examples as E
    for name, n in (("spring", 1), ("room", 2), ("doublePendulum", 0)):
        got = F.found(api.system_from_spec(E.get(name)).source)
        assert got["exp"] == (0, n) and got["exp_sink"] == (0, n), (name, got)
    assert F.found(api.system_from_spec(E.get("spring")).source)["exp_after_f"] == 1


# ---------------------------------------------------------------------------------------------------------------------------------
# VALUES on the host
# ---------------------------------------------------------------------------------------------------------------------------------
def steppers_set_no_status(L, spec, o, pts):
    """The status words the steppers write (check_against_oracle reads the one of hamEqs only): three RK4 steps and one stepHam from the
    fixture points and from the ensemble check_against_oracle uses -- no bit set, every state finite."""
    import ctypes
    import numpy as np
    from conftest import fvec
    from hamilton_amd import examples as E
    from test_host_emulation import I, LL, P
    q0 = np.ascontiguousarray(np.stack([fvec(pt["q"]) for pt in pts], axis=1))
    p0 = np.ascontiguousarray(np.stack([fvec(pt["p"]) for pt in pts], axis=1))
    qe, qde = E.sample_config(spec, 99, 16)
    for q, p in ((q0, p0), (qe, o.to_phase_batch(qe, qde))):
        B = q.shape[1]
        for step in ("rk4", "ham"):
            q1, p1, st, ns = q.copy(), p.copy(), np.full(B, -1, np.int32), np.zeros(B, np.int32)
            if step == "rk4":
                L.emu_rk4(P(q1), P(p1), LL(B), ctypes.c_double(spec.dt), 3, I(st))
            else:
                L.emu_step_ham(P(q1), P(p1), LL(B), ctypes.c_double(0.02), I(st), I(ns))
            assert not st.any() and np.isfinite(q1).all() and np.isfinite(p1).all(), (spec.name, step, st)


def run(L, spec, o, pts, tol):
    check_against_golden(L, spec.name, pts=pts)
    check_against_oracle(L, spec, o, B=16, start=99, dt_ham=0.02, all_lanes=True, tol=tol)
    steppers_set_no_status(L, spec, o, pts)


@pytest.mark.parametrize("key", F.KEYS)
def test_lane_kernels_on_host(emulate, oracle_lib, family, key):
    spec = F.spec(key)
    L, src = emulate(spec)
    check_promise(key, src)
    run(L, spec, oracle_lib.OracleSystem(spec), family[key]["points"], 1e-11)


@pytest.mark.parametrize("mode", ["R", "H", "D"])
@pytest.mark.parametrize("key", F.FUSED_KEYS)
def test_fused_rsqrt_under_every_ad_mode_on_host(emulate, oracle_lib, family, key, mode):
    """hamk::rsqrt_of at Jet1, JetH / Jet2 and in plain doubles next to the generated reverse sweep (which has its own rules)."""
    spec = F.spec(key)
    L, src = emulate(spec, {"HAMK_AD_MODE": mode})
    assert MARKER[mode] in src and ("MODE_R = true" in src) == (mode == "R")
    check_promise(key, src)
    run(L, spec, oracle_lib.OracleSystem(spec), family[key]["points"], 1e-11)


# the cooperative mappings against the oracle at 1e-10, as everywhere in tests/test_host_emulation.py (their K = J^T M J is summed in
# another order); against the fixtures at the ladder
@pytest.mark.parametrize("key", F.KEYS)
def test_quad_kernels_on_host(emulate_quad, oracle_lib, family, key):
    spec = F.spec(key)
    run(emulate_quad(spec), spec, oracle_lib.OracleSystem(spec), family[key]["points"], 1e-10)


@pytest.mark.parametrize("key", F.KEYS)
def test_wave_kernels_on_host(emulate_wave, oracle_lib, family, key):
    spec = F.spec(key)
    run(emulate_wave(spec, True), spec, oracle_lib.OracleSystem(spec), family[key]["points"], 1e-10)
