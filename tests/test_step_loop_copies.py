"""Register copies in the double pendulum's RK4 stepping loop, counted from the gfx950 code object (a cross-compile and llvm-objdump
through scripts/isa_stats.py; no GPU).  The module is built with -DHAMK_PROBE_NO_SLOWPATH, which removes the bodies of the rare branches,
so the hottest loop of hamk_rk4_steps_k is one RK4 step of a healthy lane.

With HAMK_STEP_CONST_VGPR (hamk_device.hpp StepK: the loop's addend constants and grad U's coefficients parked in vector registers, the
step's last combination as a three-address FMA) the loop holds NO v_mov_b64 and 264 VALU instructions, 257 of them fp64 -- the same 257
as without: only copies went.  Without the define the probe build of this toolchain (ROCm 7.2 hiprtc) has 7 copies in 271 VALU
instructions: four VGPR -> VGPR copies in front of the grad U pairs and three loop-carried y <- acc copies; the seven SGPR -> VGPR
constant copies that an earlier count of this loop reported (14 in 278) are hoisted out of the PROBE build's loop by the compiler
itself here and show only in the shipped build, whose slow-path branches leave it short of scalar registers (a healthy lane's path
through it: 295 VALU / 21 copies without the define).  The figures below pin both forms."""
import os
import sys

import pytest

from hamilton_amd import examples as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import isa_stats  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_stats.OBJDUMP), reason="llvm-objdump not installed")


@pytest.fixture(scope="module")
def api(hamk_lib):
    from hamilton_amd import api as _api
    return _api


def probe_loop(api, name, opt):
    """Mnemonics of the hottest loop of hamk_rk4_steps_k in the probe build of `name` with hamk_options::step_const_vgpr = opt."""
    from hamilton_amd import _abi
    env = {"HAMK_TEST_OVERRIDES": "1", "HAMK_HIPRTC_FLAGS": "-DHAMK_PROBE_NO_SLOWPATH"}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = api.system_from_spec(E.get(name), _abi.HamkOptions(step_const_vgpr=opt, mapping=_abi.MAP_LANE))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    info = {l.split()[0]: l.split()[1] for l in s.build_info.splitlines() if l}
    ins = isa_stats.disassemble(s.code_object(1 if "no-machine-licm" in info["hamk_rk4_steps_k"] else 0))["hamk_rk4_steps_k"]
    lo, hi = isa_stats.hottest_loop(ins)
    return s, [mn for _, mn, _ in ins[lo:hi + 1]], isa_stats.loop_stats(ins)


def test_the_stepping_loop_holds_no_register_copies(api):
    from hamilton_amd import _abi
    s, loop, st = probe_loop(api, "doublePendulum", _abi.ON)
    assert "#define HAMK_STEP_CONST_VGPR 1" in s.source and "gU_sym_k" in s.source
    copies = sum(1 for mn in loop if mn.startswith("v_mov_b64"))
    print("on: v_mov_b64", copies, "VALU", st["valu"], "fp64", st["valu_f64"])
    assert copies == 0
    assert st["valu"] <= 264
    assert st["valu_f64"] == 257
    assert not any(mn.startswith("scratch_") for mn in loop)


def test_the_form_without_the_define_is_the_parents(api):
    from hamilton_amd import _abi
    s, loop, st = probe_loop(api, "doublePendulum", _abi.OFF)
    assert "HAMK_STEP_CONST_VGPR" not in s.source and "gU_sym_k" not in s.source
    copies = sum(1 for mn in loop if mn.startswith("v_mov_b64"))
    print("off: v_mov_b64", copies, "VALU", st["valu"], "fp64", st["valu_f64"])
    assert copies == 7 and st["valu"] == 271 and st["valu_f64"] == 257
    assert not any(mn.startswith("scratch_") for mn in loop)


def test_the_parked_forms_are_the_same_sums(api):
    """mass_matrix_sym_k / gU_sym_k are mass_matrix_sym / gU_sym term for term, with gk[i] standing for the i-th literal of
    HAMK_GEN_PARK_LIST."""
    import re
    from symbolic_text import emitted
    src = api.system_from_spec(E.get("doublePendulum")).source
    gk = re.search(r"#define HAMK_GEN_PARK_LIST (.*)", src).group(1).split(", ")
    assert len(gk) == int(re.search(r"#define HAMK_GEN_PARK_N (\d+)", src).group(1)) == 3
    for fn in ("mass_matrix_sym", "gU_sym"):
        m = re.search(r"static void %s_k\(const double \(&q\)\[N\].*?\{\n(.*?)\n  \}" % fn, src, re.S)
        parked = {t: e for t, e in re.findall(r"^\s*(\w+(?:\[\d+\])+) = ([^;]*);", m.group(1), re.M)}
        plain = emitted(src, fn)
        assert sorted(parked) == sorted(plain)
        for t, e in parked.items():
            assert re.sub(r"gk\[(\d+)\]", lambda k: gk[int(k.group(1))], e) == plain[t], (fn, t)
