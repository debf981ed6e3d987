"""CPU, text only: hamilton_amd/csrc/hamk_fused_rk4.hpp, what the three kernels fused with classic RK4 share (hamk_lyap.hpp,
hamk_psec.hpp, hamk_exit.hpp): it holds the step and the root finder on RK4's continuous extension ONCE, and it obeys the rule
tests/test_exit.py::test_the_step_loop_has_no_barrier_and_no_lds holds hamk_exit.hpp to, because hamk_exit.hpp's step loop --
which wavefronts of one block leave at different steps -- calls into it."""
import re

import test_kernel_signatures as KS

COMPANIONS = ("hamk_lyap.hpp", "hamk_psec.hpp", "hamk_exit.hpp")
SHARED = "hamk_fused_rk4.hpp"
NEWTON = 4


def code(name):
    return re.sub(r"//[^\n]*", "", KS._text(name))


def test_the_shared_header_has_no_barrier_and_no_lds():
    """The same words absent as in hamk_exit.hpp: a block-wide barrier inside the exit kernel's step loop would hang the block."""
    text = code(SHARED)
    assert "__syncthreads" not in text and "__shared__" not in text and "s_barrier" not in text and "TRIG_TABLE" not in text
    assert "__ballot(alive) == 0" in code("hamk_exit.hpp")


def test_the_step_and_the_dense_output_are_written_once():
    """The right-hand side is called in the shared header and nowhere in the three headers, comments included, and there is one
    Newton constant."""
    assert "ham_eqs<" in code(SHARED)
    for h in COMPANIONS:
        assert "ham_eqs<" not in KS._text(h) and '#include "hamk_fused_rk4.hpp"' in KS._text(h), h
    everything = "".join(KS._text(h) for h in COMPANIONS + (SHARED,))
    assert re.findall(r"constexpr int (k\w*Newton\w*) = (\d+);", everything) == [("kDenseNewton", str(NEWTON))]
    assert len(re.findall(r"\bk\w*Newton\w*\b", "".join(code(h) for h in COMPANIONS + (SHARED,)))) == 2      # the definition and dense_root's loop
