"""Shared helpers of the symbolic right-hand-side tests (test_symbolic_k.py, test_symbolic_grad_u.py, test_symbolic_rhs.py,
test_gpu_symbolic_rhs.py): parse the text the generator emits (mass_matrix_sym, dT_sym, gU_sym: one sum of monomials per entry over
q[], v[], tc.s[], tc.c[] with hex-float coefficients), read the HAS_SYM_* flags, and evaluate the sincos pairs of the trig-cache slots
from each slot's OPERAND on the coordinate map's tape."""
import re

import numpy as np

from hamilton_amd import tracer as T

HEX = r"-?0x[0-9a-f.]+p[+-]\d+"


def emitted(src, fn):
    """{target: C++ expression} of one generated function, None where the module has an empty stub."""
    m = re.search(r"static void %s\(const double \(&q\)\[N\].*?\{\n(.*?)\n  \}" % fn, src, re.S)
    if not m:
        return None
    return {t: e for t, e in re.findall(r"^\s*(\w+(?:\[\d+\])+) = ([^;]*);", m.group(1), re.M)}


def as_python(e):
    """A generated expression as Python over q, v, s, c (one parenthesis on either side of a hex literal goes with it)."""
    e = re.sub(r"\(?(" + HEX + r")\)?", lambda m: repr(float.fromhex(m.group(1))), e)
    return e.replace("tc.s[", "s[").replace("tc.c[", "c[")


def sym_functions(src):
    """{"K": {(a, b): python expression}, "dT": {i: expression}, "gU": {i: expression}} parsed from a generated module (None where the
    module has none).  K: the upper triangle (the lower one is copied in the generated code)."""
    out = {"K": None, "dT": None, "gU": None}
    kb, db, gb = emitted(src, "mass_matrix_sym"), emitted(src, "dT_sym"), emitted(src, "gU_sym")
    if kb:
        out["K"] = {}
        for t, e in kb.items():
            a, b = (int(x) for x in re.findall(r"\[(\d+)\]", t))
            if not e.startswith("K["):
                out["K"][(a, b)] = as_python(e)
    if db:
        out["dT"] = {int(re.findall(r"\[(\d+)\]", t)[0]): as_python(e) for t, e in db.items()}
    if gb:
        out["gU"] = {int(re.findall(r"\[(\d+)\]", t)[0]): as_python(e) for t, e in gb.items()}
    return out


def trig_input_table(src):
    """The generated trig_input table: which input (or -1) each sincos slot of f takes as its operand."""
    m = re.search(r"trig_input\(int slot\) \{\n\s*constexpr int w\[\d+\] = \{([^}]*)\}", src)
    return [int(t) for t in m.group(1).split(",")]


def flags(src):
    """HAS_SYM_K / DT / GU of a generated module as a string such as "110"."""
    return "".join("1" if ("HAS_SYM_%s = true" % k) in src else "0" for k in ("K", "DT", "GU"))


def slot_operands(spec):
    """(tape of f, [tape value that is the operand of trig-cache slot k]): slots are numbered by the first SIN / COS of an operand,
    in tape order (hamk_codegen.cpp emit_body)."""
    tf, _ = spec.trace()
    slots = []
    for op, a, _, _ in tf.ops:
        if op in (T.OP_SIN, T.OP_COS) and a not in slots:
            slots.append(a)
    return tf, slots


def slot_sincos(spec, q, src=None):
    """(s, c): the sincos pair of every slot at q, correctly rounded: the slot's operand POLYNOMIAL is evaluated from the tape in
    80-bit arithmetic (an operand such as q0 + q1 rounded to fp64 first would already cost more than the ulp the tolerance grants),
    sin and cos in 80 bits, rounded once.  With `src`: the slots that are inputs must be the ones the generated table names."""
    tf, slots = slot_operands(spec)
    L = np.longdouble
    memo = {}

    def val(i):
        if i in memo:
            return memo[i]
        op, a, b, c = tf.ops[i]
        if op == T.OP_CONST: r = L(c)
        elif op == T.OP_INPUT: r = L(q[a])
        elif op == T.OP_ADD: r = val(a) + val(b)
        elif op == T.OP_SUB: r = val(a) - val(b)
        elif op == T.OP_MUL: r = val(a) * val(b)
        elif op == T.OP_DIV: r = val(a) / val(b)
        elif op == T.OP_NEG: r = -val(a)
        elif op == T.OP_POWI: r = val(a) ** b
        else: raise ValueError("sincos operand is not a polynomial: opcode %d" % op)
        memo[i] = r
        return r

    if src is not None:
        table = trig_input_table(src)
        if slots:
            assert len(table) == len(slots)
            for k, i in enumerate(slots):
                assert table[k] == (tf.ops[i][1] if tf.ops[i][0] == T.OP_INPUT else -1), (k, table)
    s = [float(np.sin(val(i))) for i in slots]
    c = [float(np.cos(val(i))) for i in slots]
    return s, c


def eval_with_bound(expr, env):
    """(value, bound) of one emitted sum of monomials at a point: the value in fp64 as Python evaluates the text, and the running-error
    bound (T + d + 4) 2^-52 sum |coefficient * monomial| for T monomials of degree at most d over sincos values correct to one ulp."""
    terms = expr.split(" + ")
    vals = [eval(t, dict(env)) for t in terms]
    d = max(len(re.findall(r"\b[qvsc]\[\d+\]", t)) for t in terms)
    value = eval(expr, dict(env))
    return value, (len(terms) + d + 4) * 2.0 ** -52 * sum(abs(x) for x in vals)
