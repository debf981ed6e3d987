"""A family of small systems that reaches every branch of the three rewrites the tape -> C++ generator applies to a tape node by node
(hamk_codegen.cpp emit_body): SHARED EXPONENTIALS (the affine analysis of an exponential's argument: ADD and SUB with the constant on
either side, MUL and DIV by a constant, NEG; the choice of the member that is evaluated), the FUSED 1 / sqrt (hamk::rsqrt_of and the three
conditions under which it must not be used) and the SINCOS slots (pairing, reuse of f's pair by a generalized potential).  Plain Python,
imported by tests/test_codegen_rewrites.py, tests/test_gpu_codegen_rewrites.py, scripts/warm_cache.py and oracle/gen_golden_rewrites.py
(which writes tests/golden/rewrite_family.json from it).

Every member has n <= 3 and m <= 4 -- the rewrites are per tape node, nothing larger can fail differently -- and cond K < 1e3 at every
fixture point (the generator script refuses a member otherwise), so no comparison leaves out a point or a trajectory.  `PROMISE[key]`
states what the generated source must contain; the tests assert it:
    exp    (hamk::exp( calls in `coords`, in `potential`)
    rsqrt  (hamk::rsqrt_of( calls in `coords`, in `potential`)
    trig   (NTRIG_F, NTRIG_U, the slots of f that `potential_after_f` reads with TRIG_REUSE)
|argument| of every exponential stays below 40 on the sampling box except in the RANGE members, whose point is the range."""
import math

from hamilton_amd import examples as E


def _box(n, lo=-1.0, hi=1.0):
    return tuple((lo, hi) for _ in range(n))


def _spec(key, n, inertia, f, u, cart, q_box=None, dt=0.005):
    q_box = q_box or _box(n)
    return E.SystemSpec(name=f"rewrite_{key}", m=len(inertia), n=n, inertia=tuple(float(w) for w in inertia), f=f, u=u,
                        u_space=E.U_CARTESIAN if cart else E.U_GENERALIZED,
                        q0=tuple(0.5 * (lo + hi) + 0.1 * (hi - lo) for lo, hi in q_box), qd0=(0.2,) * n,
                        q_box=q_box, qd_box=_box(n), dt=dt, cite="tests/rewrite_family.py")


def _scaling(n):
    return lambda q, o: [(1.0 + 0.25 * k) * q[k] for k in range(n)]


def _well(q):
    acc = 0.0
    for k, x in enumerate(q):
        acc = acc + (0.5 + 0.1 * k) * x * x
    return acc


def _exp_u(key, terms, n=2):
    """f a scaling of n = 2 coordinates, U (generalized) = a quadratic well + sum of weight * exp(argument(q)) over `terms`."""
    def u(q, o):
        acc = _well(q)
        for w, arg in terms:
            acc = acc + w * o.exp(arg(q))
        return acc
    return _spec(key, n, (1.0, 1.3, 0.8)[:n], _scaling(n), u, False)


# ---------------------------------------------------------------------------------------------------------------------------------
# shared exponentials: one member per branch of the affine analysis
# ---------------------------------------------------------------------------------------------------------------------------------
K_ASSOC, A_ASSOC = 1.7, 0.3

EXP_MEMBERS = {
    # ADD: constant on the right, constant on the left
    "exp_add": lambda: _exp_u("exp_add", [(0.05, lambda q: q[0] + 1.5), (0.2, lambda q: 0.5 + q[0])]),
    # SUB, constant on the right
    "exp_sub_right": lambda: _exp_u("exp_sub_right", [(0.3, lambda q: q[0] - 1.5), (0.2, lambda q: q[0] - 0.25)]),
    # SUB, constant on the left: slope -1 -- paired with -q0 + 0.5, which reaches slope -1 through NEG and ADD
    "exp_sub_left": lambda: _exp_u("exp_sub_left", [(0.1, lambda q: 1.5 - q[0]), (0.2, lambda q: -q[0] + 0.5)]),
    # MUL: k * x and x * k (two different tape nodes: the recorder does not reorder operands)
    "exp_mul": lambda: _exp_u("exp_mul", [(0.3, lambda q: 0.7 * q[0]), (0.1, lambda q: q[0] * 0.7 + 1.0)]),
    # DIV by a constant: (x - 1) / 4 has slope 1/4 and offset -1/4 -- paired with 0.25 x + 0.5, which gets there through MUL
    "exp_div": lambda: _exp_u("exp_div", [(0.3, lambda q: (q[0] - 1.0) / 4.0), (0.2, lambda q: 0.25 * q[0] + 0.5)]),
    # NEG of a sum and NEG of an input
    "exp_neg": lambda: _exp_u("exp_neg", [(0.3, lambda q: -(q[0] + 0.5)), (0.2, lambda q: -q[0])]),
    # the nested chain of a logistic wall, -(beta (x - pos)), at two positions (NEG of MUL of SUB)
    "exp_logistic": lambda: _spec("exp_logistic", 2, (1.0, 1.3), _scaling(2),
                                  lambda q, o: _well(q) + (1 - E.logistic(-1.5, 2.0, 0.5, q[0], o)) + E.logistic(1.5, 2.0, 0.5, q[0], o), False),
    # one function written in two associations: k (x - a) and k x - k a.  Shared if and only if the two fp64 offsets are equal
    "exp_assoc": lambda: _exp_u("exp_assoc", [(0.2, lambda q: K_ASSOC * (q[0] - A_ASSOC)), (0.1, lambda q: K_ASSOC * q[0] - K_ASSOC * A_ASSOC)]),
    # three and four exponentials of one line: ONE evaluation (a derived member is never the one another is derived from)
    "exp_three": lambda: _exp_u("exp_three", [(0.2, lambda q: q[0] - 1.0), (0.1, lambda q: q[0] + 2.0), (0.15, lambda q: 0.25 + q[0])]),
    "exp_four": lambda: _exp_u("exp_four", [(0.2, lambda q: 2.0 * q[0] - 1.0), (0.02, lambda q: 2.0 * q[0] + 2.0), (0.1, lambda q: 2.0 * q[0] + 0.5),
                                            (0.1, lambda q: (q[0] - 0.125) * 2.0)]),
    # must NOT share: one value under two slopes; one slope and offset over two values; slopes +1 and -1 over one value
    "exp_no_share": lambda: _exp_u("exp_no_share", [(0.2, lambda q: 0.5 * q[0] + 1.0), (0.2, lambda q: 0.25 * q[0] + 1.0), (0.1, lambda q: q[0] + 0.5),
                                                    (0.1, lambda q: q[1] + 0.5), (0.1, lambda q: 1.5 - q[1])]),
}


def exp_f_output():
    """An exponential that is an OUTPUT of f and is the derived member of its pair (the smaller offset); generalized polynomial U."""
    def f(q, o):
        return [q[0] + 0.2 * o.exp(0.5 * q[0] + 0.5), o.exp(0.5 * q[0] - 0.5), 1.1 * q[1]]
    return _spec("exp_f_output", 2, (1.0, 0.7, 1.3), f, lambda q, o: _well(q) + 0.3 * q[0] * q[1], False)


def exp_in_f_cart_u():
    """The pair inside f, the later member carrying the larger offset (it is hoisted); cartesian polynomial U."""
    def f(q, o):
        return [q[0] + 0.2 * o.exp(q[0] - 0.5), 1.2 * q[1] + 0.1 * o.exp(q[0] + 0.5)]
    return _spec("exp_in_f_cart_u", 2, (1.0, 1.3), f, lambda x, o: 0.5 * x[0] * x[0] + 0.4 * x[1] * x[1] + 0.2 * x[0] * x[1], True)


def exp_in_cart_u():
    """The pair inside a cartesian U: coords_sink_u emits it with f's outputs composed in for U's inputs."""
    def f(q, o):
        return [1.2 * q[0], 0.9 * q[1] + 0.2 * q[0]]
    return _spec("exp_in_cart_u", 2, (1.0, 1.3), f, lambda x, o: 0.3 * o.exp(x[0] - 0.5) + 0.05 * o.exp(x[0] + 1.0) + 0.5 * x[1] * x[1], True)


# ---------------------------------------------------------------------------------------------------------------------------------
# range members: one coordinate, f = [q0], q0 in [-1, 1]; U = A exp(q0 + a) + C exp(q0 + c) + q0^2 / 2
# ---------------------------------------------------------------------------------------------------------------------------------
def _range(key, first, second):
    """`first`, `second`: (weight, offset) in the order U writes them."""
    def u(q, o):
        return first[0] * o.exp(q[0] + first[1]) + second[0] * o.exp(q[0] + second[1]) + q[0] * q[0] / 2.0
    return _spec(key, 1, (1.0,), lambda q, o: [q[0]], u, False)


C135 = math.exp(135.0)             # C exp(q0 - 135) = exp(q0): of order one.  A = 1: exp(q0 - 735) <= 2e-319 is negligible (and subnormal in fp64)
A705, C105 = math.exp(-705.0), math.exp(-105.0)      # both terms exp(q0); exp(q0 + 705) <= 4e306 is finite in fp64 with all its derivatives
RANGE_MEMBERS = {
    "range_low_small_first": lambda: _range("range_low_small_first", (1.0, -735.0), (C135, -135.0)),
    "range_low_small_second": lambda: _range("range_low_small_second", (C135, -135.0), (1.0, -735.0)),
    "range_high_large_first": lambda: _range("range_high_large_first", (A705, 705.0), (C105, 105.0)),
    "range_high_large_second": lambda: _range("range_high_large_second", (C105, 105.0), (A705, 705.0)),
    # offsets 601 apart: beyond the sharing limit of 600
    "range_beyond_limit": lambda: _range("range_beyond_limit", (0.5 * math.exp(650.0), -650.0), (0.5 * math.exp(49.0), -49.0)),
    # three members written in the order -700, -350, 0: the one with offset 0 (the last on the tape) is evaluated, the one at -350 is
    # derived from it, and the one at -700 -- 700 below -- is evaluated itself: it must not be derived from the derived one
    "range_chain": lambda: _exp_u("range_chain", [(1.0, lambda q: q[0] - 700.0), (math.exp(350.0), lambda q: q[0] - 350.0), (0.3, lambda q: q[0] + 0.0)], n=1),
    # ONE exponential, nothing to share, whose value is subnormal in fp64 (exp(-729) ... exp(-731) = 2e-317 ... 3e-318): finite as the
    # tape writes it, so no status bit may be set
    "range_lone_subnormal": lambda: _exp_u("range_lone_subnormal", [(1.0, lambda q: q[0] - 730.0)], n=1),
}
# which offset the ONE evaluated exponential of a shared range member carries (asserted from the emitted text)
RANGE_EVALUATED_OFFSET = {"range_low_small_first": -135.0, "range_low_small_second": -135.0,
                          "range_high_large_first": 705.0, "range_high_large_second": 705.0}


# ---------------------------------------------------------------------------------------------------------------------------------
# fused 1 / sqrt
# ---------------------------------------------------------------------------------------------------------------------------------
L12 = 12.0 * math.log(10.0)        # d = exp(L12 q0) (1.5 + q1^2): 1e-12 ... 1e12 over q0 in [-1, 1]


def _d_wide(q, o):
    return o.exp(L12 * q[0]) * (1.5 + q[1] * q[1])


def _w_wide(q, o):
    return o.exp((L12 / 2.0) * q[0]) * (1.0 + 0.5 * q[1])       # ~ sqrt(d): w / sqrt(d) is of order one


def rsqrt_u():
    """1 / sqrt(d) in U, d from 1e-12 to 1e12 over the box, scaled to order one.  Fused."""
    return _spec("rsqrt_u", 2, (1.0, 1.3), _scaling(2), lambda q, o: _well(q) + 0.8 * (_w_wide(q, o) * (1.0 / o.sqrt(_d_wide(q, o)))), False)


def rsqrt_f():
    """The same in f.  Fused (the reciprocal feeds an output; the square root has one reader and is no output)."""
    def f(q, o):
        return [q[0] + 0.3 * (_w_wide(q, o) * (1.0 / o.sqrt(_d_wide(q, o)))), 1.1 * q[1], 1.0 / o.sqrt(2.0 + q[0] * q[0] + q[1] * q[1])]
    return _spec("rsqrt_f", 2, (1.0, 1.3, 0.9), f, lambda x, o: 0.5 * x[0] * x[0] + 0.4 * x[1] * x[1] + 0.3 * x[2], True)


def rsqrt_twice():
    """The square root read twice: -1 / sqrt(d) + 0.1 sqrt(d).  Not fused."""
    def u(q, o):
        s = o.sqrt(1.5 + q[0] * q[0] + q[1] * q[1])
        return _well(q) - 1.0 / s + 0.1 * s
    return _spec("rsqrt_twice", 2, (1.0, 1.3), _scaling(2), u, False)


def rsqrt_sqrt_output():
    """The square root an output of f next to 1 / sqrt of the same node: one reader, but an output.  Not fused -- fused, the module would
    not compile (the square root is never emitted)."""
    def f(q, o):
        s = o.sqrt(2.0 + q[0] * q[0] + q[1] * q[1])
        return [q[0] + 0.3 * (1.0 / s), s, 1.1 * q[1]]
    return _spec("rsqrt_sqrt_output", 2, (1.0, 0.7, 1.3), f, lambda q, o: _well(q) + 0.3 * q[0] * q[1], False)


def rsqrt_div():
    """c / sqrt(d) with c != 1 is a DIV on the tape, not a RECIP.  Not fused."""
    return _spec("rsqrt_div", 2, (1.0, 1.3), _scaling(2), lambda q, o: _well(q) - 2.5 / o.sqrt(1.5 + q[0] * q[0] + q[1] * q[1]), False)


# ---------------------------------------------------------------------------------------------------------------------------------
# sincos slots
# ---------------------------------------------------------------------------------------------------------------------------------
def _bob(q, o):
    return [0.9 * o.sin(q[0]), -(0.9 * o.cos(q[0]))]


def trig_pair():
    """sin and cos of one operand: one slot."""
    return _spec("trig_pair", 2, (1.0, 1.0, 1.3), lambda q, o: _bob(q, o) + [1.1 * q[1]], lambda q, o: _well(q) + 0.3 * q[0] * q[1], False)


def trig_sin_only():
    """Only sin of an operand: one slot, no pair."""
    return _spec("trig_sin_only", 2, (1.0, 1.3), lambda q, o: [q[0] + 0.4 * o.sin(q[1]), 1.2 * q[1]], lambda q, o: _well(q) + 0.3 * q[0] * q[1], False)


def trig_reuse():
    """q0 and q1 are sincos operands of f AND of a generalized U: U reads f's slots 0 and 1.  (The exponential keeps grad U on the jets.)"""
    def f(q, o):
        return _bob(q, o) + [q[1] + 0.3 * o.sin(q[1])]

    def u(q, o):
        return -(2.0 * o.cos(q[0])) + 0.4 * o.sin(q[1]) * o.cos(q[0]) + 0.3 * o.exp(-(q[1] * q[1])) + 0.5 * q[1] * q[1]
    return _spec("trig_reuse", 2, (1.0, 1.0, 1.3), f, u, False)


def trig_u_only():
    """U has f's operand q0 (reused) and two that f does not have: q1 and 2 q0 (slots of its own)."""
    def u(q, o):
        return -(2.0 * o.cos(q[0])) + 0.5 * o.cos(q[1]) + 0.2 * o.sin(2.0 * q[0]) + 0.3 * o.exp(-(q[1] * q[1])) + 0.5 * q[1] * q[1]
    return _spec("trig_u_only", 2, (1.0, 1.0, 1.3), lambda q, o: _bob(q, o) + [1.1 * q[1]], u, False)


def trig_cart_u():
    """The operand under a CARTESIAN U: its inputs are f's outputs, nothing is reused."""
    def u(x, o):
        return 2.0 * x[1] + 0.3 * o.sin(x[2]) + 0.2 * o.cos(x[2]) + 0.3 * o.exp(-(x[2] * x[2])) + 0.5 * x[2] * x[2]
    return _spec("trig_cart_u", 2, (1.0, 1.0, 1.3), lambda q, o: _bob(q, o) + [1.1 * q[1]], u, True)


MEMBERS = dict(EXP_MEMBERS)
MEMBERS.update({"exp_f_output": exp_f_output, "exp_in_f_cart_u": exp_in_f_cart_u, "exp_in_cart_u": exp_in_cart_u})
MEMBERS.update(RANGE_MEMBERS)
MEMBERS.update({"rsqrt_u": rsqrt_u, "rsqrt_f": rsqrt_f, "rsqrt_twice": rsqrt_twice, "rsqrt_sqrt_output": rsqrt_sqrt_output, "rsqrt_div": rsqrt_div,
                "trig_pair": trig_pair, "trig_sin_only": trig_sin_only, "trig_reuse": trig_reuse, "trig_u_only": trig_u_only, "trig_cart_u": trig_cart_u})
KEYS = list(MEMBERS)
RANGE_KEYS = list(RANGE_MEMBERS)
FUSED_KEYS = ["rsqrt_u", "rsqrt_f"]                      # the members that run the fused node under every AD mode


GPU_VARIANTS = ["default", "R", "quad", "wave"]           # the builds tests/test_gpu_codegen_rewrites.py runs every member on


def gpu_options(variant):
    """hamk_options fields (hamilton_amd.api.system_from_spec) of one of GPU_VARIANTS."""
    from hamilton_amd import _abi
    return {"default": None, "R": {"ad_mode": _abi.AD_R}, "quad": {"mapping": _abi.MAP_QUAD}, "wave": {"mapping": _abi.MAP_WAVE}}[variant]


def spec(key):
    return MEMBERS[key]()


def _p(exp=(0, 0), rsqrt=(0, 0), trig=(0, 0, ())):
    return dict(exp=tuple(exp), rsqrt=tuple(rsqrt), trig=(trig[0], trig[1], tuple(trig[2])))


PROMISE = {
    "exp_add": _p(exp=(0, 1)), "exp_sub_right": _p(exp=(0, 1)), "exp_sub_left": _p(exp=(0, 1)), "exp_mul": _p(exp=(0, 1)),
    "exp_div": _p(exp=(0, 1)), "exp_neg": _p(exp=(0, 1)), "exp_logistic": _p(exp=(0, 1)),
    "exp_assoc": _p(exp=(0, 1)),                          # fl(-0.3 * 1.7) == -fl(1.7 * 0.3): the offsets are equal, the pair shares
    "exp_three": _p(exp=(0, 1)), "exp_four": _p(exp=(0, 1)), "exp_no_share": _p(exp=(0, 5)),
    "exp_f_output": _p(exp=(1, 0)), "exp_in_f_cart_u": _p(exp=(1, 0)), "exp_in_cart_u": _p(exp=(0, 1)),
    "range_low_small_first": _p(exp=(0, 1)), "range_low_small_second": _p(exp=(0, 1)),
    "range_high_large_first": _p(exp=(0, 1)), "range_high_large_second": _p(exp=(0, 1)),
    "range_beyond_limit": _p(exp=(0, 2)), "range_chain": _p(exp=(0, 2)), "range_lone_subnormal": _p(exp=(0, 1)),
    "rsqrt_u": _p(exp=(0, 2), rsqrt=(0, 1)), "rsqrt_f": _p(exp=(2, 0), rsqrt=(2, 0)),
    "rsqrt_twice": _p(), "rsqrt_sqrt_output": _p(), "rsqrt_div": _p(),
    "trig_pair": _p(trig=(1, 0, ())), "trig_sin_only": _p(trig=(1, 0, ())),
    "trig_reuse": _p(exp=(0, 1), trig=(2, 2, (0, 1))), "trig_u_only": _p(exp=(0, 1), trig=(1, 3, (0,))),
    "trig_cart_u": _p(exp=(0, 1), trig=(1, 1, ())),
}


# ---------------------------------------------------------------------------------------------------------------------------------
# reading the generated source
# ---------------------------------------------------------------------------------------------------------------------------------
def functions(src):
    """Generated member functions of HamkSys by name -> body text (coords, potential, potential_after_f, coords_sink, coords_sink_u ...)."""
    import re
    out = {}
    for m in re.finditer(r"^  template <[^\n]*\bstatic \w+ (\w+)\([^\n]*\{\n(.*?)^  \}\n", src, re.S | re.M):
        out[m.group(1)] = m.group(2)
    return out


def found(src):
    """What PROMISE states, read from a generated source; plus the counts of the sink and after-f variants of the same tapes."""
    import re
    fn = functions(src)
    n = lambda name, what: fn[name].count(what)
    ntrig = tuple(int(re.search(rf"NTRIG_{w} = (\d+);", src).group(1)) for w in "FU")
    reuse = tuple(sorted({int(k) for k in re.findall(r"hamk::TRIG_REUSE>\([^\n]*?, tcf, (\d+)\)", fn["potential_after_f"])}))
    return dict(exp=(n("coords", "hamk::exp("), n("potential", "hamk::exp(")), rsqrt=(n("coords", "hamk::rsqrt_of("), n("potential", "hamk::rsqrt_of(")),
                trig=(ntrig[0], ntrig[1], reuse),
                exp_sink=(n("coords_sink", "hamk::exp("), n("coords_sink_u", "hamk::exp(")),
                rsqrt_sink=(n("coords_sink", "hamk::rsqrt_of("), n("coords_sink_u", "hamk::rsqrt_of(")),
                exp_after_f=n("potential_after_f", "hamk::exp("), shares_f_trig="U_SHARES_F_TRIG = true" in src)
