"""A family of systems that reaches every branch of the generator's symbolic right-hand side (hamk_codegen.cpp symbolic_mass_matrix,
poly_sweep, poly_reduce, poly_prune): plain Python, imported by tests/test_symbolic_rhs.py, tests/test_gpu_symbolic_rhs.py,
scripts/warm_cache.py and oracle/gen_golden_symbolic.py (which writes tests/golden/symbolic_family.json from it).

`spec(seed)`: seeds below 100 are RANDOM members (planar bodies at (rho sin q_i, -rho cos q_i) hanging from the origin or from the
previous body, U a random sum of linear, square, cross-product and cubic terms of its inputs; for a generalized U also
0.7 cos q_0 - 0.3 sin q_0 cos q_0, whose sincos sites must find the slot of f with the same operand).  Seeds from 100 are DIRECTED
members, one per branch the random ones do not reach -- see DIRECTED below; each carries what it promises (`PROMISE[seed]`: the
HAS_SYM_K / DT / GU flags of its generated source) and the tests assert it.

SEEDS was chosen on the CPU by the 50-digit reference alone (oracle/gen_golden.py evaluate_point): every member has
cond K < 1e4 at every fixture point, so the tests built on it leave out no trajectory and no point."""
import numpy as np

from hamilton_amd import examples as E
from hamilton_amd import tracer as T


def _box(n, lo=-1.0, hi=1.0):
    return tuple((lo, hi) for _ in range(n))


def _spec(name, n, inertia, f, u, cart, q_box=None, qd_box=None, dt=0.005):
    q_box = q_box or _box(n)
    return E.SystemSpec(name=name, m=len(inertia), n=n, inertia=tuple(float(w) for w in inertia), f=f, u=u,
                        u_space=E.U_CARTESIAN if cart else E.U_GENERALIZED,
                        q0=tuple(0.5 * (lo + hi) + 0.1 * (hi - lo) for lo, hi in q_box), qd0=(0.2,) * n,
                        q_box=q_box, qd_box=qd_box or _box(n), dt=dt, cite="tests/symbolic_family.py")


def powi_raw(x, k):
    """x ^ k with the POWI opcode ON THE TAPE for every k: the recorder folds x ^ 0 and x ^ 1 away (tracer.powi), a host shim in
    another language need not -- and the generator has a rule for them."""
    if isinstance(x, T.Var):
        return T.Var(x.tape, x.tape.emit(T.OP_POWI, x.idx, int(k)))
    return x ** int(k)


# ---------------------------------------------------------------------------------------------------------------------------------
# random members
# ---------------------------------------------------------------------------------------------------------------------------------
def random_member(seed):
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(1, 4))
    bodies = int(rng.integers(1, 3))
    m = 2 * bodies
    ps = int(rng.integers(1 << 30))
    cart = bool(rng.integers(2))
    inertia = tuple(float(np.round(rng.uniform(0.5, 2.0), 2)) for _ in range(m))

    def f(q, o):
        r = np.random.default_rng(ps)
        out, bx, by = [], 0.0, 0.0
        for b in range(bodies):
            i = b % n
            rho = float(np.round(r.uniform(0.5, 1.5), 2))
            x, y = bx + rho * o.sin(q[i]), by - rho * o.cos(q[i])
            out += [x, y]
            if r.random() < 0.6:
                bx, by = x, y                                      # the next body hangs from this one
        for k in range(bodies, n):                                 # coordinates no body drives: a direct cartesian component
            out[-1] = out[-1] + 1.3 * q[k]
        return out

    def u(z, o):
        r = np.random.default_rng(ps + 1)
        acc = 0.0
        for k, zk in enumerate(z):
            c = float(np.round(r.uniform(0.2, 2.0), 2))
            kind = int(r.integers(4))
            if kind == 0:
                acc = acc + c * zk
            elif kind == 1:
                acc = acc + c * zk * zk
            elif kind == 2:
                acc = acc + c * zk * z[(k + 1) % len(z)]
            else:
                acc = acc + c * zk ** 3 / 3.0
        if not cart:
            acc = acc + 0.7 * o.cos(z[0]) - 0.3 * o.sin(z[0]) * o.cos(z[0])
        return acc

    return _spec(f"symfam{seed}", n, inertia, f, u, cart)


# ---------------------------------------------------------------------------------------------------------------------------------
# directed members
# ---------------------------------------------------------------------------------------------------------------------------------
def _polar(npart, free=0, cubic=True):
    """`npart` particles in polar coordinates (r cos phi, r sin phi) and `free` plain cartesian coordinates: K = diag(m, m r^2, ...),
    every r-phi entry cancels analytically (poly_prune); a CARTESIAN U of degree three in f's outputs, so U . f carries
    sin^2 phi and poly_reduce runs on it."""
    n = 2 * npart + free
    inertia = []
    for i in range(npart):
        inertia += [1.0 + 0.5 * i] * 2
    inertia += [0.8 + 0.3 * k for k in range(free)]
    box = tuple(b for i in range(npart) for b in ((1.0, 2.0), (-1.0 + 0.7 * i, 1.0 + 0.7 * i))) + _box(free)

    def f(q, o):
        out = []
        for i in range(npart):
            r, ph = q[2 * i], q[2 * i + 1]
            out += [r * o.cos(ph), r * o.sin(ph)]
        for k in range(free):
            out.append(1.25 * q[2 * npart + k])
        return out

    def u(x, o):
        acc = 0.0
        for k in range(len(x)):
            acc = acc + (0.4 + 0.1 * k) * x[k] * x[k]
        if cubic:
            acc = acc + 0.3 * x[0] * x[0] * x[1] + x[1] ** 3 / 3.0 - 0.2 * x[0] * x[len(x) - 1]
        return acc

    return n, inertia, f, u, box


def polar(seed, npart, free=0):
    n, inertia, f, u, box = _polar(npart, free)
    return _spec(f"symfam{seed}", n, inertia, f, u, True, q_box=box)


def hanging(seed):
    """A body hanging from a body (the double pendulum with unequal arms and masses): K01 = m2 l1 l2 cos(q0 - q1) after sin^2 + cos^2 = 1,
    K00 and K11 constants.  GENERALIZED U with sincos sites of q0 and q1: each must read the slot of f with the same operand."""
    def f(q, o):
        x1, y1 = 0.8 * o.sin(q[0]), -(0.8 * o.cos(q[0]))
        return [x1, y1, x1 + 1.1 * o.sin(q[1]), y1 - 1.1 * o.cos(q[1])]

    def u(q, o):
        return -(3.0 * o.cos(q[0])) - 1.7 * o.cos(q[1]) + 0.4 * o.sin(q[0]) * o.cos(q[1]) + 0.25 * q[0] * q[1]

    return _spec(f"symfam{seed}", 2, (1.0, 1.0, 1.5, 1.5), f, u, False)


def small_term(seed):
    """An inertia of 1e-9 next to inertias of order one.  K01 = 1e-9 rho^2 is driven by the small body alone; K00 carries the
    small body's own monomial 1e-9 q0^2 next to terms of order one: a TRUE term eight orders above the rounding of what it sits next
    to -- it must survive poly_prune."""
    def f(q, o):
        return [1.5 * q[0], 0.9 * q[1], 0.7 * o.sin(q[0] + q[1]), -(0.7 * o.cos(q[0] + q[1])), 0.5 * q[0] * q[0]]

    def u(q, o):
        return 0.6 * q[0] * q[0] + 0.4 * q[1] * q[1] + 0.3 * q[0] * q[1]

    return _spec(f"symfam{seed}", 2, (1.0, 1.3, 1e-9, 1e-9, 1e-9), f, u, False)


def u_fails(seed, how):
    """f of `hanging`; a generalized U the symbolic gradient must REFUSE: a sincos site whose operand (2 q1) is no slot of f
    ("slot"), an exponential ("exp").  K and dT/dq stay symbolic, grad U keeps the Jet1 sweep."""
    def f(q, o):
        x1, y1 = 0.8 * o.sin(q[0]), -(0.8 * o.cos(q[0]))
        return [x1, y1, x1 + 1.1 * o.sin(q[1]), y1 - 1.1 * o.cos(q[1])]

    def u(q, o):
        base = -(3.0 * o.cos(q[0])) + 0.25 * q[0] * q[1]
        if how == "slot":
            return base + 0.6 * o.cos(2.0 * q[1])
        return base + 0.5 * o.exp(-(q[1] * q[1]))

    return _spec(f"symfam{seed}", 2, (1.0, 1.0, 1.5, 1.5), f, u, False)


def opcodes(seed):
    """Every polynomial opcode of the generator in one map (n = 3), arranged as bodies on circles so that K stays short: ADD, SUB, MUL,
    NEG, POWI with exponents 0 and 1 (kept on the tape: powi_raw), 2 and 3, division by a constant, SIN / COS of an input, of 2 q_i, of
    q_i - q_j and of q_i + q_j, one operand (q0) shared by a SIN site, a COS site and three outputs."""
    def f(q, o):
        a, b, c = q
        s0 = o.sin(a)
        return [0.8 * o.sin(2.0 * a) / 2.0 * powi_raw(b, 0), -(0.8 * o.cos(2.0 * a)) / 2.0,
                0.7 * o.sin(a - b), 0.7 * o.cos(a - b),
                0.9 * o.sin(b + c), -(0.9 * o.cos(b + c)),
                1.2 * c + 0.1 * c ** 3,
                powi_raw(b, 1) + 0.15 * a ** 2,
                0.5 * s0, -(0.5 * o.cos(a)),
                0.3 * s0 + 0.8 * c]

    def u(x, o):
        return 0.5 * x[0] * x[0] + 0.7 * x[1] + 0.3 * x[2] * x[3] - 0.2 * x[5] + 0.1 * x[6] * x[6] + 0.4 * x[7] + 0.6 * x[9]

    return _spec(f"symfam{seed}", 3, (1.0, 1.0, 1.2, 1.2, 0.8, 0.8, 1.5, 0.6, 0.9, 0.9, 1.1), f, u, True)


def pendulum_chain(seed, n, arms=None):
    """n bodies, each hanging from the previous one (the N-link chain with unequal arms): K[a][b] = c_ab cos(q_a - q_b); dT/dq has
    n (n - 1) quartic terms.  The generator's size rule for dT/dq (dt_ops <= 12 n) decides between 111 and 100."""
    arms = arms or [0.6 + 0.1 * k for k in range(n)]

    def f(q, o):
        out, ax, ay = [], 0.0, 0.0
        for k in range(n):
            ax = ax + arms[k] * o.sin(q[k])
            ay = ay - arms[k] * o.cos(q[k])
            out += [ax, ay]
        return out

    def u_cart(x, o):
        acc = 0.0
        for k in range(n):
            acc = acc + (2.0 + 0.5 * k) * x[2 * k + 1]
        return acc

    inertia = []
    for k in range(n):
        inertia += [1.0 + 0.25 * k] * 2
    return _spec(f"symfam{seed}", n, inertia, f, u_cart, True)


def dt_threshold(seed, last_power):
    """The rule dt_ops <= 12 n, steered to the operation (n = 2: 24).  A polar particle (r = q0, phi = q1: dT/dr = -m r v_phi^2, 4
    operations) and cartesian components that are pure powers q^(k+1) / (k+1) of one coordinate: each adds q^(2k) to one diagonal
    entry of K and one monomial of 2k + 2 operations to dT/dq.  q0^2/2, q0^3/3, q1^2/2 and q1^(k+1)/(k+1): k = 2 gives 4 + 4 + 6 + 4 + 6 =
    24 (inside), k = 3 gives 26 (outside).  Plain scalings of q0 and q1 pad the numerical sum so that K itself stays symbolic."""
    k = last_power

    def f(q, o):
        r, ph = q
        return [r * o.cos(ph), r * o.sin(ph), r ** 2 / 2.0, r ** 3 / 3.0, ph ** 2 / 2.0, ph ** (k + 1) / float(k + 1),
                0.5 * r, 0.5 * ph, 0.4 * r, 0.4 * ph]

    def u(x, o):
        return 0.5 * (x[0] * x[0] + x[1] * x[1]) + 0.3 * x[0] + 0.2 * x[4]

    return _spec(f"symfam{seed}", 2, (1.0, 1.0, 0.9, 0.8, 0.7, 0.6, 1.0, 1.0, 1.0, 1.0), f, u, True, q_box=((1.0, 2.0), (-1.0, 1.0)))


def _monomials(nvar, maxdeg):
    """Exponent tuples of every monomial of degree <= maxdeg in nvar variables, in a fixed order (degree, then lexicographic)."""
    out = []

    def rec(prefix, left, k):
        if k == nvar:
            out.append(tuple(prefix))
            return
        for e in range(left + 1):
            rec(prefix + [e], left - e, k + 1)
    rec([], maxdeg, 0)
    return sorted(out, key=lambda t: (sum(t), t))


def gu_threshold(seed, terms):
    """The rule |gU_i| <= 64 monomials.  f is a scaling (K constant, dT/dq = 0: both symbolic at no cost); U = q0 * (sum of `terms`
    distinct monomials of q1 .. q4), so dU/dq0 has exactly `terms` monomials: 64 inside, 65 outside."""
    monos = _monomials(4, 4)[:terms]
    assert len(monos) == terms

    def f(q, o):
        return [(1.0 + 0.1 * k) * q[k] for k in range(5)]

    def u(q, o):
        acc = 0.0
        for j, e in enumerate(monos):
            t = (0.05 + 0.01 * (j % 17)) * q[0]
            for k in range(4):
                for _ in range(e[k]):
                    t = t * q[1 + k]
            acc = acc + t
        return acc + 0.5 * sum(q[k] * q[k] for k in range(1, 5))

    return _spec(f"symfam{seed}", 5, (1.0, 1.2, 0.9, 1.4, 0.7), f, u, False)


def not_polynomial(seed, n):
    """A map the generator must leave alone altogether (000): a square root in f."""
    def f(q, o):
        return [(1.0 + 0.2 * k) * q[k] + 0.3 * o.sqrt(2.0 + q[(k + 1) % n] * q[(k + 1) % n]) for k in range(n)] + [0.5 * o.sin(q[0])]

    def u(x, o):
        acc = 0.0
        for k in range(len(x)):
            acc = acc + 0.5 * x[k] * x[k]
        return acc

    return _spec(f"symfam{seed}", n, tuple(1.0 + 0.1 * k for k in range(n + 1)), f, u, True)


DIRECTED = {
    100: lambda: polar(100, 2),                       # n = 4, cancellation, cartesian U of degree 3
    101: lambda: polar(101, 3),                       # n = 6
    102: lambda: polar(102, 3, free=1),               # n = 7: the largest n the generator takes
    103: lambda: hanging(103),                        # generalized U, sincos sites matching slots of f
    104: lambda: small_term(104),
    105: lambda: u_fails(105, "slot"),
    106: lambda: u_fails(106, "exp"),
    108: lambda: opcodes(108),
    109: lambda: pendulum_chain(109, 4),              # K only (100), as the product's chain4
    111: lambda: dt_threshold(111, 2),                # dt_ops = 24 = 12 n: inside
    112: lambda: dt_threshold(112, 3),                # dt_ops = 26: outside
    113: lambda: gu_threshold(113, 64),               # gU: 64 monomials, inside
    114: lambda: gu_threshold(114, 65),               # ... 65, outside
    115: lambda: not_polynomial(115, 3),
}

REFUSED_N = 8                                         # n > 7: refused by design (symbolic_mass_matrix)


def refused_spec():
    return pendulum_chain(199, REFUSED_N)


def spec(seed):
    if seed in DIRECTED:
        return DIRECTED[seed]()
    if seed == 199:
        return refused_spec()
    if 0 <= seed < 100:
        return random_member(seed)
    raise KeyError(seed)


# The members the tests run: chosen on the CPU by the 50-digit reference alone (cond K < 1e4 at every fixture point;
# oracle/gen_golden_symbolic.py refuses a member that is not).  Random seeds 2, 5, 15 (m < n: K singular) are not usable; the other
# random seeds left out repeat the structure of the ones kept.
SEEDS = [0, 6, 9, 21, 7, 16, 14, 20] + [100, 101, 102, 103, 104, 105, 106, 108, 109, 111, 112, 113, 114, 115]

# what each member promises: HAS_SYM_K / DT / GU of its generated source (tests/test_symbolic_rhs.py asserts them, and that SEEDS
# keeps covering every combination, both U spaces under 111 and the U-side fallbacks)
PROMISE = {0: "111", 6: "111", 9: "111", 21: "111", 7: "100", 16: "100", 14: "000", 20: "000",
           100: "111", 101: "111", 102: "111", 103: "111", 104: "111", 105: "110", 106: "110", 108: "111", 109: "100",
           111: "111", 112: "100", 113: "111", 114: "110", 115: "000"}
U_FALLBACK = {"no matching slot": 105, "non-polynomial opcode": 106}       # 110 by a failure on U's side
CUBIC_CARTESIAN_U = 100                                                      # cartesian U of degree 3 in f's outputs
SLOT_MATCHING_U = 103                                                        # generalized U whose sincos sites match slots of f
