"""A family of RECTANGULAR systems (m != n coordinate maps), one member per branch the kernels take on m against a size derived from n.
Every other system the suite steps on the four-lane or the wave-cooperative kernels has m = n, m = n + 1 or m = 2 n.  Plain Python,
imported by tests/test_rect_family.py, tests/test_gpu_rect_family.py, scripts/warm_cache.py and oracle/gen_golden_rect.py (which
writes tests/golden/rect_family.json from it).  The members are NOT examples: nothing here goes into hamilton_amd/examples.py.

Every map is SEPARABLE, x_k = sum_j (c_kj q_j + a_kj sin q_j + b_kj cos q_j), given by three sparse coefficient tables (`coefficients`):
    dense     c_kj = 2 at j = k mod n; a_kj, b_kj the fixed tables of examples.dense(N), scaled by 1 / n            (m n entries of J)
    banded    output k reads q_j, j = k mod n, and one neighbour: c, a at j, b at j + 1 (j - 1 for the last)       (2 m entries)
    single    output k reads q_j alone, j = k mod n                                                                 (m entries)
so the fixture generator has J, dJ/dq and grad U in closed form at 50 digits (it checks that form against the generic symbolic
derivation on the small members).  U is 1/2 |x|^2 over the cartesian coordinates, or sum_j (q_j^2 / 2 + 0.1 cos(q_j - q_(j+1))) over the
generalized ones.  All inertias are positive.  NP4 below is n rounded up to a multiple of four (hamk_quad.hpp Geo).

    key          n    m   map / U               asked         runs on       branch
    qd_eq        17   20  dense, cartesian      auto          quad dense    M = NP4: all of dU/dx in the rows of V; identity padding 17 -> 20
    qd_first_gu  17   21  dense, cartesian      auto          quad dense    the first row of dU/dx that waits in the rows of GU
    qd_last      20   40  dense, cartesian      auto          quad dense    M = 2 NP4, no padding: the last size the dense quad path holds
    qd_over      20   41  dense, cartesian      auto          wave          one past it: created, run, reported as the wave mapping
    qd_gen       18   54  dense, generalized    auto          quad dense    m = 3 n where dU/dx is never stored
    qb_wide      17   51  banded, cartesian     auto          quad banded   quad_eligible (at most 8 n entries of J) with m = 3 n
    qb_max       17  128  single, cartesian     auto, quad    quad banded   m at the ABI's limit
    wv_odd       33   35  banded, cartesian     auto          wave          rows of J no multiple of four, one trajectory per wavefront
    wv_max       17  128  single, cartesian     wave          wave          m = 128, two trajectories per wavefront
    ln_wide_c     3  128  dense, cartesian      lane          lane          the Jet1<128> potential sweep of one lane
    ln_wide_g    16   33  banded, generalized   lane          lane          the top n of the lane mapping with m = 2 n + 1
    ln_thin       4    4  dense, cartesian      lane          lane          control: a square member, inertias 1 ... 1e-3

cond K < 1e4 on the whole sampling box: asserted by the generator at every fixture point and by the tests, with the oracle, on every
trajectory they sample."""
from hamilton_amd import examples as E


def _box(n, lo, hi):
    return tuple((lo, hi) for _ in range(n))


# ---------------------------------------------------------------------------------------------------------------------------------
# coefficient tables: {(k, j): value}, fp64 as written
# ---------------------------------------------------------------------------------------------------------------------------------
def _dense_tables(n, m):
    s = 1.0 / n
    c = {(k, k % n): 2.0 for k in range(m)}
    a = {(k, j): s * (0.2 + 0.1 * ((3 * k + 7 * j) % 11)) for k in range(m) for j in range(n)}
    b = {(k, j): s * (0.15 + 0.1 * ((5 * k + 2 * j) % 7)) for k in range(m) for j in range(n)}
    return c, a, b


def _neighbour(j, n):
    return j + 1 if j + 1 < n else j - 1


def _banded_tables(n, m):
    c = {(k, k % n): 1.5 + 0.1 * (k % 5) for k in range(m)}
    a = {(k, k % n): 0.3 + 0.05 * (k % 7) for k in range(m)}
    b = {(k, _neighbour(k % n, n)): 0.2 + 0.04 * (k % 3) for k in range(m)}
    return c, a, b


def _single_tables(n, m):
    c = {(k, k % n): 1.5 + 0.1 * (k % 5) for k in range(m)}
    a = {(k, k % n): 0.3 + 0.05 * (k % 7) for k in range(m)}
    b = {(k, k % n): 0.2 + 0.04 * (k % 3) for k in range(m)}
    return c, a, b


TABLES = {"dense": _dense_tables, "banded": _banded_tables, "single": _single_tables}


def _map(n, m, tables):
    """x_k = sum_j (c_kj q_j + a_kj sin q_j + b_kj cos q_j), written as examples.dense writes it: the linear terms, then column by column."""
    c, a, b = tables

    def f(q, o):
        used = sorted({j for (_, j) in a} | {j for (_, j) in b})
        sn = {j: o.sin(q[j]) for j in used}
        cs = {j: o.cos(q[j]) for j in used}
        out = []
        for k in range(m):
            acc = None
            for j in range(n):
                if (k, j) in c:
                    t = c[(k, j)] * q[j]
                    acc = t if acc is None else acc + t
            for j in range(n):
                if (k, j) in a:
                    t = a[(k, j)] * sn[j]
                    acc = t if acc is None else acc + t
                if (k, j) in b:
                    t = b[(k, j)] * cs[j]
                    acc = t if acc is None else acc + t
            out.append(acc)
        return out
    return f


def _u_cart(m):
    def u(x, o):
        acc = 0.0
        for k in range(m):
            acc = acc + x[k] * x[k]
        return 0.5 * acc
    return u


def _u_gen(n):
    def u(q, o):
        acc = 0.0
        for j in range(n):
            acc = acc + 0.5 * q[j] * q[j] + 0.1 * o.cos(q[j] - q[(j + 1) % n])
        return acc
    return u


def _inertia(m):
    return tuple(1.0 + 0.25 * (k % 3) for k in range(m))


# key: (n, m, kind of map, cartesian U, mapping asked (None = auto), mapping that runs, QUAD_DENSE in the source, inertia, q box half-width, dt)
TABLE = {
    "qd_eq": (17, 20, "dense", True, None, "quad", True, _inertia, 1.0, 0.01),
    "qd_first_gu": (17, 21, "dense", True, None, "quad", True, _inertia, 1.0, 0.01),
    "qd_last": (20, 40, "dense", True, None, "quad", True, _inertia, 1.0, 0.01),
    "qd_over": (20, 41, "dense", True, None, "wave", False, _inertia, 1.0, 0.01),
    "qd_gen": (18, 54, "dense", False, None, "quad", True, _inertia, 1.0, 0.01),
    "qb_wide": (17, 51, "banded", True, None, "quad", False, _inertia, 1.0, 0.01),
    "qb_max": (17, 128, "single", True, None, "quad", False, _inertia, 1.0, 0.005),
    "wv_odd": (33, 35, "banded", True, None, "wave", False, _inertia, 1.0, 0.01),
    "wv_max": (17, 128, "single", True, "wave", "wave", False, _inertia, 1.0, 0.005),
    "ln_wide_c": (3, 128, "dense", True, "lane", "lane", False, _inertia, 1.0, 0.002),
    "ln_wide_g": (16, 33, "banded", False, "lane", "lane", False, _inertia, 1.0, 0.01),
    "ln_thin": (4, 4, "dense", True, "lane", "lane", False, lambda m: tuple(10.0 ** (-k) for k in range(m)), 1.0, 0.01),
}
KEYS = list(TABLE)
NPOINTS = 4                                            # fixture points per member: examples.sample_config(spec, 0, NPOINTS)
COND_LIMIT = 1e4


def coefficients(key):
    n, m, kind = TABLE[key][:3]
    return TABLES[kind](n, m)


def spec(key):
    n, m, kind, cart, _, _, _, inertia, half, dt = TABLE[key]
    return E.SystemSpec(name=f"rect_{key}", m=m, n=n, inertia=inertia(m), f=_map(n, m, TABLES[kind](n, m)),
                        u=_u_cart(m) if cart else _u_gen(n), u_space=E.U_CARTESIAN if cart else E.U_GENERALIZED,
                        q0=(0.1,) * n, qd0=(0.2,) * n, q_box=_box(n, -half, half), qd_box=_box(n, -0.5, 0.5), dt=dt,
                        cite="tests/rect_family.py")


def asked(key):
    return TABLE[key][4]


def runs_on(key):
    return TABLE[key][5]


def quad_dense(key):
    return TABLE[key][6]


def np4(n):
    return 4 * ((n + 3) // 4)


def options(mapping):
    """hamk_options fields (hamilton_amd.api.system_from_spec) that ask for `mapping`: None (the library's choice), "lane", "quad", "wave"."""
    from hamilton_amd import _abi
    return None if mapping is None else {"mapping": {"lane": _abi.MAP_LANE, "quad": _abi.MAP_QUAD, "wave": _abi.MAP_WAVE}[mapping]}


def mapping_code(name):
    from hamilton_amd import _abi
    return {"lane": _abi.MAP_LANE, "quad": _abi.MAP_QUAD, "wave": _abi.MAP_WAVE}[name]


# what the tests build: every member as the table asks for it; qb_max also with the quad mapping stated; on the GPU the three members
# that sit on the V / GU boundary of the dense quad path also on the wave kernels, for the comparison of the two mappings
RUNS = [(key, asked(key)) for key in KEYS] + [("qb_max", "quad")]
QUAD_AND_WAVE = ["qd_eq", "qd_first_gu", "qd_last"]
GPU_RUNS = RUNS + [(key, "wave") for key in QUAD_AND_WAVE]
