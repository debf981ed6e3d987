#!/usr/bin/env python3
"""Generate tests/golden/rect_family.json: 50-digit fixtures for the rectangular systems of tests/rect_family.py.

TEST INFRASTRUCTURE, derived data like the rest of tests/golden.  The members' maps are separable,
    x_k = sum_j (c_kj q_j + a_kj sin q_j + b_kj cos q_j),
so their mechanics have a CLOSED FORM that needs no tape, no AD and no symbolic second derivatives of an m x n x n array (n = 33, m = 128
are slow there), written out here as oracle/gen_golden.py evaluate_chain_point writes out the chains':
    J_kj       = c_kj + a_kj cos q_j - b_kj sin q_j
    dJ_kj/dq_i = delta_ij D_kj,   D_kj = -a_kj sin q_j - b_kj cos q_j
    K = J^T M J,  p = K qd,  v = K^-1 p  (mpmath LU at 50 digits),  T = v . p / 2
    dT/dq_i    = -(M J v) . ((dJ/dq_i) v) = -v_i sum_k (M J v)_k D_ki                          (Hamilton.hs:375-387)
    U = 1/2 |x|^2:  grad U = J^T x;     U = sum_j (q_j^2 / 2 + 0.1 cos(q_j - q_(j+1))):  grad U_j = q_j - 0.1 sin(q_j - q_(j+1)) + 0.1 sin(q_(j-1) - q_j)
    dq = v,  dp = -(dT/dq + grad U)
`main` asserts that this form and the generic derivation (oracle/gen_golden.py `symbolic` + `evaluate_point`: sympy differentiates the
member's definition, mpmath evaluates the reference's formulas and cross-checks them against numerical differentiation of H) agree to
27 digits on the members where the generic one is cheap (CHECKED) before it is used for the others.

Per point: q, p, vel, dp, pe = U, keP = T, hamiltonian, cond_hint.  `vel` is the velocity fromPhase returns, which is also the qd the
momenta were made from and the dq of hamEqs (asserted equal at 30 digits): the file stores it once.  No K, no J.  The generator refuses a point with
cond K >= 1e4.  Points: examples.sample_config(spec, 0, 4).

Run:  python oracle/gen_golden_rect.py      (about twenty seconds; the output is committed and reproduces byte for byte)
"""
from __future__ import annotations

import json
import os
import sys

import mpmath as mp
import sympy as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hamilton_amd import examples as E      # noqa: E402
from oracle import gen_golden as G          # noqa: E402
import rect_family as F                     # noqa: E402

CHECKED = ["ln_thin", "ln_wide_g"]           # closed form == generic symbolic derivation: one cartesian U, one generalized U


def evaluate_closed_form(key, spec, qv, qdv):
    n, m = spec.n, spec.m
    c, a, b = F.coefficients(key)
    q = [mp.mpf(float(v)) for v in qv]
    qd = mp.matrix([mp.mpf(float(v)) for v in qdv])
    sn, cs = [mp.sin(t) for t in q], [mp.cos(t) for t in q]
    J, D, x = mp.matrix(m, n), mp.matrix(m, n), [mp.mpf(0)] * m
    for (k, j), w in c.items():
        J[k, j] += mp.mpf(w)
        x[k] += mp.mpf(w) * q[j]
    for (k, j), w in a.items():
        J[k, j] += mp.mpf(w) * cs[j]
        D[k, j] -= mp.mpf(w) * sn[j]
        x[k] += mp.mpf(w) * sn[j]
    for (k, j), w in b.items():
        J[k, j] -= mp.mpf(w) * sn[j]
        D[k, j] -= mp.mpf(w) * cs[j]
        x[k] += mp.mpf(w) * cs[j]
    M = mp.diag([mp.mpf(w) for w in spec.inertia])
    K = J.T * M * J
    p = K * qd
    Ki = K ** -1
    v = Ki * p
    u = M * (J * v)
    if spec.u_space == E.U_CARTESIAN:
        U = sum(t * t for t in x) / 2
        gU = J.T * mp.matrix(x)
    else:
        U = sum(q[j] * q[j] / 2 + mp.mpf(0.1) * mp.cos(q[j] - q[(j + 1) % n]) for j in range(n))
        gU = [q[j] - mp.mpf(0.1) * mp.sin(q[j] - q[(j + 1) % n]) + mp.mpf(0.1) * mp.sin(q[(j - 1) % n] - q[j]) for j in range(n)]
    dT = [-v[i] * sum(u[k] * D[k, i] for k in range(m)) for i in range(n)]
    keP = (v.T * p)[0] / 2
    cond = mp.norm(K, 1) * mp.norm(Ki, 1)
    assert cond < F.COND_LIMIT, (key, cond)
    f = G.fmt
    assert [f(t) for t in v] == [f(t) for t in qd], key       # fromPhase . toPhase = id: ONE vector serves as qd, vel and dq
    return dict(q=[f(t) for t in q], p=[f(t) for t in p], vel=[f(t) for t in v], dp=[f(-(dT[i] + gU[i])) for i in range(n)],
                pe=f(U), keP=f(keP), hamiltonian=f(keP + U), cond_hint=f(cond))


def main():
    mp.mp.dps = G.DIGITS
    blocks = {}
    for key in F.KEYS:
        spec = F.spec(key)
        q, qd = E.sample_config(spec, 0, F.NPOINTS)
        pts = [evaluate_closed_form(key, spec, q[:, i], qd[:, i]) for i in range(F.NPOINTS)]
        if key in CHECKED:
            S = G.symbolic(spec)
            for i in range(2):
                ref = G.evaluate_point(spec, S, q[:, i], qd[:, i])
                assert ref["dq"] == ref["vel"]
                for name in ("p", "vel", "dp", "pe", "keP", "hamiltonian", "cond_hint"):
                    av = ref[name] if isinstance(ref[name], list) else [ref[name]]
                    bv = pts[i][name] if isinstance(pts[i][name], list) else [pts[i][name]]
                    for r, w in zip(av, bv):
                        assert abs(mp.mpf(r) - mp.mpf(w)) <= mp.mpf(10) ** -27 * (1 + abs(mp.mpf(r))), (key, name, r, w)
            print("closed form == symbolic derivation:", key, flush=True)
        blocks[key] = dict(system=spec.name, m=spec.m, n=spec.n, inertia=list(spec.inertia), points=pts)
        print(spec.name, "n", spec.n, "m", spec.m, "max cond", max(float(p["cond_hint"]) for p in pts), flush=True)
    doc = dict(generator="oracle/gen_golden_rect.py (sympy %s, mpmath %s, %d digits)" % (sp.__version__, mp.__version__, G.DIGITS),
               note="derived fixtures for tests/rect_family.py from the closed-form mechanics of a separable coordinate map (LU at 50 digits; "
                    "checked by the generator against the symbolic derivation of oracle/gen_golden.py on %s); points from "
                    "examples.sample_config(spec, 0, %d); `vel` = fromPhase's velocities = the qd of toPhase = the dq of hamEqs; no K, no J" % (", ".join(CHECKED), F.NPOINTS),
               members=F.KEYS, blocks=blocks)
    path = os.path.join(G.OUT, "rect_family.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
