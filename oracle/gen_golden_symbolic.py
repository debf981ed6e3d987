#!/usr/bin/env python3
"""Generate tests/golden/symbolic_family.json: 50-digit fixtures for the system family of tests/symbolic_family.py.

TEST INFRASTRUCTURE, derived data like the rest of tests/golden: oracle/gen_golden.py's `symbolic` (sympy differentiates the
definition) and `evaluate_point` (mpmath evaluates the reference's formulas at 50 digits and cross-checks them against numerical
differentiation of H) applied to every member of symbolic_family.SEEDS, at NPOINTS points of the member's sampling box
(examples.sample_config(spec, 0, NPOINTS): velocities non-zero).  Each point carries the evaluate_point record without `jac`, and
the three terms the generator's symbolic right-hand side emits as text:
    K   the n x n matrix J^T M J                                  (mass_matrix_sym)
    dT  the vector -(M J v) . ((dJ/dq_i) v) at v = qd             (dT_sym)
    gU  grad U                                                    (gU_sym)
The generator refuses a member whose K has cond K >= 1e4 at any point: the tests built on this file leave out nothing.

Run:  python oracle/gen_golden_symbolic.py      (about ten seconds; the output is committed and reproduces byte for byte)
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
import symbolic_family as F                 # noqa: E402

NPOINTS = 8
COND_LIMIT = 1e4


def evaluate(spec, S, qv, qdv):
    pt = G.evaluate_point(spec, S, qv, qdv)
    del pt["jac"]
    q = [mp.mpf(v) for v in qv]
    v = mp.matrix([mp.mpf(x) for x in qdv])
    M = mp.diag([mp.mpf(w) for w in spec.inertia])
    J = G.mat(S["J"](*q))
    dJ = [G.mat(r) for r in S["dJ"](*q)]
    K = J.T * M * J
    u = M * (J * v)
    # an entry whose terms cancel analytically (a polar K01) comes out as 1e-50 times their magnitude: that is the evaluation's own
    # rounding, not a value -- written as 0
    size = max([mp.mpf(1)] + [abs(K[a, a]) for a in range(spec.n)])
    clean = lambda x: G.fmt(x) if abs(x) > mp.mpf(10) ** -40 * size else "0.0"
    pt["K"] = [[clean(K[a, b]) for b in range(spec.n)] for a in range(spec.n)]
    pt["dT"] = [clean(-(u.T * (dJ[i] * v))[0]) for i in range(spec.n)]
    pt["gU"] = [clean(g) for g in S["gU"](*q)]
    assert float(pt["cond_hint"]) < COND_LIMIT, (spec.name, pt["cond_hint"])
    return pt


def main():
    mp.mp.dps = G.DIGITS
    blocks = {}
    for seed in F.SEEDS:
        spec = F.spec(seed)
        S = G.symbolic(spec)
        q, qd = E.sample_config(spec, 0, NPOINTS)
        blocks[str(seed)] = dict(system=spec.name, m=spec.m, n=spec.n, inertia=list(spec.inertia),
                                 points=[evaluate(spec, S, q[:, i], qd[:, i]) for i in range(NPOINTS)])
        print(spec.name, "n", spec.n, "m", spec.m, "max cond", max(float(p["cond_hint"]) for p in blocks[str(seed)]["points"]), flush=True)
    doc = dict(generator="oracle/gen_golden_symbolic.py (sympy %s, mpmath %s, %d digits)" % (sp.__version__, mp.__version__, G.DIGITS),
               note="derived fixtures for tests/symbolic_family.py: oracle/gen_golden.py evaluate_point (no `jac`) plus K = J^T M J, "
                    "dT = -(M J v) . ((dJ/dq_i) v) at v = qd and gU = grad U; points from examples.sample_config(spec, 0, %d)" % NPOINTS,
               blocks=blocks)
    path = os.path.join(G.OUT, "symbolic_family.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
