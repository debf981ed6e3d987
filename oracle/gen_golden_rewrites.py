#!/usr/bin/env python3
"""Generate tests/golden/rewrite_family.json: 50-digit fixtures for the system family of tests/rewrite_family.py.

TEST INFRASTRUCTURE, derived data like the rest of tests/golden: oracle/gen_golden.py's `symbolic` (sympy differentiates the
definition; every Python float enters as the exact rational it denotes) and `evaluate_point` (mpmath evaluates the reference's
formulas at 50 digits and cross-checks them against numerical differentiation of H) applied to every member of rewrite_family.KEYS at
NPOINTS points of the member's sampling box (examples.sample_config(spec, 0, NPOINTS)); the range members -- one coordinate -- also at
the four corners of their (q, qd) box, where the exponentials' arguments are extreme.  Each point carries the evaluate_point record
without `jac`.  mpmath's exponent range is unbounded: exp(q0 - 735) is a 50-digit number here, not a subnormal.
The generator refuses a member with cond K >= 1e3 at any point, or with a non-finite value: the tests built on this file leave out
nothing.

Run:  python oracle/gen_golden_rewrites.py      (about half a minute; the output is committed and reproduces byte for byte)
"""
from __future__ import annotations

import itertools
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
import rewrite_family as F                  # noqa: E402

NPOINTS = 6
COND_LIMIT = 1e3


def evaluate(spec, S, qv, qdv):
    pt = G.evaluate_point(spec, S, qv, qdv)
    del pt["jac"]
    assert float(pt["cond_hint"]) < COND_LIMIT, (spec.name, pt["cond_hint"])
    for key, val in pt.items():
        for x in (val if isinstance(val, list) else [val]):
            assert mp.isfinite(mp.mpf(x)), (spec.name, key, x)
    return pt


def main():
    mp.mp.dps = G.DIGITS
    blocks = {}
    for key in F.KEYS:
        spec = F.spec(key)
        assert spec.n <= 3 and spec.m <= 4, key
        S = G.symbolic(spec)
        q, qd = E.sample_config(spec, 0, NPOINTS)
        at = [(q[:, i], qd[:, i]) for i in range(NPOINTS)]
        if key in F.RANGE_KEYS:
            lo_hi = list(spec.q_box) + list(spec.qd_box)
            at += [(c[:spec.n], c[spec.n:]) for c in itertools.product(*lo_hi)]
        blocks[key] = dict(system=spec.name, m=spec.m, n=spec.n, inertia=list(spec.inertia), points=[evaluate(spec, S, a, b) for a, b in at])
        print(spec.name, "n", spec.n, "m", spec.m, "points", len(at), "max cond", max(float(p["cond_hint"]) for p in blocks[key]["points"]), flush=True)
    doc = dict(generator="oracle/gen_golden_rewrites.py (sympy %s, mpmath %s, %d digits)" % (sp.__version__, mp.__version__, G.DIGITS),
               note="derived fixtures for tests/rewrite_family.py: oracle/gen_golden.py evaluate_point (no `jac`); points from "
                    "examples.sample_config(spec, 0, %d), the range members also at the corners of their box" % NPOINTS,
               blocks=blocks)
    path = os.path.join(G.OUT, "rewrite_family.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
