#!/usr/bin/env python
"""What a build of libhamk.so hands to the GPU, as SHA-256s: for a host-side change that must move no generated source and no code object.

    python scripts/lib_identity.py --lib A/libhamk.so --out a.json      one table per library (hiprtc needs no GPU; HAMK_CACHE=0)
    python scripts/lib_identity.py --compare a.json b.json [...]        exit 1 and the differing entries if any two tables differ

Cases: every golden system on the lane mapping, chain12 / chain17 on the quad mapping, the smallest dense-quad member of
tests/rect_family.py, chain17 on the wave mapping, chain33.  Per case the generated source and build_info; the four existing companion modules' sources
(symplectic, Lyapunov, Poincare, exit-time) for the lane systems; both code objects for doublePendulum, chain8, chain12 (quad) and chain17 (wave)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LANE = ["pendulum", "doublePendulum", "room", "twoBody", "spring", "bezier", "threeBodyPolar", "chain4", "opcodeZoo", "chain8"]
CASES = [(name, "lane") for name in LANE] + [("chain12", "quad"), ("chain17", "quad"), ("rect:qd_eq", None), ("chain17", "wave"), ("chain33", None)]
WITH_CODE = {("doublePendulum", "lane"), ("chain8", "lane"), ("chain12", "quad"), ("chain17", "wave")}


def one(lib, name, mapping):
    os.environ["HAMK_CACHE"] = "0"
    from hamilton_amd import _abi, api, examples
    _abi.LIB_PATH = lib
    import rect_family
    spec = rect_family.spec(name[5:]) if name.startswith("rect:") else examples.get(name)
    s = api.system_from_spec(spec, rect_family.options(mapping))
    sha = lambda b: hashlib.sha256(b if isinstance(b, bytes) else b.encode()).hexdigest()
    row = {"source": sha(s.source), "build_info": sha(s.build_info)}
    if mapping == "lane":
        row["symplectic_source"] = sha(s.symplectic_source)
        row["lyapunov_source"] = sha(s.lyapunov_source)
        row["poincare_source"] = sha(s.poincare_source)
        row["exit_source"] = sha(s.exit_source)
    if (name, mapping) in WITH_CODE:
        row["code_object_0"], row["code_object_1"] = sha(s.code_object(0)), sha(s.code_object(1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--out")
    ap.add_argument("--case", nargs=2)
    ap.add_argument("--compare", nargs="+")
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    if a.compare:
        tables = [json.load(open(p)) for p in a.compare]
        bad = [(p, k) for p, t in zip(a.compare[1:], tables[1:]) for k in sorted(set(t) | set(tables[0])) if t.get(k) != tables[0].get(k)]
        print(json.dumps({"identical": not bad, "differ": bad}))
        return 1 if bad else 0
    if a.case:
        print(json.dumps(one(a.lib, a.case[0], None if a.case[1] == "auto" else a.case[1])))
        return 0

    def child(case):
        r = subprocess.run([sys.executable, __file__, "--lib", a.lib, "--case", case[0], case[1] or "auto"], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{case}: {r.stderr[-800:]}")
        return json.loads(r.stdout.strip().splitlines()[-1])
    with ThreadPoolExecutor(a.j) as ex:
        table = {f"{name}/{mapping or 'auto'}": row for (name, mapping), row in zip(CASES, ex.map(child, CASES))}
    with open(a.out, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
