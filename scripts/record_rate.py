"""The fused recording stepper (hamk_record_steps) on one MI355X against the only route there was before, back to back in one
process.
  doublePendulum, B = 1, 4096 and 2^20 from examples.sample_config, dt = 0.01, 1000 steps per launch, every in {1, 10, 100}.
    (a)   hamk_record_steps with state rows + hout;
    (a')  state rows only;
    (a'') hout only;
    (a0)  every = nsteps + 1: stepping alone (row 0 is still written, once per launch);
    (b)   per row one hamk_rk4_steps launch of `every` steps, a copy of q, p into the row, and hamk_observe_batch into hout's row.
  (b) steps with the headline kernel (table-and-rotation sincos); the fused launch steps with the companions' TRIG_FULL step: the rows
  of the two are not the same bits, and the step rates differ.
  Every launch starts from the same fresh state (cloned outside the clock) and writes into row buffers allocated once: no variant
  reads them.  Launches alternate between the variants; medians over --launches launches after --warmup, host clock between two
  device synchronisations.  Reported per (B, every): the medians, (b) / (a), the bytes the rows take and the achieved store rate of
  (a') and (a) over the time they take beyond (a0).
  bench  `bench.py --gpus 1 --steps 20 --warmup 5` in a child process afterwards: the headline line of the same session.
  build  hamk_record_build_info (bytes, spills, registers) for pendulum, doublePendulum, opcodeZoo, chain8, chain16.
Appends one JSON line per figure to profiles/record_rate.jsonl.  Needs the GPU: there is no fall-back.
  python scripts/record_rate.py [--launches 7] [--warmup 2] [--steps 1000] [--sizes 1 4096 1048576] [--out profiles/record_rate.jsonl]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from hamilton_amd import _abi, api, examples

DEVICE = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 4096, 1 << 20])
    ap.add_argument("--every", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "record_rate.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU"
    torch.cuda.set_device(0)
    L = _abi.lib()
    rows = []

    def emit(row):
        row["device"] = torch.cuda.get_device_name(0)
        rows.append(row)
        print(json.dumps(row), flush=True)

    spec = examples.get("doublePendulum")
    s = api.system_from_spec(spec)
    dt, K, n = 0.01, a.steps, spec.n
    _abi.check(L.hamk_set_stream(s._h, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    for B in a.sizes:
        q_h, qd_h = examples.sample_config(spec, 17, B)
        q0 = torch.from_numpy(np.ascontiguousarray(q_h)).cuda()
        p0 = api.momenta(s, api.Config(q0, torch.from_numpy(np.ascontiguousarray(qd_h)).cuda()))
        st = torch.zeros(B, dtype=torch.int32, device="cuda")
        for every in a.every:
            nrows = K // every + 1
            rq = torch.empty((nrows, n, B), dtype=torch.float64, device="cuda")           # allocated once per (B, every), outside the clock
            rp = torch.empty_like(rq)
            rh = torch.empty((nrows, B), dtype=torch.float64, device="cuda")

            def fused(states, energy, ev):
                def launch(q, p):
                    _abi.check(L.hamk_record_steps(s._h, B, q.data_ptr(), p.data_ptr(), dt, K, ev, nrows, rq.data_ptr() if states else None,
                                                   rp.data_ptr() if states else None, rh.data_ptr() if energy else None, 0, st.data_ptr(), DEVICE))
                return launch

            def separate(q, p):
                rq[0].copy_(q); rp[0].copy_(p)
                _abi.check(L.hamk_observe_batch(s._h, B, q.data_ptr(), p.data_ptr(), None, None, rh[0].data_ptr(), st.data_ptr(), DEVICE))
                for k in range(1, nrows):
                    _abi.check(L.hamk_rk4_steps(s._h, B, q.data_ptr(), p.data_ptr(), dt, every, st.data_ptr(), DEVICE))
                    rq[k].copy_(q); rp[k].copy_(p)
                    _abi.check(L.hamk_observe_batch(s._h, B, q.data_ptr(), p.data_ptr(), None, None, rh[k].data_ptr(), st.data_ptr(), DEVICE))
                rest = K - (nrows - 1) * every
                if rest:
                    _abi.check(L.hamk_rk4_steps(s._h, B, q.data_ptr(), p.data_ptr(), dt, rest, st.data_ptr(), DEVICE))

            A, AS, AH, A0 = "(a) state rows + hout", "(a') state rows only", "(a'') hout only", "(a0) every = nsteps + 1: stepping alone"
            BB = "(b) per row: hamk_rk4_steps + copies + hamk_observe_batch"
            variants = [(A, fused(True, True, every)), (AS, fused(True, False, every)), (AH, fused(False, True, every)), (A0, fused(True, True, K + 1)),
                        (BB, separate)]
            times = {name: [] for name, _ in variants}
            for r in range(a.warmup + a.launches):
                for name, launch in variants:                  # alternating: every variant sees the same state of the machine
                    q, p = q0.clone(), p0.clone()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    launch(q, p)
                    torch.cuda.synchronize()
                    if r >= a.warmup:
                        times[name].append(time.perf_counter() - t0)
            med = {name: float(np.median(v)) for name, v in times.items()}
            state_bytes, h_bytes = 2 * nrows * n * B * 8, nrows * B * 8
            for name, _ in variants:
                row = {"figure": "rate", "system": spec.name, "B": B, "steps_per_launch": K, "every": every, "rows": nrows, "dt": dt, "variant": name,
                       "launches": len(times[name]), "median_launch_s": med[name], "min_launch_s": float(min(times[name])),
                       "max_launch_s": float(max(times[name])), "trajectory_steps_per_s": B * K / med[name]}
                if name != A:
                    row["time_over_a"] = med[name] / med[A]
                emit(row)
            extra = lambda name: max(med[name] - med[A0], 0.0)
            emit({"figure": "stores", "system": spec.name, "B": B, "every": every, "rows": nrows, "state_row_bytes": state_bytes, "hout_bytes": h_bytes,
                  "a_prime_seconds_beyond_a0": extra(AS), "a_prime_store_GB_per_s_over_that": (state_bytes / extra(AS) / 1e9) if extra(AS) > 0 else None,
                  "a_prime_store_GB_per_s_over_the_launch": state_bytes / med[AS] / 1e9,
                  "a_seconds_beyond_a0": extra(A), "a_store_GB_per_s_over_the_launch": (state_bytes + h_bytes) / med[A] / 1e9,
                  "b_over_a": med[BB] / med[A], "a0_trajectory_steps_per_s": B * K / med[A0]})
            del rq, rp, rh
            torch.cuda.empty_cache()
    for name in ("pendulum", "doublePendulum", "opcodeZoo", "chain8", "chain16"):
        emit({"figure": "build", "system": name, "record_build_info": api.system_from_spec(examples.get(name)).record_build_info.strip()})
    if not a.no_bench:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], capture_output=True, text=True,
                           timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        emit({"figure": "bench", "command": "bench.py --gpus 1 --steps 20 --warmup 5", "returncode": r.returncode, "line": json.loads(line[-1]) if line else None})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
