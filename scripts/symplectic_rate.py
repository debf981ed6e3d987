"""The symplectic stepper (hamk_symplectic_steps) beside the RK4 kernel on one MI355X, back to back in one process:
  rate    doublePendulum, B = 2^20, 1000 steps per launch, dt = 0.01: hamk_rk4_steps at the library's own options against
          hamk_symplectic_steps at order 2 with 4 and 8 iterations and at order 4 with 4 -- launches alternate between the variants,
          medians over --launches launches after --warmup; trajectory-steps/s and right-hand sides/s (RK4: 4 per step; the
          symplectic stepper: iters per substep, 1 or 3 substeps per step);
  energy  the per-launch energy error max / median over the ensemble of |H - H0| / max(1, |H0|) of both steppers over
          --energy-steps steps (launches of 1000) on the systems bench.py --full reports its drift for.
Appends one JSON line per figure to profiles/symplectic_rate.jsonl.  Needs the GPU: there is no fall-back.
  python scripts/symplectic_rate.py [--launches 12] [--warmup 3] [--energy-steps 100000] [--out profiles/symplectic_rate.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from hamilton_amd import api, examples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--energy-steps", type=int, default=100000)
    ap.add_argument("--energy-batch", type=int, default=1 << 14)
    ap.add_argument("--energy-systems", default="doublePendulum,pendulum")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "symplectic_rate.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU"
    torch.cuda.set_device(0)
    rows = []

    def emit(row):
        row["device"] = torch.cuda.get_device_name(0)
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- rate ------------------------------------------------------------------------------------------------------
    spec = examples.get("doublePendulum")
    s = api.system_from_spec(spec)
    dt, B, K = 0.01, a.batch, a.steps
    q, qd = examples.sample_config(spec, 0, B)
    start = api.toPhase(s, api.Config(torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda()))
    variants = [("rk4", None, 4), ("symplectic order 2 iters 4", (2, 4), 4), ("symplectic order 2 iters 8", (2, 8), 8),
                ("symplectic order 4 iters 4", (4, 4), 12)]
    states = {name: api.Phase(start.positions.clone(), start.momenta.clone()) for name, _, _ in variants}
    times = {name: [] for name, _, _ in variants}

    def launch(name, how):
        st = states[name]
        if how is None:
            api.rk4Steps(dt, K, s, st, inplace=True)
        else:
            api.symplecticSteps(dt, K, s, st, order=how[0], iters=how[1], inplace=True)
    for r in range(a.warmup + a.launches):
        for name, how, _ in variants:                       # alternating: every variant sees the same state of the machine
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            launch(name, how)
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    base = None
    for name, how, rhs in variants:
        t = float(np.median(times[name]))
        row = {"figure": "rate", "system": spec.name, "B": B, "steps_per_launch": K, "dt": dt, "variant": name, "launches": len(times[name]),
               "median_launch_s": t, "min_launch_s": float(min(times[name])), "max_launch_s": float(max(times[name])),
               "trajectory_steps_per_s": B * K / t, "rhs_per_step": rhs, "rhs_per_s": B * K * rhs / t}
        if how is None:
            base = row
        else:
            row["rhs_rate_over_rk4"] = row["rhs_per_s"] / base["rhs_per_s"]
            row["step_rate_over_rk4"] = row["trajectory_steps_per_s"] / base["trajectory_steps_per_s"]
        emit(row)
    emit({"figure": "build", "system": spec.name, "symplectic_build_info": s.symplectic_build_info.strip(), "rk4_options": s.options(B)})

    # ---- energy ----------------------------------------------------------------------------------------------------
    for sysname in [x for x in a.energy_systems.split(",") if x]:
        spec = examples.get(sysname)
        s = api.system_from_spec(spec)
        Be, nl = a.energy_batch, max(1, a.energy_steps // 1000)
        q, qd = examples.sample_config(spec, 0, Be)
        start = api.toPhase(s, api.Config(torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda()))
        H0 = api.hamiltonian(s, start)
        scale = torch.clamp(H0.abs(), min=1.0)
        for name, how in (("rk4", None), ("symplectic order 2 iters 8", (2, 8)), ("symplectic order 4 iters 8", (4, 8))):
            st = api.Phase(start.positions.clone(), start.momenta.clone())
            worst, med, resid = [], [], 0.0
            for _ in range(nl):
                if how is None:
                    api.rk4Steps(spec.dt, 1000, s, st, inplace=True)
                else:
                    _, res = api.symplecticSteps(spec.dt, 1000, s, st, order=how[0], iters=how[1], inplace=True, with_residual=True)
                    resid = max(resid, float(torch.nan_to_num(res, nan=0.0, posinf=0.0).max()))
                e = ((api.hamiltonian(s, st) - H0).abs() / scale)
                e = torch.nan_to_num(e, nan=float("inf"))
                worst.append(float(e.max()))
                med.append(float(e.median()))
            pick = sorted({0, min(9, nl - 1), nl - 1})
            emit({"figure": "energy", "system": sysname, "B": Be, "dt": spec.dt, "launches_of_1000_steps": nl, "variant": name,
                  "median_lane_rel_energy_error_after_launch": {str(i + 1): med[i] for i in pick},
                  "worst_lane_rel_energy_error_after_launch": {str(i + 1): worst[i] for i in pick},
                  "median_lane_max_over_first_half": max(med[:max(1, nl // 2)]), "median_lane_max_over_second_half": max(med[nl // 2:]),
                  "largest_residual": resid if how else None})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
