"""The fused Lyapunov stepper (hamk_lyapunov_steps) on one MI355X against the same computation done from outside, back to back in
one process:
  rate    doublePendulum, B = 2^20, dt = 0.01, 1000 steps per "launch" renormalised every 10:
            (a) one hamk_lyapunov_steps call of 100 intervals of 10 steps;
            (b) what a host had to do before: 100 times { hamk_rk4_steps of 10 steps on the ensemble, the same on a shadow
                ensemble, then delta = s - y, d = |delta|, logsum += log(d / d0), s = y + d0 delta / d with torch operations }
          launches alternate between the two, medians over --launches launches after --warmup; trajectory-steps/s (main
          trajectories), right-hand sides/s (both trajectories: 8 per step) and the ratio (a) / (b);
  build   hamk_lyapunov_build_info (bytes, spills, registers) for doublePendulum, chain8, chain16;
  map     the share of a --grid x --grid lattice of (theta1, theta2) starts at rest with lambda T > 3 at T = 100 (the lambda
          array itself is not kept).
Appends one JSON line per figure to profiles/lyapunov_rate.jsonl.  Needs the GPU: there is no fall-back.
  python scripts/lyapunov_rate.py [--launches 12] [--warmup 3] [--grid 512] [--out profiles/lyapunov_rate.jsonl]"""
import argparse
import json
import math
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
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--d0", type=float, default=1e-7)
    ap.add_argument("--grid", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lyapunov_rate.jsonl"))
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
    dt, B, K, every, d0 = 0.01, a.batch, a.steps, a.every, a.d0
    nint = K // every
    q, qd = examples.sample_config(spec, 0, B)
    start = api.toPhase(s, api.Config(torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda()))
    c = 1.0 / math.sqrt(2.0 * spec.n)
    # (a) state, w, logsum; (b) state, shadow, logsum
    fused = dict(y=api.Phase(start.positions.clone(), start.momenta.clone()),
                 w=api.Phase(torch.full_like(start.positions, c), torch.full_like(start.momenta, c)),
                 logsum=torch.zeros(B, dtype=torch.float64, device="cuda"))
    outside = dict(y=api.Phase(start.positions.clone(), start.momenta.clone()),
                   s=api.Phase(start.positions + d0 * c, start.momenta + d0 * c),
                   logsum=torch.zeros(B, dtype=torch.float64, device="cuda"))

    def launch_fused():
        api.lyapunovSteps(dt, nint, every, s, fused["y"], w=fused["w"], d0=d0, logsum=fused["logsum"], inplace=True)

    def launch_outside():
        y, sh = outside["y"], outside["s"]
        for _ in range(nint):
            api.rk4Steps(dt, every, s, y, inplace=True)
            api.rk4Steps(dt, every, s, sh, inplace=True)
            dq, dp = sh.positions - y.positions, sh.momenta - y.momenta
            d = torch.sqrt((dq * dq).sum(0) + (dp * dp).sum(0))
            outside["logsum"] += torch.log(d / d0)
            torch.addcdiv(y.positions, dq, d, value=d0, out=sh.positions)
            torch.addcdiv(y.momenta, dp, d, value=d0, out=sh.momenta)
    variants = [("fused hamk_lyapunov_steps", launch_fused), ("outside: 2 x hamk_rk4_steps + torch renormalisation", launch_outside)]
    times = {name: [] for name, _ in variants}
    for r in range(a.warmup + a.launches):
        for name, fn in variants:                           # alternating: every variant sees the same state of the machine
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    result = {}
    for name, _ in variants:
        t = float(np.median(times[name]))
        result[name] = {"figure": "rate", "system": spec.name, "B": B, "steps_per_launch": K, "every": every, "dt": dt, "d0": d0, "variant": name,
                        "launches": len(times[name]), "median_launch_s": t, "min_launch_s": float(min(times[name])),
                        "max_launch_s": float(max(times[name])), "trajectory_steps_per_s": B * K / t, "rhs_per_s": B * K * 8 / t}
    result[variants[0][0]]["rate_over_outside"] = result[variants[1][0]]["median_launch_s"] / result[variants[0][0]]["median_launch_s"]
    # the two ways agree on what they computed (different rounding: the chaotic lanes drift apart, the median does not)
    lam = lambda x: (x / ((a.warmup + a.launches) * K * dt)).cpu().numpy()
    result[variants[0][0]]["median_lambda"] = float(np.nanmedian(lam(fused["logsum"])))
    result[variants[1][0]]["median_lambda"] = float(np.nanmedian(lam(outside["logsum"])))
    for name, _ in variants:
        emit(result[name])
    for name in ("doublePendulum", "chain8", "chain16"):
        emit({"figure": "build", "system": name, "lyapunov_build_info": api.system_from_spec(examples.get(name)).lyapunov_build_info.strip()})

    # ---- the lambda map --------------------------------------------------------------------------------------------
    G, T = a.grid, 100.0
    th = torch.linspace(-math.pi, math.pi, G, dtype=torch.float64, device="cuda")
    q0 = torch.stack([th.repeat_interleave(G), th.repeat(G)]).contiguous()
    ph = api.toPhase(s, api.Config(q0, torch.zeros_like(q0)))
    w, ls = None, None
    nsteps = int(round(T / dt))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):                                      # ten launches of T / 10 each, w and logsum carried
        ph, w, ls = api.lyapunovSteps(dt, nsteps // every // 10, every, s, ph, w=w, d0=d0, logsum=ls)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    st = s.last_status
    lt = ls.cpu().numpy()
    fin = np.isfinite(lt)
    emit({"figure": "map", "system": spec.name, "grid": [G, G], "starts": "theta1, theta2 in [-pi, pi], at rest", "T": T, "dt": dt, "every": every,
          "d0": d0, "seconds": t1 - t0, "finite": int(fin.sum()), "flagged_last_launch": int((st != 0).sum()),
          "share_lambda_T_above_3": float((lt[fin] > 3.0).mean()), "median_lambda": float(np.median(lt[fin]) / T),
          "largest_lambda": float(lt[fin].max() / T)})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
