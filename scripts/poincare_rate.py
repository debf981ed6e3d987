"""The fused Poincare-section stepper (hamk_poincare_steps) on one MI355X against the same computation done from outside, back to
back in one process:
  rate    doublePendulum, B = 2^20, dt = 0.01, 1000 steps per "launch", section theta1 = 0 (mod 2 pi) upward:
            (a) one hamk_poincare_steps call of 1000 steps;
            (b) what a host had to do before: 1000 times { keep y0, hamk_rk4_steps of 1 step, the cell test on theta1 and a
                LINEAR interpolation of the crossing with torch operations, scattered into the same fixed-size buffers }
          launches alternate between the two, medians over --launches launches after --warmup; the hit counts are zeroed before
          every launch (outside the clock) so that no lane overflows its --max-hits rows; trajectory-steps/s, right-hand
          sides/s (4 per step) and the ratio (b) / (a);
  build   hamk_poincare_build_info (bytes, spills, registers) for pendulum, doublePendulum, opcodeZoo, chain8, chain16;
  section --starts starts on ONE energy shell of the double pendulum (theta1 = 0, theta2 spread over [-1, 1], p2 = 0, p1 > 0 from
          H = E), T = 200: the counts of hits, of lanes that overflowed and of flagged lanes, and how far the hits' energy is from E
          (the points themselves are not kept).
Appends one JSON line per figure to profiles/poincare_rate.jsonl.  Needs the GPU: there is no fall-back.
  python scripts/poincare_rate.py [--launches 12] [--warmup 3] [--max-hits 32] [--starts 400] [--out profiles/poincare_rate.jsonl]"""
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

TWO_PI = 2.0 * math.pi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--max-hits", type=int, default=32)
    ap.add_argument("--starts", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poincare_rate.jsonl"))
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
    dt, B, K, R, n = 0.01, a.batch, a.steps, a.max_hits, spec.n
    q, qd = examples.sample_config(spec, 0, B)
    start = api.toPhase(s, api.Config(torch.from_numpy(q).cuda(), torch.from_numpy(qd).cuda()))
    zeros = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")

    def state():
        return dict(y=api.Phase(start.positions.clone(), start.momenta.clone()),
                    hits=api.Hits(zeros(R, n, B), zeros(R, n, B), zeros(R, B), zeros(B, dtype=torch.int32)), step0=0, most=0)
    fused, outside = state(), state()
    lanes = torch.arange(B, device="cuda")

    def launch_fused():
        api.poincareSteps(dt, K, s, fused["y"], 0, 0.0, TWO_PI, 1, hits=fused["hits"], step0=fused["step0"], inplace=True)

    def launch_outside():
        y, h = outside["y"], outside["hits"]
        for k in range(K):
            q0, p0 = y.positions.clone(), y.momenta.clone()
            api.rk4Steps(dt, 1, s, y, inplace=True)
            c1 = torch.floor(y.positions[0] / TWO_PI)
            up = c1 > torch.floor(q0[0] / TWO_PI)
            th = (TWO_PI * c1 - q0[0]) / (y.positions[0] - q0[0])
            ok = up & (h.count < R)
            row = h.count.long().clamp(max=R - 1)

            def put(buf, at, new):                          # full-width and free of host synchronisation: no boolean indexing
                flat = buf.view(-1)
                flat.scatter_(0, at, torch.where(ok, new, flat.gather(0, at)))
            for j in range(n):
                at = row * (n * B) + j * B + lanes
                put(h.positions, at, q0[j] + th * (y.positions[j] - q0[j]))
                put(h.momenta, at, p0[j] + th * (y.momenta[j] - p0[j]))
            put(h.times, row * B + lanes, float(outside["step0"] + k) + th)
            h.count += up.to(torch.int32)
    variants = [("fused hamk_poincare_steps", launch_fused, fused), ("outside: hamk_rk4_steps per step + torch cell test and linear interpolation", launch_outside, outside)]
    times = {name: [] for name, _, _ in variants}
    for r in range(a.warmup + a.launches):
        for name, fn, st in variants:                       # alternating: every variant sees the same state of the machine
            st["hits"].count.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append(time.perf_counter() - t0)
            st["step0"] += K
            st["most"] = max(st["most"], int(st["hits"].count.max()))
    result = {}
    for name, _, st in variants:
        t = float(np.median(times[name]))
        result[name] = {"figure": "rate", "system": spec.name, "B": B, "steps_per_launch": K, "dt": dt, "section": "theta1 = 0 (mod 2 pi), upward",
                        "max_hits": R, "variant": name, "launches": len(times[name]), "median_launch_s": t, "min_launch_s": float(min(times[name])),
                        "max_launch_s": float(max(times[name])), "trajectory_steps_per_s": B * K / t, "rhs_per_s": B * K * 4 / t,
                        "most_hits_of_a_lane_in_a_launch": st["most"], "hits_last_launch": int(st["hits"].count.sum())}
    result[variants[0][0]]["rate_over_outside"] = result[variants[1][0]]["median_launch_s"] / result[variants[0][0]]["median_launch_s"]
    for name, _, _ in variants:
        emit(result[name])
    for name in ("pendulum", "doublePendulum", "opcodeZoo", "chain8", "chain16"):
        emit({"figure": "build", "system": name, "poincare_build_info": api.system_from_spec(examples.get(name)).poincare_build_info.strip()})
    del fused, outside

    # ---- one section -----------------------------------------------------------------------------------------------
    G, T, rows_max = a.starts, 200.0, 256
    q0 = torch.stack([torch.zeros(G, dtype=torch.float64, device="cuda"), torch.linspace(-1.0, 1.0, G, dtype=torch.float64, device="cuda")]).contiguous()
    zero, unit = torch.zeros_like(q0), torch.stack([torch.ones(G, dtype=torch.float64, device="cuda"), torch.zeros(G, dtype=torch.float64, device="cuda")]).contiguous()
    u = api.hamiltonian(s, api.Phase(q0, zero))                              # H(q, 0) = U(q)
    half_kinv = api.hamiltonian(s, api.Phase(q0, unit)) - u                  # H(q, (1, 0)) - U = K^-1_11 / 2
    E = float(u.max()) + 0.5
    p0 = torch.stack([torch.sqrt((E - u) / half_kinv), torch.zeros(G, dtype=torch.float64, device="cuda")]).contiguous()
    nsteps = int(round(T / dt))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ph, hits = api.poincareSteps(dt, nsteps, s, api.Phase(q0, p0), 0, 0.0, TWO_PI, 1, max_hits=rows_max)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    cnt = hits.count.cpu().numpy()
    m = torch.arange(rows_max, device="cuda")[:, None] < hits.count.clamp(max=rows_max)[None, :]
    hq, hp = hits.positions.permute(1, 0, 2)[:, m].contiguous(), hits.momenta.permute(1, 0, 2)[:, m].contiguous()
    he = api.hamiltonian(s, api.Phase(hq, hp)) if hq.shape[1] else torch.zeros(0)
    emit({"figure": "section", "system": spec.name, "starts": G, "shell": "theta1 = 0, theta2 in [-1, 1], p2 = 0, p1 > 0 with H = E", "E": E, "T": T,
          "dt": dt, "section": "theta1 = 0 (mod 2 pi), upward", "max_hits": rows_max, "seconds": t1 - t0, "hits": int(cnt.sum()),
          "hits_stored": int(m.sum()), "fewest_per_lane": int(cnt.min()), "most_per_lane": int(cnt.max()), "lanes_overflowed": int((cnt > rows_max).sum()),
          "flagged": int((s.last_status != 0).sum()), "largest_energy_error_of_a_hit": float((he - E).abs().max()) if hq.shape[1] else None,
          "largest_energy_error_of_the_final_state": float((api.hamiltonian(s, ph) - E).abs().max())})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
