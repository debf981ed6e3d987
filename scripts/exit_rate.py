"""The fused exit-time stepper (hamk_exit_steps) on one MI355X: the flip-time map of the double pendulum, against the two routes
there were before, back to back in one process.
  doublePendulum, B = 2^20 on a 1024 x 1024 grid of (theta1, theta2) in (-pi, pi)^2, p = 0, dt = 0.01, gates theta1, theta2 in
  [-pi, pi], 10^4 steps per launch.  ROW-MAJOR: lane = 1024 i1 + i2, so a wavefront holds 64 neighbours of one grid row.
    (a)  one hamk_exit_steps call;
    (a') the same call on the same starts in a SHUFFLED lane order (a fixed permutation): what lane coherence is worth;
    (b)  what a host had to do before: per step { keep y0, hamk_rk4_steps of 1 step, the gate test and a LINEAR interpolation of
         the exit time with torch operations, stopped lanes put back to y0's successor once };
    (c)  hamk_poincare_steps over the same steps (section theta1 = pi mod 2 pi, upward, 4 rows): the cost of not stopping.
  Every launch starts from the same fresh state (cloned outside the clock).  Launches alternate between the variants; medians over
  --launches launches after --warmup.  Reported: the medians, (b) / (a), (c) / (a), (a') / (a), the fraction of lanes that exited
  and the mean fraction of the steps a wavefront ran (from texit: a wavefront runs until its last lane has stopped), in both lane
  orders.
  build  hamk_exit_build_info (bytes, spills, registers) for pendulum, doublePendulum, opcodeZoo, chain8, chain16.
Appends one JSON line per figure to profiles/exit_rate.jsonl.  Needs the GPU: there is no fall-back.
  python scripts/exit_rate.py [--launches 12] [--warmup 3] [--steps 10000] [--out profiles/exit_rate.jsonl]"""
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

PI = math.pi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--side", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10000)
    ap.add_argument("--outside-launches", type=int, default=None, help="launches of variant (b), which takes seconds each (default: --launches)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exit_rate.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU"
    torch.cuda.set_device(0)
    rows = []

    def emit(row):
        row["device"] = torch.cuda.get_device_name(0)
        rows.append(row)
        print(json.dumps(row), flush=True)

    spec = examples.get("doublePendulum")
    s = api.system_from_spec(spec)
    dt, G, K, n = 0.01, a.side, a.steps, spec.n
    B = G * G
    gates = [(0, -PI, PI), (1, -PI, PI)]
    axis = torch.linspace(-PI, PI, G + 2, dtype=torch.float64, device="cuda")[1:-1]
    q0 = torch.stack([axis.repeat_interleave(G), axis.repeat(G)]).contiguous()            # row-major: lane = G i1 + i2
    p0 = torch.zeros_like(q0)
    perm = torch.from_numpy(np.random.default_rng(1).permutation(B)).cuda()
    q0s = q0[:, perm].contiguous()

    def fresh_exits():
        return api.Exits(torch.full((B,), -1, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.float64, device="cuda"),
                         torch.zeros(n, B, dtype=torch.float64, device="cuda"), torch.zeros(n, B, dtype=torch.float64, device="cuda"))

    def fused(start):
        def prepare():
            return dict(y=api.Phase(start.clone(), p0.clone()), ex=fresh_exits())

        def launch(st):
            api.exitSteps(dt, K, s, st["y"], gates, exits=st["ex"], inplace=True)
            return st["ex"]
        return prepare, launch

    def outside_prepare():
        return dict(y=api.Phase(q0.clone(), p0.clone()), alive=torch.ones(B, dtype=torch.bool, device="cuda"),
                    t=torch.zeros(B, dtype=torch.float64, device="cuda"), code=torch.full((B,), -1, dtype=torch.int32, device="cuda"))

    pi_t = torch.tensor(PI, dtype=torch.float64, device="cuda")

    def outside_launch(st):
        y, alive = st["y"], st["alive"]
        for k in range(K):
            qa, pa = y.positions.clone(), y.momenta.clone()
            api.rk4Steps(dt, 1, s, y, inplace=True)
            q1 = y.positions
            above, below = q1 > PI, q1 < -PI
            fire = (above | below) & alive[None, :]
            tgt = torch.where(above, pi_t, -pi_t)
            th = torch.where(fire, (tgt - qa) / (q1 - qa), 2.0)
            best, g = th.min(0)
            out = fire.any(0)
            side = torch.gather(above, 0, g[None, :])[0].to(torch.int32)
            st["t"] = torch.where(out, float(k) + best, st["t"])
            st["code"] = torch.where(out, 2 * g.to(torch.int32) + side, st["code"])
            y.positions.copy_(torch.where(alive[None, :], q1, qa))                        # a stopped lane stays where its exit step ended
            y.momenta.copy_(torch.where(alive[None, :], y.momenta, pa))
            alive &= ~out
        return api.Exits(st["code"], st["t"], None, None)

    def psec_prepare():
        z = lambda *shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device="cuda")
        return dict(y=api.Phase(q0.clone(), p0.clone()), hits=api.Hits(z(4, n, B), z(4, n, B), z(4, B), z(B, dtype=torch.int32)))

    def psec_launch(st):
        api.poincareSteps(dt, K, s, st["y"], 0, PI, 2.0 * PI, 1, hits=st["hits"], inplace=True)
        return None

    A, AS = "(a) hamk_exit_steps, row-major grid", "(a') hamk_exit_steps, shuffled lane order"
    BB, C = "(b) outside: hamk_rk4_steps per step + torch gate test and linear interpolation", "(c) hamk_poincare_steps over the same steps (nothing stops)"
    variants = [(A, *fused(q0), a.launches), (AS, *fused(q0s), a.launches),
                (BB, outside_prepare, outside_launch, a.launches if a.outside_launches is None else a.outside_launches), (C, psec_prepare, psec_launch, a.launches)]
    times = {name: [] for name, *_ in variants}
    last = {}
    for r in range(a.warmup + a.launches):
        for name, prepare, launch, count in variants:       # alternating: every variant sees the same state of the machine
            if r >= a.warmup + count:
                continue
            st = prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = launch(st)
            torch.cuda.synchronize()
            if r >= a.warmup:
                times[name].append(time.perf_counter() - t0)
            if res is not None:
                last[name] = (res.code.cpu().numpy(), res.t.cpu().numpy())
            del st, res

    def waves(code, t):
        """(fraction of lanes exited, mean fraction of the steps a wavefront of 64 consecutive lanes ran)"""
        ran = np.where(code >= 0, np.floor(t) + 1.0, np.where(code == -2, t, float(K)))
        return float((code != -1).mean()), float(ran.reshape(-1, 64).max(1).mean() / K)

    med = {name: float(np.median(v)) for name, v in times.items()}
    for name, *_ in variants:
        row = {"figure": "rate", "system": spec.name, "B": B, "grid": f"{G} x {G} (theta1, theta2) in (-pi, pi)^2, p = 0", "steps_per_launch": K, "dt": dt,
               "gates": "theta1, theta2 in [-pi, pi]", "variant": name, "launches": len(times[name]), "median_launch_s": med[name],
               "min_launch_s": float(min(times[name])), "max_launch_s": float(max(times[name]))}
        if name in last:
            row["fraction_of_lanes_exited"], row["mean_fraction_of_steps_a_wavefront_ran"] = waves(*last[name])
        if name != A:
            row["time_over_a"] = med[name] / med[A]
        emit(row)
    ca, ta = last[A]
    cs, ts = last[AS]
    pm = perm.cpu().numpy()
    cb, tb = last[BB]
    both = (ca >= 0) & (cb >= 0)
    emit({"figure": "agreement", "shuffled_equals_row_major_bitwise": bool(np.array_equal(cs, ca[pm]) and np.array_equal(ts, ta[pm])),
          "outside_codes_equal_fused": float((ca == cb).mean()), "outside_largest_texit_difference_in_steps": float(np.abs(ta - tb)[both].max())})
    for name in ("pendulum", "doublePendulum", "opcodeZoo", "chain8", "chain16"):
        emit({"figure": "build", "system": name, "exit_build_info": api.system_from_spec(examples.get(name)).exit_build_info.strip()})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for row in rows:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
