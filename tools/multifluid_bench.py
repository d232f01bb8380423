#!/usr/bin/env python3
"""Throughput of multicomponent Shan-Chen fluids: the one-launch step, the two-launch step, the literal port, k_pm_step, the copy rate.

    python tools/multifluid_bench.py [--sizes 256,512,1024,2048,4096,8192] [--fluids 1,2,3] [--rounds 3] > profiles/multifluid_bench.txt

For every box size n x n and number of fluids NF, on handles created once and measured `rounds` times IN ALTERNATION (best of the
rounds; every sample is host wall-clock time around work that ends in a device synchronise):
  run         lb_run_fluids(steps) on a periodic set with an interaction table (NF = 1: a shan_chen self term; NF = 2: a linear
              pair; NF = 3: three pairs): k_mc_moments + k_mc_collide, two launches per step.  Compulsory traffic per fluid and
              cell: 36 B read + 4 B written (moments), 36 B + 4 B read and 36 B written (collide) = 116 B
  fused       the same set with lb_set_variant(1): k_mc_step, one launch per step; a workgroup owns R = 6 rows (NF = 3: 2) and reads
              R + 2: 36 (R + 2) / R B read + 36 B written per fluid and cell = 84 B (NF = 3: 108 B)
  run, none   the two-launch step on the same set without a table
  phases      the literal port on the set with the table: move, move_bcs, update_hydro per fluid, update_forces,
              update_bary_velocity, update_feq and collide_particles per fluid, with a host wait after each, as the reference waits
              after each of its kernels (its Gx, Gy = 0 and its additional forces are one kernel here): a lower bound of the
              reference's cost
  k_pm_step   lb_run(steps) on NF porous handles of the same size one after the other (72 B per cell): what the same lattices
              cost without the coupling
  copy        lb_copy_calibration on a member of the set
Printed per case: microseconds per step and MLUPS in FLUID-cell updates (cells x NF per step), the step's compulsory traffic
against the copy rate, the step against the literal port and against k_pm_step.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.coupled import Shan_Chen_Fluids    # noqa: E402
from LB_D2Q9.simulation import Simulation      # noqa: E402

OMEGAS = (1.25, 0.9, 1.05)
TABLES = {1: [(0, 0, -1.5, "shan_chen", 1.)], 2: [(0, 1, 1., "linear", 0.)],
          3: [(0, 1, 1., "linear", 0.), (0, 2, 0.7, "linear", 0.), (1, 2, 0.5, "shan_chen", 1.)]}
BYTES = 116.


def wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def fluids(n, nf, rho, table):
    s = Shan_Chen_Fluids(n, n, OMEGAS[:nf], bc="periodic")
    zero = np.zeros((n, n), np.float32)
    s.set_bary_velocity(zero, zero)
    for i, m in enumerate(s.members):
        m.set_fields((0.7 + 0.1 * i) * rho, zero, zero)
        m.update_feq()
        m.init_pop(None)
    s.set_interactions(table)
    return s


def case(n, nf, rounds):
    x = np.arange(n, dtype=np.float32)
    rho = np.asfortranarray(1. + 0.02 * np.sin(2. * np.pi * x / n)[:, None] * np.cos(2. * np.pi * x / n)[None, :])
    steps = int(max(20, min(1000, 1.0e8 / (float(n) * n * nf))))
    lit_steps = max(3, steps // 8)
    main, bare, one = fluids(n, nf, rho, TABLES[nf]), fluids(n, nf, rho, []), fluids(n, nf, rho, TABLES[nf])
    main.set_variant(0)
    bare.set_variant(0)
    one.set_variant(1)
    pm = []
    for i in range(nf):
        p = Simulation(n, n, OMEGAS[i], bc="periodic", semantics="porous")
        p.set_porous(1., 0., 1., 0.)
        p.set_fields(rho, np.zeros_like(rho), np.zeros_like(rho))
        p.set_bary_velocity(np.zeros_like(rho), np.zeros_like(rho))
        p.update_feq()
        p.init_pop(None)
        pm.append(p)

    def phases():
        for _ in range(lit_steps):
            main.step_phases()

    def porous():
        for p in pm:
            p.run(steps, wait=False)
        for p in pm:
            p.sync()

    samples = {"run": (lambda: main.run(steps), steps), "fused": (lambda: one.run(steps), steps), "run, none": (lambda: bare.run(steps), steps), "phases": (phases, lit_steps),
               "k_pm_step": (porous, steps)}
    for fn, _ in samples.values():
        fn()                                    # warm-up
    best, copy = {k: None for k in samples}, 0.
    for _ in range(rounds):
        for k, (fn, _) in samples.items():
            t = wall(fn)
            best[k] = t if best[k] is None else min(best[k], t)
        copy = max(copy, main.members[0].copy_calibration(iters=10)[0])
    cells = float(n) * n * nf
    us = {k: best[k] / samples[k][1] * 1e6 for k in samples}
    mlups = {k: cells / us[k] for k in samples}
    print("n=%5d NF=%d  %d steps per sample (%d for the literal port); %s" % (n, nf, steps, lit_steps, main.hot_kernel().split(" (")[0]))
    for k in samples:
        print("    %-10s %9.2f us / step  %9.0f MLUPS" % (k, us[k], mlups[k]))
    gb = {"run": BYTES, "fused": 108. if nf == 3 else 84., "run, none": BYTES}
    rate = {k: b * cells / us[k] / 1e3 for k, b in gb.items()}
    print("    copy %.0f GB/s; %s" % (copy, "; ".join("%s %.0f GB/s at %d B (%.2f of copy)" % (k, rate[k], gb[k], rate[k] / copy) for k in rate)))
    print("    the one-launch step against the two-launch step: %.2f x" % (mlups["fused"] / mlups["run"]))
    print("    the step against the literal port: %.1f x; against k_pm_step on the same lattices: %.2f of its rate (byte ratio 72 / 116 = %.2f)"
          % (mlups["run"] / mlups["phases"], mlups["run"] / mlups["k_pm_step"], 72. / BYTES), flush=True)
    for s in [main, bare, one] + pm:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--fluids", default="1,2,3")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    print("# multicomponent Shan-Chen fluids: microseconds per step, best of %d rounds alternating the samples on handles of one size; wall "
          "clock around synchronised work; MLUPS counts fluid-cell updates" % a.rounds)
    for n in [int(k) for k in a.sizes.split(",")]:
        for nf in [int(k) for k in a.fluids.split(",")]:
            case(n, nf, a.rounds)


if __name__ == "__main__":
    main()
