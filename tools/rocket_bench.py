#!/usr/bin/env python3
"""Throughput of surfactant-propelled colonies: the one-launch step, the two-launch step, the literal port, k_mc_step, the copy rate.

    python tools/rocket_bench.py [--sizes 256,512,1024,2048,4096,8192] [--modes flow,forces] [--rounds 3] > profiles/rocket_bench.txt

For every box size n x n and mode, on handles created once and measured `rounds` times IN ALTERNATION (best of the rounds; every
sample is host wall-clock time around work that ends in a device synchronise):
  one launch   lb_run_rocket(steps) with lb_set_variant(1): k_ry_step; a workgroup owns R rows of a 256-cell tile and reads R + 2:
               72 (R + 2) / R B read + 72 B written per cell (both lattices)
  two launches the same colony with lb_set_variant(0): k_ry_moments + k_ry_collide: 72 B read + 8 B written, then 72 B + 8 B read
               and 72 B written = 232 B per cell
  phases       the literal port: move, update_hydro, update_velocity, update_forces, update_feq and collide_particles with a host
               wait after each, as the reference waits after each of its kernels: a lower bound of the reference's cost
  k_mc_step    lb_run_fluids(steps) on two Shan-Chen fluids of the same size with an empty interaction table, one launch per step: it
               moves the same bytes per cell (two lattices, six rows a workgroup: 72 x 8 / 6 + 72 B) -- the yardstick
  copy         lb_copy_calibration on a member
Printed per case: microseconds per step and MLUPS in CELL updates (a cell = both lattices), the step's compulsory traffic against
the copy rate, the one-launch step against the two-launch step, the literal port and k_mc_step.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9 import _native                                     # noqa: E402
from LB_D2Q9.coupled import Shan_Chen_Fluids, Surfactant_Colony  # noqa: E402

PARAMS = dict(G=0.01, G_c=0.002, epsilon=0.5, rho_o=1., G_chen=-0.5, c_o=0.25, alpha=2.)


def wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def start(n):
    """a smooth state near a fixed point of neither lattice: nothing blows up within the timed steps, nothing is trivially zero"""
    x = np.arange(n, dtype=np.float32)
    wave = np.float32(0.02) * np.sin(2. * np.pi * x / n)[:, None] * np.cos(2. * np.pi * x / n)[None, :]
    return np.asfortranarray(np.stack([0.9 + wave, 0.3 - wave], axis=2).astype(np.float32))


def reset(s, rho):
    """f = feq(rho, u = 0) on the device (no upload of populations: 4.8 GB a colony at 8192^2)"""
    zero = np.zeros(rho.shape[:2], np.float32)
    if isinstance(s, Shan_Chen_Fluids):
        s.set_bary_velocity(zero, zero)
        s.set_fields(rho)
    else:
        s.set_fields(rho, zero, zero)
    s.update_feq()
    s.init_pop(None)


def colony(n, mode, variant):
    s = Surfactant_Colony(n, n, 0.8, 0.8, mode=mode)
    s.set_params(**PARAMS)
    s.set_variant(variant)
    return s


def case(n, mode, rounds):
    rho = start(n)
    steps = int(max(20, min(1000, 5.0e7 / (float(n) * n))))
    lit_steps = max(3, steps // 8)
    one, two, lit = colony(n, mode, 1), colony(n, mode, 0), colony(n, mode, -1)
    mc = Shan_Chen_Fluids(n, n, (0.8, 0.8), bc="periodic")
    mc.set_variant(1)

    def phases():
        for _ in range(lit_steps):
            lit.step_phases()

    def restart():
        # (the surfactant has no sink: every round starts from the same state)
        for s in (one, two, lit, mc):
            reset(s, rho)

    samples = {"one launch": (lambda: one.run(steps), steps), "two launches": (lambda: two.run(steps), steps), "phases": (phases, lit_steps),
               "k_mc_step": (lambda: mc.run(steps), steps)}
    restart()
    for fn, _ in samples.values():
        fn()                                    # warm-up
    best, copy = {k: None for k in samples}, 0.
    for _ in range(rounds):
        restart()
        for k, (fn, _) in samples.items():
            t = wall(fn)
            best[k] = t if best[k] is None else min(best[k], t)
        copy = max(copy, one.members[0].copy_calibration(iters=10)[0])
    ok = all(c["n_nonfinite"] == 0 for s in (one, two) for c in s.check())
    cells = float(n) * n
    us = {k: best[k] / samples[k][1] * 1e6 for k in samples}
    mlups = {k: cells / us[k] for k in samples}
    R = _native.RY_ROWS
    gb = {"one launch": 72. * (R + 2) / R + 72., "two launches": 232., "k_mc_step": 72. * 8 / 6 + 72.}
    rate = {k: b * cells / us[k] / 1e3 for k, b in gb.items()}
    print("n=%5d mode=%-6s  %d steps per sample (%d for the literal port); finite: %s; %s" % (n, mode, steps, lit_steps, ok, one.hot_kernel().split(" (")[0]))
    for k in samples:
        print("    %-12s %9.2f us / step  %9.0f MLUPS" % (k, us[k], mlups[k]))
    print("    copy %.0f GB/s; %s" % (copy, "; ".join("%s %.0f GB/s at %.0f B (%.2f of copy)" % (k, rate[k], gb[k], rate[k] / copy) for k in rate)))
    print("    the one-launch step against the two-launch step: %.2f x; against the literal port: %.1f x; against k_mc_step: %.2f of its rate"
          % (mlups["one launch"] / mlups["two launches"], mlups["one launch"] / mlups["phases"], mlups["one launch"] / mlups["k_mc_step"]), flush=True)
    for s in (one, two, lit, mc):
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--modes", default="flow,forces")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("rocket_bench needs a GPU: nothing is measured without one")
    print("# surfactant-propelled colonies: microseconds per step, best of %d rounds alternating the samples on handles of one size; wall "
          "clock around synchronised work; MLUPS counts cell updates (both lattices of a cell); k_ry_step owns %d rows a workgroup" % (a.rounds, _native.RY_ROWS))
    for n in [int(k) for k in a.sizes.split(",")]:
        for mode in a.modes.split(","):
            case(n, mode, a.rounds)


if __name__ == "__main__":
    main()
