#!/usr/bin/env python3
"""Throughput of forced flow in a porous medium: the fused step, the literal port, k_ad_step, the copy rate.

    python tools/porous_bench.py [--sizes 256,512,1024,2048,4096,8192] [--rounds 3] > profiles/porous_bench.txt

For every box size n x n, on handles created once and measured `rounds` times IN ALTERNATION (best of the rounds; every sample is
host wall-clock time around work that ends in a device synchronise):
  run         lb_run(steps) on a zero-gradient handle: k_pm_step, one launch per step, 72 B per cell (+ 28 B on the last launch)
  run+field   the same with a force field: 80 B per cell
  periodic    lb_run(steps) on a periodic handle of the same size
  phases      the literal port on the zero-gradient handle: lb_move, lb_move_bcs, lb_update_hydro, lb_update_forces,
              lb_update_bary_velocity, lb_update_feq, lb_collide_particles with a host wait after each, as the reference waits after
              each of its eleven kernels (its Gx, Gy = 0 and its additional forces are inside lb_update_forces here): a lower bound
              of the reference's cost
  k_ad_step   lb_run(steps) on a scalar-lattice handle (LB_SEM_DIFFUSION, LB_BC_OPEN, single-step kernel forced) of the same size
  copy        lb_copy_calibration on the porous handle
Printed per size: microseconds per step and MLUPS of each, the fused step's compulsory traffic against the copy rate, the same
for k_ad_step (80 B), and the fused step against the literal port.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.simulation import Simulation      # noqa: E402
from LB_D2Q9.variants import K_STEP            # noqa: E402

W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4, dtype=np.float32)


def porous_handle(n, f0, bc):
    s = Simulation(n, n, 1.25, bc=bc, semantics="porous")
    s.set_porous(0.7, 0.15, 20., 0.3)
    s.set_body_force(2e-4, -1e-4)
    s.set_f(f0)
    return s


def wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def case(n, rounds):
    rng = np.random.default_rng(n)
    f0 = np.empty((n, n, 9), np.float32, order="F")
    for k in range(9):
        f0[:, :, k] = W[k] * (1. + 0.05 * rng.uniform(-1, 1, (n, n)).astype(np.float32))
    steps = int(max(20, min(2000, 2.0e8 / (float(n) * n))))
    lit_steps = max(5, steps // 4)
    main, per, fld = porous_handle(n, f0, "zero_gradient"), porous_handle(n, f0, "periodic"), porous_handle(n, f0, "zero_gradient")
    field = np.asfortranarray((1e-4 * rng.uniform(-1, 1, (n, n))).astype(np.float32))
    fld.set_force_field(field, field)
    ad = Simulation(n, n, 0.9, bc="open", semantics="diffusion")
    ad.set_f(f0)
    ad.set_variant(K_STEP)
    del f0

    def phases():
        for _ in range(lit_steps):
            main.move(); main.move_bcs(); main.update_hydro(); main.update_forces(); main.update_bary_velocity()
            main.update_feq(); main.collide_particles()

    samples = {"run": (lambda: main.run(steps), steps), "run+field": (lambda: fld.run(steps), steps),
               "periodic": (lambda: per.run(steps), steps), "phases": (phases, lit_steps), "k_ad_step": (lambda: ad.run(steps), steps)}
    for fn, _ in samples.values():
        fn()                                    # warm-up
    best, copy = {k: None for k in samples}, 0.
    for _ in range(rounds):
        for k, (fn, _) in samples.items():
            t = wall(fn)
            best[k] = t if best[k] is None else min(best[k], t)
        copy = max(copy, main.copy_calibration(iters=10)[0])
    cells = float(n) * n
    us = {k: best[k] / samples[k][1] * 1e6 for k in samples}
    mlups = {k: cells / us[k] for k in samples}
    print("n=%5d  %d steps per sample (%d for the literal port); %s" % (n, steps, lit_steps, main.hot_kernel().split(" (")[0]))
    for k in samples:
        print("    %-10s %9.2f us / step  %9.0f MLUPS" % (k, us[k], mlups[k]))
    gb = {"run": 72., "run+field": 80., "periodic": 72., "k_ad_step": 80.}
    rate = {k: b * cells / us[k] / 1e3 for k, b in gb.items()}
    print("    copy %.0f GB/s; %s" % (copy, "; ".join("%s %.0f GB/s at %d B (%.2f of copy)" % (k, rate[k], gb[k], rate[k] / copy) for k in gb)))
    print("    k_pm_step against k_ad_step: %.2f of its rate in cells (byte ratio 80 / 72 = %.2f); against the literal port: %.1f x"
          % (mlups["run"] / mlups["k_ad_step"], 80. / 72., mlups["run"] / mlups["phases"]), flush=True)
    for s in (main, per, fld, ad):
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    print("# forced flow in a porous medium: microseconds per step, best of %d rounds alternating the samples on handles of one size; wall "
          "clock around synchronised work" % a.rounds)
    for n in [int(k) for k in a.sizes.split(",")]:
        case(n, a.rounds)


if __name__ == "__main__":
    main()
