#!/usr/bin/env python3
"""Throughput of the LB Poisson solver: the fused iteration, lb_solve at several batch lengths, the literal port, k_ad_step, the copy rate.

    python tools/poisson_bench.py [--sizes 256,512,1024,2048,4096] [--rounds 3] > profiles/poisson_bench.txt

For every box size n x n, on handles created once and measured `rounds` times IN ALTERNATION (best of the rounds; every sample is
host wall-clock time around work that ends in a device synchronise, so that lb_solve's own read-backs are inside it):
  run       lb_run(steps): k_ps_step<false>, one launch per iteration, no check
  solve/B   lb_solve(steps) with tolerance 0 (it never stops) and B launches between two reads of the stop word: k_ps_step<true> +
            k_ps_check per iteration.  B is fixed when a handle is created (its diagnostic word), so each B has a handle of its own,
            in the same state as the others
  phases    the literal port: lb_move, lb_move_bcs, lb_update_hydro, lb_update_feq, lb_collide_particles with a host wait after each,
            as the reference waits after each of its kernels -- and NO convergence check at all: a lower bound of the reference's cost
  phases+check   ... plus a host-side check every iteration: rho downloaded and the ratio formed in numpy (the reference reduces on
            the device and reads two scalars back: cheaper than this at large sizes, not cheaper than `phases`)
  k_ad_step lb_run(steps) on a scalar-lattice handle (LB_SEM_DIFFUSION, LB_BC_OPEN, single-step kernel forced) of the same size
  copy      lb_copy_calibration on the Poisson handle
Printed per size: microseconds per iteration and MLUPS of each, the fused iteration's compulsory traffic (72 B of populations + 4 B
of source [+ 8 B of rho read and written + the partials, in lb_solve's form]) against the copy rate, the byte ratio against k_ad_step
(80 B), and lb_solve / literal port.
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


def poisson_handle(n, f0, src, batch=None):
    old = os.environ.pop("LB_DIAG", None)
    if batch:
        os.environ["LB_DIAG"] = str(batch)
    try:
        s = Simulation(n, n, 0.5, bc="dirichlet", semantics="poisson")
    finally:
        os.environ.pop("LB_DIAG", None)
        if old is not None:
            os.environ["LB_DIAG"] = old
    s.set_poisson(0.1, 0.25, 0.)
    s.set_source(src)
    s.set_f(f0)
    return s


def wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def case(n, rounds, batches):
    rng = np.random.default_rng(n)
    f0 = np.asfortranarray((W * 0.3 * (1. + 0.05 * rng.uniform(-1, 1, (n, n, 9)))).astype(np.float32))
    src = np.asfortranarray((1e-4 * rng.uniform(size=(n, n))).astype(np.float32))
    steps = int(max(20, min(2000, 2.0e8 / (float(n) * n))))
    lit_steps = max(10, steps // 4)
    main = poisson_handle(n, f0, src)
    solvers = {b: poisson_handle(n, f0, src, b) for b in batches}
    ad = Simulation(n, n, 0.9, bc="open", semantics="diffusion")
    ad.set_f(f0)
    ad.set_variant(K_STEP)

    def run():
        main.run(steps)

    def phases(check):
        def go():
            for _ in range(lit_steps):
                before = main.get_fields(("rho",))["rho"] if check else None
                main.move(); main.move_bcs(); main.update_hydro(); main.update_feq(); main.collide_particles()
                if check:
                    rho = main.get_fields(("rho",))["rho"]
                    float(np.abs(before - rho).mean() / before.mean())
        return go

    samples = {"run": (run, steps), "phases": (phases(False), lit_steps), "phases+check": (phases(True), lit_steps),
               "k_ad_step": (lambda: ad.run(steps), steps)}
    for b, s in solvers.items():
        samples["solve/%d" % b] = ((lambda s=s: s.solve(steps)), steps)
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
    print("n=%5d  %d iterations per sample (%d for the literal port)" % (n, steps, lit_steps))
    for k in samples:
        print("    %-13s %9.2f us / iteration  %9.0f MLUPS" % (k, us[k], mlups[k]))
    gb_run, gb_ad = 76. * cells / us["run"] / 1e3, 80. * cells / us["k_ad_step"] / 1e3
    chosen = "solve/%d" % batches[len(batches) // 2]
    gb_solve = 88. * cells / us[chosen] / 1e3
    print("    copy %.0f GB/s; k_ps_step<false> %.0f GB/s at 76 B (%.2f of copy); %s %.0f GB/s at 88 B (%.2f of copy); k_ad_step %.0f GB/s at 80 B "
          "(%.2f of copy)" % (copy, gb_run, gb_run / copy, chosen, gb_solve, gb_solve / copy, gb_ad, gb_ad / copy))
    print("    %s against k_ad_step: %.2f of its rate (byte ratio 80 / 88 = %.2f); against the literal port: %.1f x `phases`, %.1f x `phases+check`"
          % (chosen, mlups[chosen] / mlups["k_ad_step"], 80. / 88., mlups[chosen] / mlups["phases"], mlups[chosen] / mlups["phases+check"]), flush=True)
    for s in [main, ad] + list(solvers.values()):
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="1,16,32,64,256")
    a = ap.parse_args()
    batches = [int(k) for k in a.batches.split(",")]
    print("# LB Poisson solver: microseconds per iteration, best of %d rounds alternating the samples on handles of one size; wall clock around "
          "synchronised work; lb_solve with tolerance 0 (never stops); the middle batch length of %s is the library's" % (a.rounds, batches))
    for n in [int(k) for k in a.sizes.split(",")]:
        case(n, a.rounds, batches)


if __name__ == "__main__":
    main()
