#!/usr/bin/env python3
"""Cost of a step of a population and its nutrient under the spectral velocity: fused, un-fused, and beside its nearest neighbour.

    python tools/nutrient_bench.py [--sizes 256,512,1024,2048,4096] [--rounds 3] > profiles/nutrient_bench.txt

For every box n x n, on objects created once and measured `rounds` times IN ALTERNATION (best of the rounds; every sample is host
wall-clock time around work that ends in a device synchronise):
  (a) plain, fused    lb_run_nutrient(steps), clumpy = 0: k_ad_moments (36 + 4 B per cell), the three launches of the solve (84 B),
                      k_sn_step<false> (144 B gathered and stored + 8 B of u, v): 276 B
  (a) clumpy, fused   the same with clumpy = 1: k_sn_step<true> also reads rho_p of its rows and their halo, (4 + 2) / 4 x 4 B: 282 B
  (b) phases          the un-fused sequence of the plain variant -- lb_move and lb_update_hydro on both members, lb_nutrient_velocity,
                      lb_update_feq on both, lb_collide_nutrient -- with a host wait after each, as the reference waits after each of
                      its launches
  (c) screened        lb_run_screened(steps) on ONE scalar lattice of the same size (periodic, no growth): k_ad_moments, the solve,
                      k_ad_step: 204 B -- the nearest neighbour that existed before this set
  solve               lb_spectral_velocity(sp, s, scale, 0) alone, a call of its own with its event hand-over between two streams: the
                      share of (a) that is the solve (above 100 % where that hand-over costs more than the launches it brackets)
  k_ad_step           lb_run(steps) with lb_set_variant(0) on one scalar lattice of the same size with an imposed velocity (80 B): what one
                      more lattice's traffic costs on its own -- by bytes alone, (a) - (c)
Printed per size: microseconds per step, the ratios (a) / (c) and (b) / (a), the solve's share of (a), GB/s at the bytes above, and
(a) - (c) beside k_ad_step's time.
"""
import argparse
import os
import sys
import time

import torch            # first: one HIP runtime in the process, torch's; the library binds to it
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9 import _native                     # noqa: E402
from LB_D2Q9.nutrient_set import Nutrient_Set   # noqa: E402
from LB_D2Q9.simulation import Simulation       # noqa: E402

OMEGA, OMEGA_N, G = 0.8, 1.25, 0.01


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def droplet(n):
    x = (np.arange(n, dtype=np.float64) - n // 2) / (n / 3.)
    return np.asfortranarray(1.2 * np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / 0.25).astype(np.float32))


def nutrient_set(n, rho_p, scale, clumpy):
    s = Nutrient_Set(n, n, OMEGA, OMEGA_N, lam=1., dx=1. / n)
    s.set_params(G=G, scale=scale, clumpy=clumpy, rho_o=1., G_chen=-1.)
    zero = np.zeros((n, n), np.float32)
    s.set_fields(np.stack([rho_p, np.ones_like(rho_p)], axis=2), zero, zero)
    s.update_velocity()
    s.update_forces()
    s.update_feq()
    s.init_pop()
    return s


def case(n, rounds):
    L = _native.lib()
    rho = droplet(n)
    scale = -3.0 / n                        # (a lattice velocity of a few 1e-3: the state stays smooth and finite)
    reps = int(max(3, min(200, 4.0e7 / (float(n) * n))))
    plain, clumpy, lit = nutrient_set(n, rho, scale, False), nutrient_set(n, rho, scale, True), nutrient_set(n, rho, scale, False)
    one = Simulation(n, n, OMEGA, bc="periodic", semantics="diffusion")
    zero = np.zeros((n, n), np.float32)
    one.set_fields(rho, zero, zero)
    sp = plain.solver._h
    _native.check(L.lb_spectral_velocity(sp, one._h, scale, 0))
    one.update_feq()
    one.init_pop()
    alone = Simulation(n, n, OMEGA, bc="periodic", semantics="diffusion")
    alone.set_variant(0)
    g = one.get_fields(("u", "v"))
    alone.set_fields(rho, g["u"], g["v"])
    alone.update_feq()
    alone.init_pop()

    def phases():
        for _ in range(reps):
            lit.step_phases()

    def solve():
        for _ in range(reps):
            _native.check(L.lb_spectral_velocity(sp, one._h, scale, 0))

    samples = {"(a) plain, fused": lambda: plain.run(reps, wait=False), "(a) clumpy, fused": lambda: clumpy.run(reps, wait=False),
               "(b) phases": phases, "(c) screened": lambda: _native.check(L.lb_run_screened(sp, one._h, scale, reps)), "solve": solve,
               "k_ad_step": lambda: alone.run(reps, wait=False)}
    for fn in samples.values():
        fn()                                # warm-up
    best = {k: None for k in samples}
    for _ in range(rounds):
        for k, fn in samples.items():
            t = wall(fn)
            best[k] = t if best[k] is None else min(best[k], t)
    ok = all(c["n_nonfinite"] == 0 for s in (plain, clumpy, lit) for c in s.check()) and one.check()["n_nonfinite"] == 0 and alone.check()["n_nonfinite"] == 0
    cells = float(n) * n
    us = {k: best[k] / reps * 1e6 for k in samples}
    gb = {"(a) plain, fused": 276., "(a) clumpy, fused": 282., "(c) screened": 204., "solve": 84., "k_ad_step": 80.}
    print("n=%5d  %d steps per sample; finite: %s" % (n, reps, ok))
    for k in samples:
        extra = "  %7.0f GB/s at %.0f B per cell" % (gb[k] * cells / us[k] / 1e3, gb[k]) if k in gb else ""
        print("    %-18s %10.2f us%s" % (k, us[k], extra))
    a, c = us["(a) plain, fused"], us["(c) screened"]
    print("    (a) / (c) = %.2f plain, %.2f clumpy; (b) / (a) = %.2f; the solve is %.0f %% of (a); (a) - (c) = %.2f us, k_ad_step alone "
          "%.2f us" % (a / c, us["(a) clumpy, fused"] / c, us["(b) phases"] / a, 100. * us["solve"] / a, a - c, us["k_ad_step"]), flush=True)
    for s in (plain, clumpy, lit, one, alone):
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("nutrient_bench needs a GPU: nothing is measured without one")
    print("# a population and its nutrient under the spectral velocity: microseconds per step, best of %d rounds alternating the samples; "
          "wall clock around synchronised work" % a.rounds)
    for n in [int(k) for k in a.sizes.split(",")]:
        case(n, a.rounds)


if __name__ == "__main__":
    main()
