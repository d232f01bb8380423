#!/usr/bin/env python3
"""A Fisher wave with demographic noise (the reference's Noisy_Advected_Fisher_Wave, fused in HIP).

    python examples/noisy_fisher_wave.py [--steps 2000] [--every 500] [--Nc 100] [--seed 0]

A Gaussian droplet grows logistically, diffuses and is carried by a uniform flow; every cell adds sqrt(Dg rho (1 - rho)) z per step, z a
standard normal drawn inside the kernel from a counter-based stream (Philox4x32-10 under --seed): no buffer of random numbers, no launch
to refill one.  Nc is the number of individuals per deme: the smaller, the rougher the front.  Every `every` steps the total mass, the
extreme densities, the noise counter and the number of cells that left [0, 1] (NaN from then on, as in the reference) are printed.
Two runs with the same seed print the same lines.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.reaction_diffusion.noisy_fisher_wave import Noisy_Advected_Fisher_Wave      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=500)
    ap.add_argument("--Nc", type=float, default=100.)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    sim = Noisy_Advected_Fisher_Wave(Lx=2.0, Ly=2.0, D=1.0, z=0.1, vx=0.5, vy=0., vc=1.0, g=10., Nc=a.Nc, N=10, seed=a.seed)
    print("grid %d x %d, omega %s, G %s, Dg %s" % (sim.nx, sim.ny, sim.omega, sim.lb_Gd, sim.lb_Dg))
    done = 0
    while done < a.steps:
        n = min(a.every, a.steps - done)
        sim.run(n)
        done += n
        rho = sim.get_fields()["rho"]
        bad = sim.sim.check()["n_nonfinite"]
        print("step %5d  mass %.6e  rho in [%.4f, %.4f]  noise counter %d  cells outside [0, 1]: %d"
              % (done, float(np.nansum(rho.astype(np.float64))), float(np.nanmin(rho)), float(np.nanmax(rho)), sim.sim.noise()[2], bad))


if __name__ == "__main__":
    main()
