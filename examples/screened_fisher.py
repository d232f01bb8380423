#!/usr/bin/env python3
"""A colony that pushes itself apart (the reference's Screened_Fisher_Wave, fused in HIP).

    python examples/screened_fisher.py [--steps 2000] [--every 500] [--vc 1.0] [--lam 1.0]

A Gaussian droplet of radius R0 = 0.5 grows logistically and diffuses (D = 1/4, G = 1: a Fisher wave of speed 1) while it advects
itself down the gradient of a screened potential, (1 - lam^2 laplace) phi = rho, u = -vc grad phi: every step solves that equation by
FFT in the periodic box and steps the lattice with the result.  Every `every` steps the radius at which the density along the x axis
falls below one half, the total mass and the largest Mach number are printed.  With vc = 0 the front is the plain Fisher wave.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.reaction_diffusion.screened_poisson_waves import Screened_Fisher_Wave      # noqa: E402


def half_radius(rho, sim):
    row = rho[sim.x_center:, sim.y_center]
    below = np.nonzero(row < 0.5)[0]
    return (below.min() if len(below) else len(row)) / float(sim.N)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=500)
    ap.add_argument("--vc", type=float, default=1.0)
    ap.add_argument("--lam", type=float, default=1.0)
    a = ap.parse_args()
    sim = Screened_Fisher_Wave(Lx=12.8, Ly=9.6, vc=a.vc, lam=a.lam, R0=0.5, N=20)       # 256 x 192 cells: 2^8, 2^6 x 3
    print("grid %d x %d, omega %s, G %s, u = %s Re grad phi" % (sim.nx, sim.ny, sim.omega, sim.lb_G, sim.velocity_scale))
    done = 0
    while done < a.steps:
        n = min(a.every, a.steps - done)
        sim.run(n)
        done += n
        rho = sim.get_fields()["rho"]
        print("step %5d  t = %.3f T  half-density radius %.2f L  total mass %.1f  max Mach %.3f"
              % (done, done * sim.delta_t, half_radius(rho, sim), rho.sum(), sim.sim.check()["max_mach"]))


if __name__ == "__main__":
    main()
