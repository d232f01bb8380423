#!/usr/bin/env python3
"""A colony that eats its way outwards (the reference's Surfactant_Nutrient_Wave and its clumpy variant, fused in HIP).

    python examples/surfactant_nutrient.py [--steps 2000] [--every 500] [--vc 0.5] [--lam 1.0] [--clumpy]

A noisy Gaussian droplet of radius R0 = 0.5 sits on a uniform nutrient.  The population grows by G rho_p rho_n, the nutrient loses
the same amount, both diffuse (D = 1/4, Dn = 0.1) and both are advected down the gradient of a screened potential of the population,
(1 - lam^2 laplace) phi = rho_p, u = -vc grad phi; --clumpy adds the Shan-Chen self-attraction of the population.  Every `every` steps
the total population, the total nutrient, their sum -- which the collision conserves up to rounding -- and the largest speed in
lattice units are printed.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.reaction_diffusion.surfactant_nutrient_waves import Clumpy_Surfactant_Nutrient_Wave, Surfactant_Nutrient_Wave      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=500)
    ap.add_argument("--vc", type=float, default=0.5)
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--clumpy", action="store_true")
    a = ap.parse_args()
    kw = dict(Lx=12.8, Ly=9.6, vc=a.vc, lam=a.lam, Dn=0.1, R0=0.5, N=20, rng=1)        # 256 x 192 cells: 2^8, 2^6 x 3
    sim = Clumpy_Surfactant_Nutrient_Wave(rho_o=1., G_chen=-1., **kw) if a.clumpy else Surfactant_Nutrient_Wave(**kw)
    print("grid %d x %d, omega %s, omega_n %s, G %s, u = %s Re grad phi" % (sim.nx, sim.ny, sim.omega, sim.omega_n, sim.lb_G, sim.velocity_scale))
    done = 0
    while done < a.steps:
        n = min(a.every, a.steps - done)
        sim.run(n)
        done += n
        g = sim.get_fields()
        pop, nut = g["rho"][:, :, 0].astype(np.float64).sum(), g["rho"][:, :, 1].astype(np.float64).sum()
        speed = float(np.sqrt(g["u"].astype(np.float64) ** 2 + g["v"].astype(np.float64) ** 2).max())
        print("step %5d  t = %.3f T  population %.3f  nutrient %.3f  sum %.3f  max |u| %.4f" % (done, done * sim.delta_t, pop, nut, pop + nut, speed))


if __name__ == "__main__":
    main()
