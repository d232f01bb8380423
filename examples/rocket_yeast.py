#!/usr/bin/env python3
"""A droplet of cells that spreads on the surfactant it secretes (LB_D2Q9.rocket_yeast).

    python examples/rocket_yeast.py [--forces] [--Lx 6.4] [--Ly 6.4] [--N 10] [--steps 100] [--every 20] [--epsilon 1.0]

A Gaussian droplet of radius R0 = 1 with 5 % noise grows logistically and secretes surfactant; the surfactant's gradient drives a
Marangoni flow outwards (`Rocket_Yeast`), or, with --forces, a surface force and a pressure force do (`Rocket_Yeast_Forces_Only`).
Printed every few steps: the total population, the total surfactant, the colony's radius of gyration and the largest speed.  The
surfactant has no sink in this model, so a long run ends in a box full of it: the reference's fork is a sketch of the early spreading.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.rocket_yeast.rocket_yeast import Rocket_Yeast                          # noqa: E402
from LB_D2Q9.rocket_yeast.rocket_yeast_forces_only import Rocket_Yeast_Forces_Only  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forces", action="store_true")
    ap.add_argument("--Lx", type=float, default=6.4)
    ap.add_argument("--Ly", type=float, default=6.4)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--epsilon", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    cls = Rocket_Yeast_Forces_Only if a.forces else Rocket_Yeast
    sim = cls(Lx=a.Lx, Ly=a.Ly, R0=1., epsilon=a.epsilon, Dc=1., N=a.N, rng=a.seed, check_max_ulb=True)
    print("%s, %d x %d cells, omega %.3f / %.3f: %s" % (cls.__name__, sim.nx, sim.ny, sim.omega, sim.omega_c, sim.engine.hot_kernel().split(" (")[0]))
    r2 = sim.X ** 2 + sim.Y ** 2
    done = 0
    while done < a.steps:
        n = min(a.every, a.steps - done)
        sim.run(n)
        done += n
        rho = np.asarray(sim.rho, np.float64)
        speed = np.sqrt(np.asarray(sim.u, np.float64) ** 2 + np.asarray(sim.v, np.float64) ** 2)
        p = rho[:, :, 0]
        print("step %4d: population %.2f, surfactant %.2f, radius of gyration %.3f, max |u| %.4f"
              % (done, p.sum(), rho[:, :, 1].sum(), np.sqrt((p * r2).sum() / p.sum()), speed.max()))


if __name__ == "__main__":
    main()
