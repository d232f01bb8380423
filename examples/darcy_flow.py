#!/usr/bin/env python3
"""A uniform fluid driven by gravity through a porous medium (LB_D2Q9.porous_media.single_component), against the analytic steady
states.

    python examples/darcy_flow.py [--nx 64] [--ny 32] [--steps 2000] [--bc periodic]

With the linear drag alone (Fe = 0) the fluid settles at the Darcy velocity u = g K / nu_fluid; with the quadratic drag as well at
the positive root of (Fe / sqrt(K)) u^2 + (nu_fluid / K) u - g = 0 (Forchheimer).  Printed for both: the steady barycentric velocity
the lattice reaches, the analytic value, and the relative difference (float32 lattice: a few 1e-5).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.porous_media import Pourous_Media, Simulation_Runner      # noqa: E402


def steady_velocity(nx, ny, steps, bc, g, K, nu_fluid, Fe, epsilon=0.6, nu_e=0.1):
    sim = Simulation_Runner(nx=nx, ny=ny)
    fluid = Pourous_Media(sim, 0, nu_e=nu_e, epsilon=epsilon, nu_fluid=nu_fluid, K=K, Fe=Fe, bc=bc)
    sim.add_fluid(fluid)
    sim.complete_setup()
    sim.add_constant_body_force(0, g, 0.)
    fluid.initialize(np.ones((nx, ny)), f_amp=0.)             # rho = 1 at rest
    sim.run(steps)
    return float(np.asarray(sim.u_bary, np.float64).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=64)
    ap.add_argument("--ny", type=int, default=32)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--bc", default="periodic", choices=("periodic", "zero_gradient"))
    a = ap.parse_args()
    g, K, nu = 1e-3, 2., 0.2
    for Fe in (0., 0.5):
        got = steady_velocity(a.nx, a.ny, a.steps, a.bc, g, K, nu, Fe)
        p, q = Fe / np.sqrt(K), nu / K
        want = g / q if Fe == 0 else (-q + np.sqrt(q * q + 4. * p * g)) / (2. * p)
        print("%-12s Fe = %.2f: u_b = %.8e, analytic %.8e (%s), relative difference %.2e"
              % (a.bc, Fe, got, want, "g K / nu" if Fe == 0 else "Forchheimer root", abs(got / want - 1.)))


if __name__ == "__main__":
    main()
