#!/usr/bin/env python3
"""Two fluids that repel each other separate from a noisy mixture (LB_D2Q9.multicomponent_multiphase.multi).

    python examples/two_fluid_demix.py [--nx 128] [--ny 128] [--steps 3000] [--every 300] [--G 3.0]

Both fluids start at rho = 0.5 (1 + 1 % noise) everywhere in a periodic box, with a `linear` Shan-Chen pair force of strength
G between them.  Above the demixing threshold (about G rho_total > 2 for equal viscosities) the noise grows into domains of one fluid or
the other.  Printed every few hundred steps: the order parameter <|rho_1 - rho_2| / (rho_1 + rho_2)>, which rises from ~0.005
towards 1 as the fluids separate, and each fluid's mass, which the pair force conserves.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.multicomponent_multiphase.multi import Fluid, Simulation_Runner      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--ny", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--every", type=int, default=300)
    ap.add_argument("--G", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    sim = Simulation_Runner(nx=a.nx, ny=a.ny, num_populations=2)
    sim.set_bary_velocity(np.zeros((a.nx, a.ny)), np.zeros((a.nx, a.ny)))      # at rest
    for i in range(2):
        fluid = Fluid(sim, i, nu=1. / 6. + 0.02 * i, bc='periodic')
        sim.add_fluid(fluid)
        fluid.initialize(0.5 * (1. + 0.01 * rng.standard_normal((a.nx, a.ny))), f_amp=0.)
    sim.complete_setup()
    sim.add_interaction_force(0, 1, a.G, bc='periodic', potential='linear')
    print(sim.engine.hot_kernel().split(" (")[0])
    done = 0
    while done < a.steps:
        n = min(a.every, a.steps - done)
        sim.run(n)
        done += n
        rho = np.asarray(sim.rho, np.float64)
        order = np.abs(rho[:, :, 0] - rho[:, :, 1]) / (rho[:, :, 0] + rho[:, :, 1])
        print("step %5d: order parameter %.4f, masses %.3f %.3f, min rho %.3f" % (done, order.mean(), rho[:, :, 0].sum(), rho[:, :, 1].sum(), rho.min()))


if __name__ == "__main__":
    main()
