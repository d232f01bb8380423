#!/usr/bin/env python3
"""Two strains expanding into a nutrient, with demographic noise (the reference's stochastic_nutrients.Expansion, fused in HIP).

    python examples/stochastic_expansion.py [--steps 600] [--every 150] [--seed 0]

Both strains are inoculated well mixed in a strip along the edge y = 0 of an open box filled with nutrient; strain 1 grows a little
faster.  They eat the nutrient where they are and spread into what is left ahead of them; the multiplicative noise (strength Dg ~ mu /
Nb per strain, drawn inside the kernel from a seeded Philox stream, one launch per step for both strains and the nutrient) makes the
two take turns at the front.  Every `every` steps: each strain's mass, the nutrient left, the front row -- the largest y at which the
strains' summed row-average exceeds the cutoff -- and the noise counters.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.advecting_range_expansion.stochastic_nutrients import Expansion      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--every", type=int, default=150)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    sim = Expansion(Lx=8., Ly=16., mu_list=[1.0, 1.1], D_list=[1., 1.], Nb=20., Dc=1., N=10, seed=a.seed)
    print("grid %d x %d, omega %s, omega_nutrient %s, G %s, Dg %s, zero_cutoff %s"
          % (sim.nx, sim.ny, sim.omega, sim.omega_nutrient, sim.lb_G, sim.lb_Dg, sim.zero_cutoff))
    done = 0
    while done < a.steps:
        n = min(a.every, a.steps - done)
        sim.run(n)
        done += n
        rho = sim.get_fields()["rho"]
        strains = rho[:, :, :-1]
        rows = np.nonzero(strains.sum(axis=2).mean(axis=0) > float(sim.zero_cutoff))[0]
        print("step %5d  t = %.3f T  mass %s  nutrient left %.1f  front row %d of %d  noise counters %s"
              % (done, done * sim.delta_t, ", ".join("%.1f" % m for m in strains.sum(axis=(0, 1))), float(rho[:, :, -1].sum()),
                 int(rows.max()) if len(rows) else -1, sim.ny, [t for _, _, t in sim.noise()]))
    sim.sim.close()


if __name__ == "__main__":
    main()
