#!/usr/bin/env python3
"""Two strains expanding from the wall of a closed box (the reference's Fisher_Expansion, fused in HIP).

    python examples/fisher_expansion.py [--steps 400] [--every 100]

Strain 0 grows faster (mu = 1.2 against 1.0); both are inoculated side by side along the wall y = 0 and spread into the box
as Fisher waves of speed ~ 2 sqrt(D mu).  Every `every` steps the front position of each strain is printed: the largest y,
in units of the characteristic length, at which its column-averaged density exceeds one half of its maximum.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.advecting_range_expansion.deterministic_fisher_waves import Fisher_Expansion      # noqa: E402


def fronts(rho, N):
    out = []
    for i in range(rho.shape[2]):
        profile = rho[:, :, i].mean(axis=0)                     # along y
        above = np.nonzero(profile > 0.5 * profile.max())[0]
        out.append(above.max() / float(N) if len(above) else 0.)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=100)
    a = ap.parse_args()
    sim = Fisher_Expansion(Lx=8., Ly=16., mu_list=[1.2, 1.0], D_list=[1., 1.], N=20,
                           initial_frac_widths=[0.5, 0.5], initial_frac_indices=[0, 1])
    print("grid %d x %d, omega %s, G %s" % (sim.nx, sim.ny, sim.omega, sim.lb_G))
    done = 0
    while done < a.steps:
        n = min(a.every, a.steps - done)
        sim.run(n)
        done += n
        rho = sim.get_fields()["rho"]
        print("step %5d  t = %.3f T  fronts (L): %s  total mass %s"
              % (done, done * sim.delta_t, ", ".join("%.2f" % y for y in fronts(rho, sim.N)), rho.sum(axis=(0, 1))))


if __name__ == "__main__":
    main()
