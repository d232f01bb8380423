#!/usr/bin/env python3
"""Dye carried by a periodic double shear layer, coupled to the live flow in EVERY step: one launch advances both lattices.

    python examples/dye_in_live_flow.py [--n 512] [--frames 20] [--every 50] [--out frames_dye_live] [--form -1]

The shear layer of ``dye_in_shear_layer.py`` with the dye advected through ``LB_D2Q9.coupled.Advected_Scalars``: in each step the dye
sees the velocity the flow's step forms from its streamed populations, handed on in registers (``--form 1``) or read from the flow's
own planes (``--form 0``) -- no copy of u, v and no velocity that is some steps old.  ``Frame_Dumper`` writes one image of the dye per
frame; at the end the dye's mass, the flow's Mach number and the kernel that ran are printed.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.coupled import Advected_Scalars       # noqa: E402
from LB_D2Q9.frames import Frame_Dumper            # noqa: E402
from LB_D2Q9.simulation import Simulation          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--every", type=int, default=50, help="steps per frame")
    ap.add_argument("--form", type=int, default=-1, choices=(-1, 0, 1), help="-1: the planner's choice, 1: one launch per step, 0: one per lattice")
    ap.add_argument("--out", default="frames_dye_live")
    a = ap.parse_args()
    n = a.n
    x, y = np.meshgrid(np.arange(n) / n, np.arange(n) / n, indexing="ij")
    u0 = 0.05 * np.where(y <= 0.5, np.tanh(80. * (y - 0.25)), np.tanh(80. * (0.75 - y)))
    v0 = 0.05 * 0.05 * np.sin(2. * np.pi * (x + 0.25))
    flow = Simulation(n, n, 1.9, bc="periodic")
    flow.init_equilibrium(np.ones((n, n)), u0, v0)
    dye = Simulation(n, n, 1.8, bc="periodic", semantics="diffusion")
    stripe = ((y > 0.2) & (y < 0.3)) | ((y > 0.7) & (y < 0.8))
    dye.init_equilibrium(stripe.astype(np.float32), u0, v0)
    pair = Advected_Scalars(flow, [dye])

    dumper = Frame_Dumper(dye, "rho", num_steps_per_draw=a.every, max_magnitude=1.0, render_folder=a.out,
                          run_func=lambda steps: pair.run(steps, form=a.form))
    frames = dumper.run(a.frames)
    health = pair.check()
    print("wrote %d frames to %s; dye mass %.6f, flow max Mach %.3f" % (len(frames), os.path.abspath(a.out),
                                                                        health["scalars"][0]["sum_rho"], health["flow"]["max_mach"]))
    print("kernel: %s" % pair.hot_kernel(a.form))


if __name__ == "__main__":
    main()
