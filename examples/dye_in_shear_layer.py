#!/usr/bin/env python3
"""Dye carried by a periodic double shear layer: a flow lattice and a scalar lattice coupled on the device.

    python examples/dye_in_shear_layer.py [--n 512] [--frames 20] [--every 50] [--out frames_dye]

The flow is a ``Simulation`` in a periodic box started from two shear layers with a small transverse kick; the dye is a
scalar lattice (``semantics='diffusion'``) whose imposed velocity is taken from the flow every ``--couple`` steps with
``set_velocity_from`` -- a device-to-device copy ordered behind the flow's kernels, no trip through the host.  Between two
couplings both lattices advance with their fused kernels.  ``Frame_Dumper`` writes one image of the dye per frame.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.frames import Frame_Dumper            # noqa: E402
from LB_D2Q9.simulation import Simulation          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--every", type=int, default=50, help="steps per frame")
    ap.add_argument("--couple", type=int, default=10, help="steps between two velocity updates of the dye")
    ap.add_argument("--out", default="frames_dye")
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

    def advance(steps):
        done = 0
        while done < steps:
            k = min(a.couple, steps - done)
            dye.set_velocity_from(flow)              # the flow's current u, v
            flow.run(k, wait=False)
            dye.run(k, wait=False)
            done += k
        dye.sync()

    dumper = Frame_Dumper(dye, "rho", num_steps_per_draw=a.every, max_magnitude=1.0, render_folder=a.out, run_func=advance)
    frames = dumper.run(a.frames)
    print("wrote %d frames to %s; dye mass %.6f, flow max Mach %.3f"
          % (len(frames), os.path.abspath(a.out), dye.check()["sum_rho"], flow.check()["max_mach"]))


if __name__ == "__main__":
    main()
