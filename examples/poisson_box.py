#!/usr/bin/env python3
"""A few Gaussian sources in a grounded box, solved to tolerance by the LB Poisson solver (LB_D2Q9.poisson.Poisson_Solver).

    python examples/poisson_box.py [--n 256] [--tolerance 1e-6] [--max-iterations 200000]

The solver relaxes rho until it has stopped changing; the stop is decided on the device (one fused launch and one small one per
iteration, four bytes read back per batch of iterations).  Printed: the iteration count, the last ratio, and how well the result
solves a Poisson problem: the five-point Laplacian of rho is proportional to the source, so the residual printed is the RMS of
laplace(rho) + c source over the interior, relative to the RMS of c source, with the one constant c fitted by least squares.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.poisson import Poisson_Solver      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--tolerance", type=float, default=1e-6)
    ap.add_argument("--max-iterations", type=int, default=200000)
    a = ap.parse_args()
    n = a.n
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    src = np.zeros((n, n))
    for cx, cy, s, amp in ((0.3, 0.3, 0.05, 1.0), (0.7, 0.4, 0.08, 0.6), (0.5, 0.75, 0.04, 1.5)):
        src += amp * np.exp(-(((x - cx * n) / (s * n)) ** 2 + ((y - cy * n) / (s * n)) ** 2))
    src = np.asfortranarray((1e-3 * src).astype(np.float32))
    ps = Poisson_Solver(nx=n, ny=n, sources=src, delta_t=0.5, delta_x=1., rho_on_boundary=0., tolerance=a.tolerance)
    ps.run(a.max_iterations)
    rho = np.asarray(ps.rho, np.float64)
    print("iterations: %d, converged: %s, last ratio: %.3e, max rho: %.4e"
          % (ps.num_iterations, ps.converged, ps.sim.solve(0)[2], rho.max()))
    lap = (rho[2:, 1:-1] + rho[:-2, 1:-1] + rho[1:-1, 2:] + rho[1:-1, :-2] - 4. * rho[1:-1, 1:-1])[1:-1, 1:-1]
    s = src.astype(np.float64)[2:-2, 2:-2]
    c = -float((lap * s).sum() / (s * s).sum())
    print("laplace(rho) = -%.4f source; residual %.3e of the source term's RMS"
          % (c, np.sqrt(((lap + c * s) ** 2).mean()) / np.sqrt(((c * s) ** 2).mean())))
    print("largest |grad rho| (u, v of the stop): %.3e" % np.hypot(np.asarray(ps.u), np.asarray(ps.v)).max())


if __name__ == "__main__":
    main()
