#!/usr/bin/env python3
"""Throughput of the scalar-lattice kernels k_ad_step and k_ad_tile4 (every shape) against the device's own copy rate.

    python tools/scalar_bench.py [--sizes 512,1024,2048,4096,8192] [--steps 40] [--rounds 3] > profiles/scalar_bench.txt

For every box size, both families (periodic, open) and G = 0 / G != 0: the engine's timers around lb_run(steps) with
k_ad_step forced (K_STEP) and with k_ad_tile4 forced in each of its three shapes (TILES, the shape in the ROWS field), taken
`rounds` times IN ALTERNATION -- step, tile shape 0, 1, 2, copy, step, ... -- on the same handle, with lb_copy_calibration (a
16-byte-per-lane copy of one lattice into the other: known bytes, the streaming ceiling in the kernel's own access shape);
best of the rounds.  Printed per case: MLUPS of each, k_ad_step's compulsory traffic 80 B x updates / time (72 B of
populations + 8 B of u, v) against the copy rate, and the best tile shape's rate over k_ad_step's -- what the size rule of
plan.cpp (scalar_use_tiles) is read from: the tiles are chosen only where that ratio is above 1 in every case of a size.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.simulation import Simulation      # noqa: E402
from LB_D2Q9.variants import K_STEP, TILES     # noqa: E402

W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4, dtype=np.float32)


def case(n, bc, G, steps, rounds):
    s = Simulation(n, n, 1.2, bc=bc, semantics="diffusion")
    s.set_reaction(G)
    x = np.arange(n, dtype=np.float32)
    u = np.asfortranarray(0.05 * np.sin(2 * np.pi * x / n)[None, :] * np.ones((n, 1), np.float32))
    v = np.asfortranarray(0.05 * np.cos(2 * np.pi * x / n)[:, None] * np.ones((1, n), np.float32))
    s.set_fields(np.zeros((n, n), np.float32), u, v)
    f0 = np.empty((n, n, 9), np.float32, order="F")
    f0[:] = 0.5 * W[None, None, :]
    s.set_f(f0)
    del f0
    variants = [K_STEP] + [TILES | (k << 2) for k in (1, 2, 3)]      # k_ad_step; k_ad_tile4 shapes 0, 1, 2
    for v in variants:                              # warm-up
        s.set_variant(v)
        s.run(steps)
    best, best_copy = [None] * 4, 0.
    for _ in range(rounds):
        for i, v in enumerate(variants):
            s.set_variant(v)
            ms = s.timed_run(steps)
            best[i] = ms if best[i] is None else min(best[i], ms)
        gbs, _ = s.copy_calibration(iters=10)
        best_copy = max(best_copy, gbs)
    upd = float(n) * n * steps
    mlups = [upd / (ms * 1e-3) / 1e6 for ms in best]
    gb = 80. * mlups[0] * 1e6 / 1e9
    print("%-9s n=%5d G=%-5g  k_ad_step %7.0f MLUPS (%5.0f GB/s at 80 B, copy %5.0f GB/s, ratio %.2f)  k_ad_tile4 32x16x2 %7.0f  "
          "32x16x1 %7.0f  16x16 %7.0f  best tile / step %.2f"
          % (bc, n, G, mlups[0], gb, best_copy, gb / best_copy, mlups[1], mlups[2], mlups[3], max(mlups[1:]) / mlups[0]), flush=True)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert a.steps % 4 == 0
    print("# scalar lattices: k_ad_step and k_ad_tile4 (three shapes), %d steps per sample, best of %d rounds alternating step / tiles / "
          "lb_copy_calibration on one handle" % (a.steps, a.rounds))
    for n in [int(k) for k in a.sizes.split(",")]:
        for bc in ("periodic", "open"):
            for G in (0., 0.01):
                case(n, bc, G, a.steps, a.rounds)


if __name__ == "__main__":
    main()
