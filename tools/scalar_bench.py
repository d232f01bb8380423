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

    python tools/scalar_bench.py --noise [--sizes 1024,4096] >> profiles/scalar_bench.txt

The noise column: the same alternation on one handle with the noisy collision off (lb_set_noise(0): the plain kernels, the
yardstick) and on (Dg = 1e-4, the kernels that draw Philox normals in registers), G = 1e-4 in both; per case the rates of
k_ad_step and of the three tile shapes without and with noise -- the tiles with each of their two noise plans, the noise plane in
LDS and a draw per cell (the A/B switch STEP4_NO_AHEAD) --, noisy over noiseless for k_ad_step and for the best tile shape, the
noisy best tile over the noisy step, and the round-to-round spread (max / min - 1) of the noiseless samples.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9.noisy_simulation import NoisySimulation      # noqa: E402
from LB_D2Q9.simulation import Simulation      # noqa: E402
from LB_D2Q9.variants import K_STEP, STEP4_NO_AHEAD, TILES     # noqa: E402

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


def noise_case(n, bc, steps, rounds):
    s = NoisySimulation(n, n, 1.2, bc=bc)
    s.set_reaction(1e-4)
    x = np.arange(n, dtype=np.float32)
    u = np.asfortranarray(0.05 * np.sin(2 * np.pi * x / n)[None, :] * np.ones((n, 1), np.float32))
    v = np.asfortranarray(0.05 * np.cos(2 * np.pi * x / n)[:, None] * np.ones((1, n), np.float32))
    s.set_fields(np.zeros((n, n), np.float32), u, v)
    f0 = np.empty((n, n, 9), np.float32, order="F")
    f0[:] = 0.5 * W[None, None, :]
    s.set_f(f0)
    del f0
    variants = [K_STEP] + [TILES | (k << 2) for k in (1, 2, 3)]
    # noiseless step, tiles 0 1 2; noisy step, tiles 0 1 2 with the noise plane in LDS; noisy tiles 0 1 2 drawing per cell
    configs = [(dg, v) for dg in (0., 1e-4) for v in variants] + [(1e-4, v | STEP4_NO_AHEAD) for v in variants[1:]]
    for dg, v in configs:                           # warm-up
        s.set_noise(dg, 1)
        s.set_variant(v)
        s.run(steps)
    samples = [[] for _ in configs]
    for _ in range(rounds):
        for i, (dg, v) in enumerate(configs):
            s.set_noise(dg, 1)
            s.set_variant(v)
            samples[i].append(s.timed_run(steps))
    upd = float(n) * n * steps
    mlups = [upd / (min(ms) * 1e-3) / 1e6 for ms in samples]
    spread = max(max(ms) / min(ms) - 1. for ms in samples[:4])
    plain, noisy, cell = mlups[:4], mlups[4:8], mlups[8:]
    print("%-9s n=%5d  plain: k_ad_step %7.0f MLUPS  tiles 32x16x2 %7.0f  32x16x1 %7.0f  16x16 %7.0f | noisy: k_ad_step %7.0f  tiles, noise plane "
          "%7.0f  %7.0f  %7.0f  tiles, per cell %7.0f  %7.0f  %7.0f | noisy / plain: step %.2f  best tile plane %.2f  per cell %.2f | "
          "noisy best tile / noisy step: plane %.2f  per cell %.2f | plain spread %.1f %%"
          % (bc, n, plain[0], plain[1], plain[2], plain[3], noisy[0], noisy[1], noisy[2], noisy[3], cell[0], cell[1], cell[2],
             noisy[0] / plain[0], max(noisy[1:]) / max(plain[1:]), max(cell) / max(plain[1:]), max(noisy[1:]) / noisy[0],
             max(cell) / noisy[0], 100. * spread), flush=True)
    assert np.isfinite(s.get_fields(("rho",))["rho"]).all()
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert a.steps % 4 == 0
    if a.noise:
        print("# scalar lattices, the noisy collision (k_ad_tile4: both noise plans): G = 1e-4, Dg = 0 / 1e-4, %d steps per sample, best of %d "
              "rounds alternating the eleven kernels on one handle" % (a.steps, a.rounds))
        for n in [int(k) for k in a.sizes.split(",")]:
            for bc in ("periodic", "open"):
                noise_case(n, bc, a.steps, a.rounds)
        return
    print("# scalar lattices: k_ad_step and k_ad_tile4 (three shapes), %d steps per sample, best of %d rounds alternating step / tiles / "
          "lb_copy_calibration on one handle" % (a.steps, a.rounds))
    for n in [int(k) for k in a.sizes.split(",")]:
        for bc in ("periodic", "open"):
            for G in (0., 0.01):
                case(n, bc, G, a.steps, a.rounds)


if __name__ == "__main__":
    main()
