#!/usr/bin/env python3
"""Cost of the spectral screened-Poisson solve and of the Fisher step coupled to it: fused, un-fused, the lattice alone, rocFFT.

    python tools/spectral_bench.py [--sizes 256,512,1024,2048,4096] [--rounds 3] > profiles/spectral_bench.txt

For every box n x n, on objects created once and measured `rounds` times IN ALTERNATION (best of the rounds; every sample is host
wall-clock time around work that ends in a device synchronise):
  solve, fused        lb_spectral_velocity(sp, s, scale, 0): k_sp_rows_fwd<real> (4 B read + 8 B written per cell), k_sp_cols_mid
                      (8 + 8, then twice 8 + 8: 48 B, the re-reads its own lines), k_sp_rows_inv<velocity> (2 x (8 + 4) = 24 B): 84 B
  solve, phases       the literal port: the charge copied in (device to device), lb_spectral_transform, _screen, _grad_multiply and two
                      inverse lb_spectral_transform, a host wait after each, as the reference waits after each of its passes:
                      8 launches, 16 B each per array they touch
  torch.fft           torch.fft.fft2 of the complex charge and two torch.fft.ifft2: rocFFT's price for the three transforms ALONE
                      (no cast, screening, multipliers, real part or scale), one wait at the end
  step, fused         lb_run_screened(steps): k_ad_moments (36 + 4 B), the three launches above, k_ad_step (72 + 8 B): 204 B
  step, phases        lb_move, lb_update_hydro, lb_spectral_velocity, lb_update_feq, lb_collide_particles, a host wait after each (the
                      literal port's step costs this plus `solve, phases` minus `solve, fused`)
  k_ad_step           lb_run(steps) with lb_set_variant(0) on a lattice of the same size with an imposed velocity: the step without
                      its solve (80 B)
Printed per size: microseconds per solve / step, the ratios, and GB/s at the bytes above.
"""
import argparse
import ctypes as ct
import os
import sys
import time

import torch            # first: one HIP runtime in the process, torch's; the library binds to it
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "2d-lb_amd"))

from LB_D2Q9 import _native                 # noqa: E402
from LB_D2Q9.simulation import Simulation   # noqa: E402

OMEGA, G = 0.8, 0.01


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def droplet(n):
    x = (np.arange(n, dtype=np.float64) - n // 2) / (n / 3.)
    return np.asfortranarray(np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / 0.25).astype(np.float32))


def lattice(n, rho, sp, scale, L):
    sim = Simulation(n, n, OMEGA, bc="open", semantics="diffusion")
    sim.set_reaction(G)
    zero = np.zeros((n, n), np.float32)
    sim.set_fields(rho, zero, zero)
    _native.check(L.lb_spectral_velocity(sp, sim._h, scale, 0))
    sim.update_feq()
    sim.init_pop()
    return sim


def case(n, rounds):
    L = _native.lib()
    rho = droplet(n)
    scale = -3.0 / n                        # (a lattice velocity of a few 1e-3: the state stays smooth and finite)
    reps = int(max(3, min(200, 4.0e7 / (float(n) * n))))
    sp = ct.c_void_p()
    _native.check(L.lb_spectral_create(n, n, 0, 1.0, ct.byref(sp)))
    fused, lit, alone = (lattice(n, rho, sp, scale, L) for _ in range(3))
    alone.set_variant(0)
    charge = torch.from_numpy(np.ascontiguousarray(rho.T)).to("cuda").to(torch.complex64)
    spec = torch.fft.fft2(charge)

    def solve_fused():
        for _ in range(reps):
            _native.check(L.lb_spectral_velocity(sp, fused._h, scale, 0))

    def solve_phases():
        for _ in range(reps):
            _native.check(L.lb_spectral_set(sp, 0, charge.data_ptr(), 1))
            for call in ((L.lb_spectral_transform, 0, 1), (L.lb_spectral_screen,), (L.lb_spectral_grad_multiply,),
                         (L.lb_spectral_transform, 1, 0), (L.lb_spectral_transform, 2, 0)):
                _native.check(call[0](sp, *call[1:]))
                torch.cuda.synchronize()

    def torch_fft():
        for _ in range(reps):
            a = torch.fft.fft2(charge)
            torch.fft.ifft2(a)
            torch.fft.ifft2(spec)

    def step_fused():
        _native.check(L.lb_run_screened(sp, fused._h, scale, reps))

    def step_phases():
        for _ in range(reps):
            lit.move()
            lit.update_hydro()
            _native.check(L.lb_spectral_velocity(sp, lit._h, scale, 0))
            lit.sync()
            lit.update_feq()
            lit.collide_particles()

    samples = {"solve, fused": solve_fused, "solve, phases": solve_phases, "torch.fft": torch_fft, "step, fused": step_fused,
               "step, phases": step_phases, "k_ad_step": lambda: alone.run(reps, wait=False)}
    for fn in samples.values():
        fn()                                # warm-up (rocFFT plans among it)
    best = {k: None for k in samples}
    for _ in range(rounds):
        for k, fn in samples.items():
            t = wall(fn)
            best[k] = t if best[k] is None else min(best[k], t)
    ok = all(s.check()["n_nonfinite"] == 0 for s in (fused, lit, alone))
    cells = float(n) * n
    us = {k: best[k] / reps * 1e6 for k in samples}
    gb = {"solve, fused": 84., "step, fused": 204., "k_ad_step": 80.}
    print("n=%5d  %d solves / steps per sample; finite: %s" % (n, reps, ok))
    for k in samples:
        extra = "  %7.0f GB/s at %.0f B per cell" % (gb[k] * cells / us[k] / 1e3, gb[k]) if k in gb else ""
        print("    %-14s %10.2f us%s" % (k, us[k], extra))
    print("    the fused solve: %.2f x the phases, %.2f x torch.fft's three transforms; the fused step: %.2f x the phases, %.2f x k_ad_step's "
          "time; the solve is %.0f %% of the fused step" % (us["solve, phases"] / us["solve, fused"], us["torch.fft"] / us["solve, fused"],
                                                         us["step, phases"] / us["step, fused"], us["step, fused"] / us["k_ad_step"],
                                                         100. * us["solve, fused"] / us["step, fused"]), flush=True)
    for s in (fused, lit, alone):
        s.close()
    _native.check(L.lb_spectral_destroy(sp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("spectral_bench needs a GPU: nothing is measured without one")
    print("# spectral screened-Poisson solve and the coupled Fisher step: microseconds per solve / step, best of %d rounds alternating the "
          "samples; wall clock around synchronised work; ratios > 1: the fused form is that much faster" % a.rounds)
    for n in [int(k) for k in a.sizes.split(",")]:
        case(n, a.rounds)


if __name__ == "__main__":
    main()
