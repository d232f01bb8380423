#!/usr/bin/env python3
"""Cost of a step of noisy strains on a shared nutrient: fused, un-fused, and beside the coupled set that moves the same bytes.

    python tools/expansion_bench.py [--sizes 256,512,1024,2048,4096,8192] [--rounds 3] > profiles/expansion_bench.txt

For every box n x n, family (open, periodic) and number of strains NP = 1, 2, 3, on objects created once and measured `rounds` times IN
ALTERNATION (best of the rounds; every sample is host wall-clock time around work that ends in a device synchronise):
  noisy      lb_run_expansion(steps), every strain with Dg > 0: k_ex_step gathers and stores NP + 1 lattices (72 B each per cell), loads
             u and v once (8 B) and draws NP lanes of normals in registers: 72 (NP + 1) + 8 B per cell and step
  quiet      the same handles with Dg = 0 on every strain: the same bytes, nothing drawn
  phases     the un-fused sequence on a set of its own -- lb_move on every member, lb_update_hydro_expansion, lb_update_feq on every
             member, lb_collide_expansion -- with a host wait after each, as the reference waits after each of its launches
  coupled    lb_run_coupled(steps) on NP + 1 LB_SEM_MULTIFIELD handles of the same box (open: the closed box LB_BC_BOX; periodic:
             periodic): k_mf_step moves the same bytes with no noise, no cutoff and no floor -- the yardstick
  copy       torch's device-to-device copy of 36 (NP + 1) n^2 B, read and written once: the same bytes but u, v
Printed per case: microseconds per step, GB/s at 72 (NP + 1) + 8 B per cell, and the ratios coupled / noisy (the share of the
yardstick's rate the noisy step reaches), coupled / quiet, phases / noisy.
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

from LB_D2Q9 import _native                         # noqa: E402
from LB_D2Q9.expansion_set import Expansion_Set     # noqa: E402
from LB_D2Q9.simulation import Simulation           # noqa: E402

OMEGAS, OMEGA_N, GS, DGS, CUT = (1.1, 0.9, 1.25), 1.3, (0.01, 0.014, 0.012), (2.0e-3, 1.0e-3, 5.0e-4), 0.01


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def start(n, n_fields):
    """Smooth strains in [0.15, 0.55] and a nutrient in [0.7, 1], a velocity of a few 1e-2.  Over the thousands of steps of a case the
    strains eat the nutrient down; whether every density is still above the cutoff at the end is printed (boxes up to 2048^2)."""
    x = np.arange(n, dtype=np.float32)[:, None] / n
    y = np.arange(n, dtype=np.float32)[None, :] / n
    bump = (0.5 + 0.5 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)).astype(np.float32)
    rho = np.empty((n, n, n_fields), np.float32, order="F")
    for i in range(n_fields - 1):
        rho[:, :, i] = 0.15 + 0.4 * bump
    rho[:, :, n_fields - 1] = 1.0 - 0.3 * bump
    u = np.asfortranarray((0.03 * np.sin(2 * np.pi * y) * np.ones_like(x)).astype(np.float32))
    v = np.asfortranarray((0.03 * np.cos(2 * np.pi * x) * np.ones_like(y)).astype(np.float32))
    return rho, u, v


def expansion_set(n, n_strains, bc, rho, u, v):
    s = Expansion_Set(n, n, OMEGAS[:n_strains], OMEGA_N, GS[:n_strains], bc=bc, zero_cutoff=CUT)
    s.set_fields(rho, u, v)
    s.update_feq()
    s.init_pop()
    return s


def coupled_set(n, n_fields, bc, rho, u, v):
    ms = [Simulation(n, n, om, bc=bc, semantics="multifield") for om in (OMEGAS + (OMEGA_N,))[:n_fields]]
    for i, m in enumerate(ms):
        m.set_reaction(0.01)
        m.set_fields(0.2 * rho[:, :, i], u, v)       # (the coupled set's growth needs sum rho < 1)
        m.update_feq()
        m.init_pop()
    return ms


def case(n, bc, n_strains, rounds):
    L = _native.lib()
    nf = n_strains + 1
    rho, u, v = start(n, nf)
    fused, lit = expansion_set(n, n_strains, bc, rho, u, v), expansion_set(n, n_strains, bc, rho, u, v)
    lit.set_noise(DGS[:n_strains], 7)
    coupled = coupled_set(n, nf, "box" if bc == "open" else "periodic", rho, u, v)
    handles = (ct.c_void_p * nf)(*[m._h for m in coupled])
    src = torch.zeros(9 * nf * n * n, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    cells = float(n) * n
    reps = int(max(3, min(200, 1.2e9 / (cells * nf))))
    reps_lit = max(2, reps // 5)

    def noisy():
        fused.set_noise(DGS[:n_strains], 7)
        fused.run(reps, wait=False)

    def quiet():
        fused.set_noise(0., 7)
        fused.run(reps, wait=False)

    def phases():
        for _ in range(reps_lit):
            lit.step_phases()

    def copy():
        for _ in range(reps):
            dst.copy_(src)

    samples = {"noisy": (noisy, reps), "quiet": (quiet, reps), "phases": (phases, reps_lit),
               "coupled": (lambda: _native.check(L.lb_run_coupled(handles, nf, reps)), reps), "copy": (copy, reps)}
    for fn, _ in samples.values():
        fn()                                # warm-up
    best = {k: None for k in samples}
    for _ in range(rounds):
        for k, (fn, _) in samples.items():
            t = wall(fn)
            best[k] = t if best[k] is None else min(best[k], t)
    ok = all(c["n_nonfinite"] == 0 for s in (fused, lit) for c in s.check()) and all(m.check()["n_nonfinite"] == 0 for m in coupled)
    above = float(fused.get_fields(("rho",))["rho"].min()) >= CUT if n <= 2048 else None
    us = {k: best[k] / samples[k][1] * 1e6 for k in samples}
    b = 72. * nf + 8.
    print("n=%5d %-8s NP=%d  %d steps per sample (%d by phases); finite: %s; every density above the cutoff: %s"
          % (n, bc, n_strains, reps, reps_lit, ok, above))
    for k in samples:
        bytes_k = 72. * nf if k == "copy" else b
        extra = "" if k == "phases" else "  %7.0f GB/s at %.0f B per cell" % (bytes_k * cells / us[k] / 1e3, bytes_k)
        print("    %-8s %10.2f us%s" % (k, us[k], extra))
    print("    coupled / noisy = %.2f; coupled / quiet = %.2f; phases / noisy = %.1f"
          % (us["coupled"] / us["noisy"], us["coupled"] / us["quiet"], us["phases"] / us["noisy"]), flush=True)
    for s in [fused, lit] + coupled:
        s.close()
    del src, dst
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512,1024,2048,4096,8192")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if _native.device_count() < 1:
        raise SystemExit("expansion_bench needs a GPU: nothing is measured without one")
    print("# noisy strains on a shared nutrient: microseconds per step, best of %d rounds alternating the samples; wall clock around "
          "synchronised work" % a.rounds)
    for n in [int(k) for k in a.sizes.split(",")]:
        for bc in ("open", "periodic"):
            for n_strains in (1, 2, 3):
                case(n, bc, n_strains, a.rounds)


if __name__ == "__main__":
    main()
