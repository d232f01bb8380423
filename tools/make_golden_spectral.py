#!/usr/bin/env python3
"""Fixtures for the spectral screened-Poisson solver and the Fisher lattice coupled to it, recorded from the float64 model.

    python tools/make_golden_spectral.py        # -> tests/golden/sp_solve_30x18.npz, tests/golden/sp_fisher_30x18.npz

The reference's spectral_poisson/screened_poisson.py needs pyopencl and gpyfft and has no C to drive on a host; what it computes is
numpy's fft2 / ifft2 with the multipliers tests/spectral_model.py restates.  The arrays are that model's, in float64 / complex128.

Case: Screened_Fisher_Wave(Lx=3, Ly=1.8, vc=1, lam=1, R0=0.5, time_prefactor=1, N=10): a 30 x 18 box (mixed radices, not square),
omega = 0.8, G = 0.01, scale = -0.1; the initial density is the droplet times 1 + 0.05 x a normal draw (seed 20240611).

  sp_solve_30x18    charge (float32, what the device is given), lam, spec, xgrad, ygrad (complex128, (nx, ny))
  sp_fisher_30x18   nx, ny, omega, G, lam, scale, rho0, steps and for each family b in (open, periodic) and each n in steps
                    b_f_n, b_rho_n, b_u_n, b_v_n: the state after n steps (rho, u, v: those of the last step's update_hydro and
                    update_u_and_v), float64

A fixture is refused unless the float32 model stays within contract_tol(n) of the float64 model at every recorded step,
max |u| < 0.15 and 0 <= rho <= 1.5 throughout.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spectral_model as M          # noqa: E402
from scalar_model import contract_tol   # noqa: E402

CASE = dict(Lx=3., Ly=1.8, vc=1., lam=1., R0=0.5, time_prefactor=1., N=10)
SEED = 20240611
STEPS = (1, 10, 50)


def models(bc, p, rho0):
    out = []
    for dtype in (np.float64, np.float32):
        m = M.ScreenedFisherModel(p["nx"], p["ny"], p["omega"], p["lb_G"], CASE["lam"], p["scale"], bc=bc, dtype=dtype)
        m.redo_initial_condition(rho0)
        out.append(m)
    return out


def main():
    p = M.fisher_lattice_parameters(CASE["Lx"], CASE["Ly"], CASE["vc"], CASE["time_prefactor"], CASE["N"])
    nx, ny = p["nx"], p["ny"]
    assert (nx, ny) == (30, 18)
    rho0 = M.noisy_droplet(nx, ny, CASE["N"], CASE["R0"], SEED)

    spec, xg, yg = M.solve(rho0, CASE["lam"])
    s32 = M.solve(rho0, CASE["lam"], np.complex64)
    print("float32 solve off the float64 one: %.2e of max |grad|" % max(abs(a - b).max() / abs(b).max() for a, b in zip(s32[1:], (xg, yg))))
    np.savez_compressed(os.path.join(GOLDEN, "sp_solve_30x18.npz"), charge=rho0, lam=CASE["lam"], spec=spec, xgrad=xg, ygrad=yg)

    out = dict(nx=nx, ny=ny, omega=p["omega"], G=p["lb_G"], lam=CASE["lam"], scale=p["scale"], rho0=rho0, steps=np.array(STEPS))
    for bc in ("open", "periodic"):
        m64, m32 = models(bc, p, rho0)
        done = 0
        for n in STEPS:
            for _ in range(n - done):
                m64.step()
                m32.step()
                assert np.abs(m64.u).max() < 0.15 and np.abs(m64.v).max() < 0.15, "max |u| too large for a fixture"
                assert m64.rho.min() >= 0. and m64.rho.max() <= 1.5, "rho leaves [0, 1.5]"
            done = n
            tol = contract_tol(n)
            for k in ("f", "rho", "u", "v"):
                d = np.abs(getattr(m32, k).astype(np.float64) - getattr(m64, k)).max()
                print("%-8s step %3d  %-3s float32 - float64 = %.2e (tolerance %.2e)" % (bc, n, k, d, tol[k]))
                assert d <= tol[k], "the float32 model leaves the contract: no fixture"
                out["%s_%s_%d" % (bc, k, n)] = getattr(m64, k).copy()
    np.savez_compressed(os.path.join(GOLDEN, "sp_fisher_30x18.npz"), **out)
    for name in ("sp_solve_30x18.npz", "sp_fisher_30x18.npz"):
        print(name, os.path.getsize(os.path.join(GOLDEN, name)), "bytes")


if __name__ == "__main__":
    main()
