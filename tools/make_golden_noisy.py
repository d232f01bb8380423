#!/usr/bin/env python3
"""Fixtures for the noisy collision of a scalar lattice, recorded from the reference's own OpenCL C.

    python tools/make_golden_noisy.py <reference dir>      # -> tests/golden/nf_*.npz

As tools/make_golden_scalar.py: a small C driver that #includes the reference's LB_D2Q9/D2Q9_diffusion.cl BY PATH, built with gcc
(-O1 -ffp-contract=off) in a temporary directory, drives the kernels in the order of reaction_diffusion/noisy_fisher_wave.py's run
(:420-430): move -> copy_buffer -> (move_bcs: pass) -> update_hydro_diffusion -> update_feq_diffusion ->
collide_particles_noisy_fisher.  The reference refills its random_normal buffer between steps from pyopencl's unseeded generator;
here the normals of step t are the project's stream (tests/noise_model.py: Philox4x32-10, float64 transcendental part) under the
recorded seed at noise counter t, rounded to float32 -- and stored in the fixture, so a test can feed the very same numbers.

The reference's box is the OPEN family.  For the PERIODIC family only the streaming differs, and streaming computes nothing: the tool
rolls the arrays itself and runs the reference's C for update_hydro, update_feq and the collision.

Files (arrays as the reference's host arrays: float32, F-ordered (nx, ny) / (nx, ny, 9)):
  nf_run_<family>_37x23   nx, ny, omega, G, Dg, seed, f0, u, v, z (50, nx, ny), steps and f_n, rho_n, feq_n for n in steps.  The tool
                          refuses to write unless rho stayed inside [0.02, 0.98] in every step: near rho = 1 a rounding difference
                          flips finite to NaN, and no tolerance can hold that.
  nf_phases_21x13         one step, the buffers after each phase, from a start with three groups of cells: rho ~ 1e-4 (the clamp fires
                          where z is negative enough), rho (1 - rho) < -1e-3 (NaN in all nine links), rho (1 - rho) > 1e-3 (finite);
                          no cell of the last two kinds lies in between.  clamped: the links the reference set to 0.
"""
import ctypes as ct
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_scalar import CS, CX, CY, DRIVER, GOLDEN, W, RefBox, start_state      # noqa: E402
from noise_model import normals32                                                        # noqa: E402

NOISY_DRIVER = DRIVER + r"""
void drv_collide_noisy(float *f, float *feq, float *rho, float *normal, float omega, float G, float Dg, const float *w, int nx, int ny)
{
    RANGE(1, collide_particles_noisy_fisher(f, feq, rho, normal, omega, G, Dg, w, nx, ny))
}
"""


def build_driver(ref, tmp):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "D2Q9_diffusion.cl")
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    src, so = os.path.join(tmp, "drv.c"), os.path.join(tmp, "drv.so")
    open(src, "w").write(NOISY_DRIVER % {"cl": cl})
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class NoisyBox(RefBox):
    """The reference's buffers and noisy_fisher_wave.py's run loop; periodic: the streaming is a roll made here."""

    def __init__(self, lib, f0, u, v, omega, G, Dg, seed, periodic=False):
        super(NoisyBox, self).__init__(lib, f0, u, v, omega, G)
        self.Dg, self.seed, self.t, self.periodic = np.float32(Dg), int(seed), 0, periodic
        self.z = []

    def move(self):
        if not self.periodic:
            return super(NoisyBox, self).move()
        for k in range(9):
            self.f[:, :, k] = np.roll(self.f[:, :, k], (CX[k], CY[k]), axis=(0, 1))
        self.fs[...] = self.f

    def collide(self):
        z = np.asfortranarray(normals32(self.nx, self.ny, self.seed, self.t))
        self.z.append(z)
        self.t += 1
        self.lib.drv_collide_noisy(self._p(self.f), self._p(self.feq), self._p(self.rho), self._p(z), ct.c_float(self.omega),
                                   ct.c_float(self.G), ct.c_float(self.Dg), self._p(W), self.nx, self.ny)


def save(name, out):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    assert size <= 400 * 1024, "fixture too large"


def record_run(lib, name, nx, ny, omega, G, Dg, seed, periodic, steps):
    rng = np.random.default_rng(seed)
    _, u, v = start_state(nx, ny, seed, True)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    rho = 0.1 + 0.8 * np.exp(-(((x - 0.4 * nx) / (0.25 * nx)) ** 2 + ((y - 0.55 * ny) / (0.3 * ny)) ** 2))      # in [0.1, 0.9]
    f0 = np.asfortranarray((W[None, None, :] * rho[:, :, None] * (1. + 0.01 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(np.float32))
    box = NoisyBox(lib, f0, u, v, omega, G, Dg, seed, periodic)
    out = dict(nx=nx, ny=ny, omega=np.float32(omega), G=np.float32(G), Dg=np.float32(Dg), seed=np.uint64(seed), f0=f0, u=u, v=v,
               steps=np.array(steps, np.int32))
    lo, hi = 1., 0.
    for n in range(1, max(steps) + 1):
        box.run(1)
        lo, hi = min(lo, float(box.rho.min())), max(hi, float(box.rho.max()))
        if n in steps:
            out["f_%d" % n], out["rho_%d" % n], out["feq_%d" % n] = box.f.copy(order="F"), box.rho.copy(order="F"), box.feq.copy(order="F")
    print("%s: rho stayed inside [%.4f, %.4f]" % (name, lo, hi))
    if not (lo >= 0.02 and hi <= 0.98 and np.isfinite(box.f).all()):
        raise SystemExit("%s: rho left [0.02, 0.98]: not written" % name)
    out["z"] = np.stack(box.z)
    save(name, out)


def record_phases(lib, name, nx, ny, omega, G, Dg, seed):
    _, u, v = start_state(nx, ny, seed, True)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    rho = np.where(x < nx // 3, 1.0e-4, np.where(x < 2 * (nx // 3), 0.5, 1.3)) * (1. + 0.02 * np.sin(1.7 * y))
    f0 = np.asfortranarray((W[None, None, :] * rho[:, :, None]).astype(np.float32))
    box = NoisyBox(lib, f0, u, v, omega, G, Dg, seed)
    out = dict(nx=nx, ny=ny, omega=np.float32(omega), G=np.float32(G), Dg=np.float32(Dg), seed=np.uint64(seed), f0=f0, u=u, v=v)
    box.move()
    out["f_move"] = box.f.copy(order="F")
    box.hydro()
    out["rho_hydro"] = box.rho.copy(order="F")
    box.update_feq()
    out["feq_feq"] = box.feq.copy(order="F")
    box.collide()
    out["f_collide"], out["z"] = box.f.copy(order="F"), box.z[0]
    room = box.rho.astype(np.float64) * (1. - box.rho.astype(np.float64))
    nan_cells, tiny = room < -1.0e-3, box.rho < 2.0e-4
    finite_cells = room > 1.0e-3
    if not np.all(nan_cells | finite_cells | tiny) or not np.all(room[tiny] > 5.0e-5):
        raise SystemExit("%s: a cell lies between the groups: not written" % name)
    isnan = np.isnan(box.f)
    clamped = (box.f == 0.) & ~isnan
    if not (np.array_equal(isnan.all(axis=2), nan_cells) and np.array_equal(isnan.any(axis=2), nan_cells)):
        raise SystemExit("%s: the NaN cells are not the cells with rho (1 - rho) < 0: not written" % name)
    if not (clamped[tiny].any() and (~clamped[tiny]).any() and nan_cells.any() and finite_cells.any()):
        raise SystemExit("%s: a group is empty: not written" % name)
    print("%s: %d NaN cells, %d clamped links in %d cells" % (name, nan_cells.sum(), clamped.sum(), clamped.any(axis=2).sum()))
    out["nan_cells"], out["clamped"] = nan_cells, clamped
    save(name, out)


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(ref, tmp)
        record_run(lib, "nf_run_open_37x23", 37, 23, 1.1, 1.0e-4, 1.0e-3, 21, False, (1, 10, 50))
        record_run(lib, "nf_run_periodic_37x23", 37, 23, 1.1, 1.0e-4, 1.0e-3, 24, True, (1, 10, 50))
        record_phases(lib, "nf_phases_21x13", 21, 13, 1.2, 1.0e-4, 1.0e-3, 23)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
