#!/usr/bin/env python3
"""Fixtures for scalar lattices, recorded from the reference's own OpenCL C.

    python tools/make_golden_scalar.py <reference dir>      # -> tests/golden/ad_*.npz

The reference's LB_D2Q9/D2Q9_diffusion.cl is plain C apart from the address-space qualifiers and the work-item id
built-in.  This tool writes a small C driver into a temporary directory that #includes that file BY PATH behind a handful
of #defines, builds it with gcc (-std=gnu99 -O1 -ffp-contract=off: no fused multiply-add, as an OpenCL compiler without
-cl-mad-enable), and drives the kernels in the order of reaction_diffusion/diffusion.py's Diffusion.run:
move -> copy_buffer -> (move_bcs: pass) -> update_hydro_diffusion -> update_feq_diffusion -> collide_particles[_fisher]
(the latter with the arguments in the order of the kernel's signature).  Only the recorded arrays are written; the driver
and the library built from it live and die in the temporary directory.  Nothing at test time needs the reference.

Arrays are the reference's host arrays: float32, F-ordered (nx, ny) / (nx, ny, 9)  (flat index k nx ny + y nx + x).
Every file holds nx, ny, omega, G, f0, u, v, steps and, for each n in steps, f_n, rho_n, feq_n: the buffers as the reference
holds them after n iterations (rho and feq are those of the last iteration's update_hydro / update_feq).
"""
import ctypes as ct
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4, dtype=np.float32)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1], dtype=np.int32)
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1], dtype=np.int32)
CS = np.float32(1. / np.sqrt(3.))          # np.float32(cs), diffusion.py:28, 303

DRIVER = r"""
#include <math.h>
static int g_gid[3];
#define __kernel
#define __global
#define __constant const
#define __read_only
#define __write_only
static inline int get_global_id(int d) { return g_gid[d]; }
#include "%(cl)s"

#define RANGE(nz, CALL)                                          \
    for (g_gid[2] = 0; g_gid[2] < (nz); ++g_gid[2])              \
        for (g_gid[1] = 0; g_gid[1] < ny; ++g_gid[1])            \
            for (g_gid[0] = 0; g_gid[0] < nx; ++g_gid[0]) { CALL; }

void drv_move(float *f, float *fs, const int *cx, const int *cy, int nx, int ny)
{
    RANGE(9, move(f, fs, cx, cy, nx, ny))
    RANGE(9, copy_buffer(fs, f, nx, ny))
}
void drv_hydro(float *f, float *u, float *v, float *rho, int nx, int ny) { RANGE(1, update_hydro_diffusion(f, u, v, rho, nx, ny)) }
void drv_feq(float *feq, float *rho, float *u, float *v, const float *w, const int *cx, const int *cy, float cs, int nx, int ny)
{
    RANGE(1, update_feq_diffusion(feq, rho, u, v, w, cx, cy, cs, nx, ny))
}
void drv_collide(float *f, float *feq, float omega, int nx, int ny) { RANGE(1, collide_particles(f, feq, omega, nx, ny)) }
void drv_collide_fisher(float *f, float *feq, float *rho, float omega, float G, const float *w, int nx, int ny)
{
    RANGE(1, collide_particles_fisher(f, feq, rho, omega, G, w, nx, ny))
}
"""


def build_driver(ref, tmp):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "D2Q9_diffusion.cl")
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    src, so = os.path.join(tmp, "drv.c"), os.path.join(tmp, "drv.so")
    open(src, "w").write(DRIVER % {"cl": cl})
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class RefBox(object):
    """The reference's buffers and its run loop."""

    def __init__(self, lib, f0, u, v, omega, G):
        self.lib = lib
        self.nx, self.ny = f0.shape[:2]
        self.f = np.asfortranarray(f0, dtype=np.float32).copy(order="F")
        self.fs = self.f.copy(order="F")                       # init_pop fills f and f_streamed alike
        self.feq = np.zeros_like(self.f, order="F")
        self.rho = np.zeros((self.nx, self.ny), np.float32, order="F")
        self.u = np.asfortranarray(u, dtype=np.float32).copy(order="F")
        self.v = np.asfortranarray(v, dtype=np.float32).copy(order="F")
        self.omega, self.G = np.float32(omega), np.float32(G)

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ct.c_void_p)

    def move(self):
        self.lib.drv_move(self._p(self.f), self._p(self.fs), self._p(CX), self._p(CY), self.nx, self.ny)

    def hydro(self):
        self.lib.drv_hydro(self._p(self.f), self._p(self.u), self._p(self.v), self._p(self.rho), self.nx, self.ny)

    def update_feq(self):
        self.lib.drv_feq(self._p(self.feq), self._p(self.rho), self._p(self.u), self._p(self.v), self._p(W), self._p(CX),
                         self._p(CY), ct.c_float(CS), self.nx, self.ny)

    def collide(self):
        if self.G != 0:
            self.lib.drv_collide_fisher(self._p(self.f), self._p(self.feq), self._p(self.rho), ct.c_float(self.omega),
                                        ct.c_float(self.G), self._p(W), self.nx, self.ny)
        else:
            self.lib.drv_collide(self._p(self.f), self._p(self.feq), ct.c_float(self.omega), self.nx, self.ny)

    def run(self, n):
        for _ in range(n):
            self.move()
            self.hydro()
            self.update_feq()
            self.collide()


def start_state(nx, ny, seed, flow):
    """A blob of concentration with 5 % noise on the populations; flow: a non-uniform imposed field, |u|, |v| <= 0.07."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    rho = 0.15 + 0.8 * np.exp(-(((x - 0.4 * nx) / (0.25 * nx)) ** 2 + ((y - 0.55 * ny) / (0.3 * ny)) ** 2))
    f0 = (W[None, None, :] * rho[:, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(np.float32)
    if flow:
        u = 0.07 * np.sin(2. * np.pi * y / ny + 0.3) * np.cos(np.pi * x / nx)
        v = 0.07 * np.cos(2. * np.pi * x / nx) * np.sin(np.pi * (y + 0.5) / ny)
    else:
        u, v = np.zeros((nx, ny)), np.zeros((nx, ny))
    return np.asfortranarray(f0), np.asfortranarray(u.astype(np.float32)), np.asfortranarray(v.astype(np.float32))


def record_run(lib, name, nx, ny, omega, G, flow, steps, seed):
    f0, u, v = start_state(nx, ny, seed, flow)
    box = RefBox(lib, f0, u, v, omega, G)
    out = dict(nx=nx, ny=ny, omega=np.float32(omega), G=np.float32(G), f0=f0, u=u, v=v, steps=np.array(steps, np.int32))
    done = 0
    for n in steps:
        box.run(n - done)
        done = n
        out["f_%d" % n], out["rho_%d" % n], out["feq_%d" % n] = box.f.copy(order="F"), box.rho.copy(order="F"), box.feq.copy(order="F")
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


def record_phases(lib, name, nx, ny, omega, G, seed):
    """One step, the buffers after each phase."""
    f0, u, v = start_state(nx, ny, seed, True)
    box = RefBox(lib, f0, u, v, omega, G)
    out = dict(nx=nx, ny=ny, omega=np.float32(omega), G=np.float32(G), f0=f0, u=u, v=v)
    box.move()
    out["f_move"] = box.f.copy(order="F")
    box.hydro()
    out["rho_hydro"] = box.rho.copy(order="F")
    box.update_feq()
    out["feq_feq"] = box.feq.copy(order="F")
    box.collide()
    out["f_collide"] = box.f.copy(order="F")
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(ref, tmp)
        record_run(lib, "ad_diffusion_37x23", 37, 23, 0.9, 0., False, (1, 10, 200), 11)
        record_run(lib, "ad_advection_37x23", 37, 23, 1.3, 0., True, (1, 10, 200), 12)
        record_run(lib, "ad_fisher_37x23", 37, 23, 1.1, 0.01, True, (1, 200, 1000), 13)
        record_phases(lib, "ad_phases_21x13", 21, 13, 1.2, 0.01, 14)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
