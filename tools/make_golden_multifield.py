#!/usr/bin/env python3
"""Fixtures for coupled scalar lattices, recorded from the reference's own OpenCL C.

    python tools/make_golden_multifield.py <reference dir>      # -> tests/golden/mf_*.npz

The reference's LB_D2Q9/D2Q9_multifield_fisher.cl is plain C apart from the address-space qualifiers, `bool` and the work-item
id built-in.  As tools/make_golden_scalar.py does for the Diffusion classes, this tool writes a small C driver into a
temporary directory that #includes that file BY PATH behind a handful of #defines (and <stdbool.h>), builds it with gcc
(-std=gnu99 -O1 -ffp-contract=off: no fused multiply-add, as an OpenCL compiler without -cl-mad-enable) and drives the
kernels in the order of advecting_range_expansion/deterministic_fisher_waves.py's Fisher_Expansion.run:
move -> copy_buffer -> move_bcs -> update_hydro -> update_feq -> collide_particles.  Only the recorded arrays are written;
the driver and the library built from it live and die in the temporary directory.  Nothing at test time needs the reference.

Arrays are the reference's host arrays: float32, F-ordered (nx, ny) / (nx, ny, nf) / (nx, ny, nf, 9)
(flat index k nf nx ny + i nx ny + y nx + x).  f_streamed starts as a copy of f, the engine's convention (lb_set_f);
corner_zero = 1 marks the case that starts with zeros in the eight never-written corner links of every field instead, which
is what the class's all-zero f_temporary amounts to.
Every run file holds nx, ny, omega[nf], G[nf], f0, u, v, corner_zero, steps and, for each n in steps, f_n and rho_n: the
buffers as the reference holds them after n iterations (rho is that of the last iteration's update_hydro; feq follows from
rho, u, v and is recorded in the phase file only, to keep the files small).
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
CS = np.float32(1. / np.sqrt(3.))          # np.float32(cs), deterministic_fisher_waves.py:27
# the eight corner links the push `move` never writes and move_bcs skips: (k, x, y), x / y = 0 or -1; the ABI's order
CORNER_LINKS = ((6, 0, 0), (8, 0, 0), (5, -1, 0), (7, -1, 0), (5, 0, -1), (7, 0, -1), (6, -1, -1), (8, -1, -1))

DRIVER = r"""
#include <math.h>
#include <stdbool.h>
static int g_gid[3];
#define __kernel
#define __global
#define __constant const
#define __read_only
#define __write_only
static inline int get_global_id(int d) { return g_gid[d]; }
#include "%(cl)s"

#define RANGE(CALL)                                              \
    for (g_gid[1] = 0; g_gid[1] < ny; ++g_gid[1])                \
        for (g_gid[0] = 0; g_gid[0] < nx; ++g_gid[0]) { CALL; }

void drv_move(float *f, float *fs, const int *cx, const int *cy, int nx, int ny, int nf)
{
    RANGE(move(f, fs, cx, cy, nx, ny, nf))
    RANGE(copy_buffer(fs, f, nx, ny, nf))
}
void drv_move_bcs(float *f, const float *w, int nx, int ny, int nf) { RANGE(move_bcs(f, w, nx, ny, nf)) }
void drv_hydro(float *f, float *u, float *v, float *rho, int nx, int ny, int nf) { RANGE(update_hydro(f, u, v, rho, nx, ny, nf)) }
void drv_feq(float *feq, float *rho, float *u, float *v, const float *w, const int *cx, const int *cy, float cs, int nx, int ny, int nf)
{
    RANGE(update_feq(feq, rho, u, v, w, cx, cy, cs, nx, ny, nf))
}
void drv_collide(float *f, float *feq, float *rho, const float *omega, const float *G, const float *w, int nx, int ny, int nf)
{
    RANGE(collide_particles(f, feq, rho, omega, G, w, nx, ny, nf))
}
"""


def build_driver(ref, tmp):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "D2Q9_multifield_fisher.cl")
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    src, so = os.path.join(tmp, "drv.c"), os.path.join(tmp, "drv.so")
    open(src, "w").write(DRIVER % {"cl": cl})
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class RefBox(object):
    """The reference's buffers and its run loop."""

    def __init__(self, lib, f0, u, v, omega, G, corner_zero=False):
        self.lib = lib
        self.nx, self.ny, self.nf = f0.shape[:3]
        self.f = np.asfortranarray(f0, dtype=np.float32).copy(order="F")
        self.fs = self.f.copy(order="F")
        if corner_zero:
            for k, x, y in CORNER_LINKS:
                self.fs[x, y, :, k] = 0.
        self.feq = np.zeros_like(self.f, order="F")
        self.rho = np.zeros((self.nx, self.ny, self.nf), np.float32, order="F")
        self.u = np.asfortranarray(u, dtype=np.float32).copy(order="F")
        self.v = np.asfortranarray(v, dtype=np.float32).copy(order="F")
        self.omega, self.G = np.array(omega, np.float32), np.array(G, np.float32)

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ct.c_void_p)

    def move(self):
        self.lib.drv_move(self._p(self.f), self._p(self.fs), self._p(CX), self._p(CY), self.nx, self.ny, self.nf)

    def move_bcs(self):
        self.lib.drv_move_bcs(self._p(self.f), self._p(W), self.nx, self.ny, self.nf)

    def hydro(self):
        self.lib.drv_hydro(self._p(self.f), self._p(self.u), self._p(self.v), self._p(self.rho), self.nx, self.ny, self.nf)

    def update_feq(self):
        self.lib.drv_feq(self._p(self.feq), self._p(self.rho), self._p(self.u), self._p(self.v), self._p(W), self._p(CX),
                         self._p(CY), ct.c_float(CS), self.nx, self.ny, self.nf)

    def collide(self):
        self.lib.drv_collide(self._p(self.f), self._p(self.feq), self._p(self.rho), self._p(self.omega), self._p(self.G),
                             self._p(W), self.nx, self.ny, self.nf)

    def run(self, n):
        for _ in range(n):
            self.move()
            self.move_bcs()
            self.hydro()
            self.update_feq()
            self.collide()


def start_state(nx, ny, nf, seed, flow):
    """Blobs of concentration, one per field, sum of rho < 1 everywhere, 5 % noise on the populations; flow: a non-uniform
    imposed field, |u|, |v| <= 0.07."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    f0 = np.zeros((nx, ny, nf, 9), np.float32, order="F")
    for i in range(nf):
        cxi, cyi = (0.25 + 0.5 * i / max(1, nf - 1)) * nx, (0.6 - 0.25 * (i % 2)) * ny
        rho = 0.02 + (0.75 / nf) * np.exp(-(((x - cxi) / (0.25 * nx)) ** 2 + ((y - cyi) / (0.3 * ny)) ** 2))
        f0[:, :, i, :] = (W[None, None, :] * rho[:, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(np.float32)
    if flow:
        u = 0.07 * np.sin(2. * np.pi * y / ny + 0.3) * np.cos(np.pi * x / nx)
        v = 0.07 * np.cos(2. * np.pi * x / nx) * np.sin(np.pi * (y + 0.5) / ny)
    else:
        u, v = np.zeros((nx, ny)), np.zeros((nx, ny))
    assert float(f0.sum(axis=(2, 3)).max()) < 1.
    return f0, np.asfortranarray(u.astype(np.float32)), np.asfortranarray(v.astype(np.float32))


def save(name, out):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


def header(nx, ny, omega, G, f0, u, v, corner_zero):
    return dict(nx=nx, ny=ny, omega=np.array(omega, np.float32), G=np.array(G, np.float32), f0=f0, u=u, v=v,
                corner_zero=np.int32(corner_zero))


def record_run(lib, name, nx, ny, omega, G, flow, steps, seed, corner_zero=False):
    f0, u, v = start_state(nx, ny, len(omega), seed, flow)
    box = RefBox(lib, f0, u, v, omega, G, corner_zero)
    out = header(nx, ny, omega, G, f0, u, v, corner_zero)
    out["steps"] = np.array(steps, np.int32)
    done = 0
    for n in steps:
        box.run(n - done)
        done = n
        out["f_%d" % n], out["rho_%d" % n] = box.f.copy(order="F"), box.rho.copy(order="F")
    save(name, out)


def record_phases(lib, name, nx, ny, omega, G, seed):
    """One step, the buffers after each phase."""
    f0, u, v = start_state(nx, ny, len(omega), seed, True)
    box = RefBox(lib, f0, u, v, omega, G)
    out = header(nx, ny, omega, G, f0, u, v, False)
    box.move()
    out["f_move"] = box.f.copy(order="F")
    box.move_bcs()
    out["f_bcs"] = box.f.copy(order="F")
    box.hydro()
    out["rho_hydro"] = box.rho.copy(order="F")
    box.update_feq()
    out["feq_feq"] = box.feq.copy(order="F")
    box.collide()
    out["f_collide"] = box.f.copy(order="F")
    save(name, out)


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(ref, tmp)
        record_run(lib, "mf_box_37x23", 37, 23, (0.9, 1.3, 1.1), (0.01, 0.02, 0.), True, (1, 10, 200), 21)
        record_run(lib, "mf_fisher_37x23", 37, 23, (1.0, 1.2), (0.01, 0.012), False, (1, 200, 1000), 22, corner_zero=True)
        record_run(lib, "mf_box_5x4", 5, 4, (0.85, 1.35), (0.01, 0.02), True, (1, 7), 23)
        record_phases(lib, "mf_phases_21x13", 21, 13, (1.2, 0.95), (0.01, 0.015), 24)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
