#!/usr/bin/env python3
"""Fixtures for the LB Poisson solver, recorded from the reference's own OpenCL C.

    python tools/make_golden_poisson.py <reference dir>      # -> tests/golden/ps_*.npz

The reference's LB_D2Q9/D2Q9_poisson.cl is plain C apart from the address-space qualifiers and the work-item id built-in.
This tool writes a small C driver into a temporary directory that #includes that file BY PATH behind a handful of
#defines, builds it with gcc (-std=gnu99 -O1 -ffp-contract=off: no fused multiply-add, as an OpenCL compiler without
-cl-mad-enable), and drives the kernels in the order of poisson/solver.py's Poisson_Solver.run: rho_before = rho, move ->
copy_buffer -> move_bcs (over the 3-D range the reference launches it on: nine times) -> update_hydro -> update_feq ->
collide_particles.  Only the recorded arrays are written; the driver and the library built from it live and die in the
temporary directory.  Nothing at test time needs the reference.

Arrays are the reference's host arrays: float32, F-ordered (nx, ny) / (nx, ny, 9)  (flat index k nx ny + y nx + x).
Every run file holds nx, ny, delta_t, delta_x, lb_D, omega, rho_on_boundary, source (as handed to the class),
scaled_source (after update_source), react_factor (delta_t lb_D), f0, steps and, for each n in steps, f_n, rho_n, feq_n:
the buffers as the reference holds them after n iterations.  ps_box_37x23 also holds ratio_iters and ratios: the
reference's convergence ratio mean |rho_before - rho| / mean rho_before of every iteration 2 ... 600, evaluated in
float64 on its float32 arrays.
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
CS = 1. / np.sqrt(3)

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

#define RANGE(nz, CALL)                                          \
    for (g_gid[2] = 0; g_gid[2] < (nz); ++g_gid[2])              \
        for (g_gid[1] = 0; g_gid[1] < ny; ++g_gid[1])            \
            for (g_gid[0] = 0; g_gid[0] < nx; ++g_gid[0]) { CALL; }

void drv_move(float *f, float *fs, const int *cx, const int *cy, int nx, int ny)
{
    RANGE(9, move(f, fs, cx, cy, nx, ny))
    RANGE(9, copy_buffer(fs, f, nx, ny))
}
void drv_move_bcs(float *f, float rho_specified, const float *w, int nx, int ny) { RANGE(9, move_bcs(f, rho_specified, w, nx, ny)) }
void drv_hydro(float *f, float *rho, int nx, int ny) { RANGE(1, update_hydro(f, rho, nx, ny)) }
void drv_feq(float *feq, float *rho, const float *w, int nx, int ny) { RANGE(1, update_feq(feq, rho, w, nx, ny)) }
void drv_collide(float *f, float *feq, float *sources, float omega, const float *w, float delta_t, float D, int nx, int ny)
{
    RANGE(1, collide_particles(f, feq, sources, omega, w, delta_t, D, nx, ny))
}
void drv_gradient(float *rho, float *u, float *v, float delta_x, int nx, int ny) { RANGE(1, update_negative_gradient(rho, u, v, delta_x, nx, ny)) }
"""


def build_driver(ref, tmp):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "D2Q9_poisson.cl")
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    src, so = os.path.join(tmp, "drv.c"), os.path.join(tmp, "drv.so")
    open(src, "w").write(DRIVER % {"cl": cl})
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class RefSolver(object):
    """The reference's buffers, its parameter arithmetic (solver.py:75-83, 143-161) and its run loop."""

    def __init__(self, lib, nx, ny, source, delta_t, delta_x, rho_on_boundary, f0=None):
        self.lib, self.nx, self.ny = lib, nx, ny
        self.delta_x, self.delta_t = np.float32(delta_x), np.float32(delta_t)
        self.lb_D = np.float32(self.delta_t / self.delta_x ** 2)
        self.omega = np.float32((.5 + float(self.lb_D) / CS ** 2) ** -1.)
        self.rho_on_boundary = np.float32(rho_on_boundary)
        self.source = np.asfortranarray(source, dtype=np.float32)
        self.scaled = np.asfortranarray(self.source * np.float32(self.lb_D * self.delta_t))
        self.f = np.zeros((nx, ny, 9), np.float32, order="F") if f0 is None else np.asfortranarray(f0, dtype=np.float32).copy(order="F")
        self.fs = self.f.copy(order="F")                        # init_pop fills f and f_streamed alike
        self.feq = np.zeros_like(self.f, order="F")
        self.rho = np.zeros((nx, ny), np.float32, order="F")
        self.rho_before = self.rho.copy(order="F")
        self.ratio = None

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ct.c_void_p)

    def move(self):
        self.lib.drv_move(self._p(self.f), self._p(self.fs), self._p(CX), self._p(CY), self.nx, self.ny)

    def move_bcs(self):
        self.lib.drv_move_bcs(self._p(self.f), ct.c_float(self.rho_on_boundary), self._p(W), self.nx, self.ny)

    def hydro(self):
        self.lib.drv_hydro(self._p(self.f), self._p(self.rho), self.nx, self.ny)

    def update_feq(self):
        self.lib.drv_feq(self._p(self.feq), self._p(self.rho), self._p(W), self.nx, self.ny)

    def collide(self):
        self.lib.drv_collide(self._p(self.f), self._p(self.feq), self._p(self.scaled), ct.c_float(self.omega), self._p(W),
                             ct.c_float(self.delta_t), ct.c_float(self.lb_D), self.nx, self.ny)

    def iterate(self):
        self.rho_before = self.rho.copy(order="F")
        self.move()
        self.move_bcs()
        self.hydro()
        self.update_feq()
        self.collide()
        d = np.abs(self.rho_before.astype(np.float64) - self.rho.astype(np.float64)).mean()
        with np.errstate(all="ignore"):
            self.ratio = d / self.rho_before.astype(np.float64).mean()

    def header(self):
        return dict(nx=self.nx, ny=self.ny, delta_t=self.delta_t, delta_x=self.delta_x, lb_D=self.lb_D, omega=self.omega,
                    rho_on_boundary=self.rho_on_boundary, source=self.source, scaled_source=self.scaled,
                    react_factor=np.float32(self.delta_t * self.lb_D), f0=self.f.copy(order="F"))


def positive_source(nx, ny, amp=1., base=0.2):
    """a constant plus an off-centre Gaussian"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    s = base + np.exp(-(((x - 0.35 * nx) / (0.15 * nx)) ** 2 + ((y - 0.6 * ny) / (0.2 * ny)) ** 2))
    return np.asfortranarray((amp * s).astype(np.float32))


def noisy_f0(nx, ny, level, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((W[None, None, :] * level * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(np.float32))


def save(name, out):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


def record_run(lib, name, nx, ny, delta_t, delta_x, rho_b, source, f0, steps, ratios_to=0):
    box = RefSolver(lib, nx, ny, source, delta_t, delta_x, rho_b, f0)
    out = box.header()
    out["steps"] = np.array(steps, np.int32)
    iters, ratios = [], []
    for n in range(1, max(max(steps), ratios_to) + 1):
        box.iterate()
        if 2 <= n <= ratios_to:
            iters.append(n)
            ratios.append(box.ratio)
        if n in steps:
            out["f_%d" % n], out["rho_%d" % n], out["feq_%d" % n] = box.f.copy(order="F"), box.rho.copy(order="F"), box.feq.copy(order="F")
    if ratios_to:
        out["ratio_iters"], out["ratios"] = np.array(iters, np.int32), np.array(ratios, np.float64)
    print("%s: omega %.6f, max |rho| at %d: %.4f" % (name, box.omega, max(steps), np.abs(out["rho_%d" % max(steps)]).max()))
    save(name, out)
    return out


def record_phases(lib, name, nx, ny, delta_t, delta_x, rho_b, seed):
    """One iteration, the buffers after each phase."""
    box = RefSolver(lib, nx, ny, positive_source(nx, ny, 0.01), delta_t, delta_x, rho_b, noisy_f0(nx, ny, 0.3, seed))
    out = box.header()
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


def record_gradient(lib, name, rho, delta_x):
    nx, ny = rho.shape
    rho = np.asfortranarray(rho, dtype=np.float32)
    u, v = np.zeros_like(rho, order="F"), np.zeros_like(rho, order="F")
    p = lambda a: a.ctypes.data_as(ct.c_void_p)
    lib.drv_gradient(p(rho), p(u), p(v), ct.c_float(delta_x), nx, ny)
    save(name, dict(nx=nx, ny=ny, delta_x=np.float32(delta_x), rho=rho, u=u, v=v))


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(ref, tmp)
        # the zero lattice and a positive source, scaled (the scheme is linear in it) so that max |rho| at the last recorded
        # iteration is about 0.5.  The constant part decides where between two iterations the ratio crosses 1e-4: with 0.15 the
        # ratios of the last iteration above and the first below are 1.3 % and 1.2 % away from it (tests/test_poisson_cpu.py
        # asks for more than 1 %, so that no float32 summation order can move the stop); 0.2 gave 0.65 % and 1.9 %.
        base = 0.15
        probe = RefSolver(lib, 37, 23, positive_source(37, 23, 1., base), 0.5, 1., 0.)
        for _ in range(200):
            probe.iterate()
        amp = 0.5 / float(np.abs(probe.rho).max())
        record_run(lib, "ps_box_37x23", 37, 23, 0.5, 1., 0., positive_source(37, 23, amp, base), None, (1, 10, 200), ratios_to=600)
        record_run(lib, "ps_noise_37x23", 37, 23, 1., 1., 0.3, positive_source(37, 23, 0.004), noisy_f0(37, 23, 0.3, 21), (1, 10, 200))
        record_run(lib, "ps_box_5x4", 5, 4, 0.5, 1., 0.2, positive_source(5, 4, 0.02), noisy_f0(5, 4, 0.25, 22), (1, 7))
        record_phases(lib, "ps_phases_21x13", 21, 13, 1., 1., 0.3, 23)
        g = RefSolver(lib, 21, 13, positive_source(21, 13, 0.01), 0.5, 1., 0.1, noisy_f0(21, 13, 0.3, 24))
        for _ in range(20):
            g.iterate()
        record_gradient(lib, "ps_grad_21x13", g.rho, 1.)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
