#!/usr/bin/env python3
"""Fixtures for forced flow in a porous medium, recorded from the reference's own OpenCL C.

    python tools/make_golden_porous.py <reference dir>      # -> tests/golden/pm_*.npz

The reference's LB_D2Q9/porous_media/single_component.cl is plain C apart from the address-space qualifiers and the work-item
built-ins.  This tool writes a small C driver into a temporary directory that #includes that file BY PATH behind a handful of
#defines, builds it with gcc (-std=gnu99 -O1 -ffp-contract=off: no fused multiply-add, as an OpenCL compiler without
-cl-mad-enable) TWICE -- as it stands (float64, what the reference runs) and with `#define double float` in front of the
include (the reference's own float32 statement) -- and drives the kernels in the order of single_component.py's
Simulation_Runner.run with one fluid: move[_periodic] -> copy_streamed_onto_f -> move_open_bcs -> update_hydro_pourous ->
Gx, Gy = 0 -> the additional forces -> update_forces_pourous -> update_bary_velocity -> update_feq_pourous ->
collide_particles_pourous.  Only the recorded arrays are written; the driver and the libraries built from it live and die in
the temporary directory.  Nothing at test time needs the reference.

A fixture is refused unless, at every recorded step, the float32 build is within the project's parity contract
(tests/scalar_model.py: contract_tol) of the float64 build, min rho > 0.5 and max |u| < 0.15: the bounds the tests hold this
project to are then conditions the reference itself satisfies.

Arrays are the reference's host arrays with its one population dropped: F-ordered (nx, ny) / (nx, ny, 9)  (flat index
k nx ny + y nx + x).  Every run file holds nx, ny, bc, nu_e, omega, epsilon, nu_fluid, K, Fe, g (the constant force),
[radial: center_x, center_y, prefactor, scaling, and field_x, field_y = what add_radial_body_force adds], f0, steps and, for
each n in steps, f_n, feq_n, rho_n, u_n, v_n, Gx_n, Gy_n, ub_n, vb_n: the float64 build's buffers after n iterations, and the
same names with _f32 appended: the float32 build's (feq left out).  pm_phases_21x13 holds <array>_after_<stage> for the arrays
each stage writes; pm_init_21x13 the buffers after initialize.
"""
import ctypes as ct
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
from scalar_model import contract_tol  # noqa: E402

W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1], dtype=np.int32)
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1], dtype=np.int32)

DRIVER = r"""
#include <math.h>
#include <stdbool.h>
static int g_gid[3];
#define cl_khr_fp64 1
#define __kernel
#define __global
#define __constant const
#define __local
#define __read_only
#define __write_only
#define CLK_LOCAL_MEM_FENCE 0
static inline int get_global_id(int d) { return g_gid[d]; }
static inline int get_local_id(int d) { (void)d; return 0; }
static inline int get_local_size(int d) { (void)d; return 1; }
static inline void barrier(int f) { (void)f; }
%(real)s
#include "%(cl)s"

#define RANGE(CALL)                                              \
    for (g_gid[1] = 0; g_gid[1] < ny; ++g_gid[1])                \
        for (g_gid[0] = 0; g_gid[0] < nx; ++g_gid[0]) { CALL; }

void drv_move(int periodic, double *f, double *fs, const int *cx, const int *cy, int nx, int ny)
{
    if (periodic) { RANGE(move_periodic(f, fs, cx, cy, nx, ny, 0, 1, 9)) }
    else { RANGE(move(f, fs, cx, cy, nx, ny, 0, 1, 9)) }
    RANGE(copy_streamed_onto_f(fs, f, cx, cy, nx, ny, 0, 1, 9))
}
void drv_move_bcs(double *f, int nx, int ny) { RANGE(move_open_bcs(f, nx, ny, 0, 1, 9)) }
void drv_hydro(double *f, double *rho, double *u, double *v, double *Gx, double *Gy, const double *par, const double *w,
               const int *cx, const int *cy, int nx, int ny)
{
    RANGE(update_hydro_pourous(f, rho, u, v, Gx, Gy, par[0], par[1], par[3], par[2], w, cx, cy, nx, ny, 0, 1, 9))
}
void drv_const_force(const double *g, double *Gx, double *Gy, int nx, int ny) { RANGE(add_constant_body_force(0, g[0], g[1], Gx, Gy, nx, ny)) }
void drv_radial_force(int center_x, int center_y, const double *ps, double *Gx, double *Gy, int nx, int ny)
{
    RANGE(add_radial_body_force(0, center_x, center_y, ps[0], ps[1], Gx, Gy, nx, ny))
}
void drv_forces(double *rho, double *u, double *v, double *Gx, double *Gy, const double *par, int nx, int ny)
{
    RANGE(update_forces_pourous(rho, u, v, Gx, Gy, par[0], par[1], par[3], par[2], nx, ny, 0, 1))
}
void drv_bary(double *ub, double *vb, double *rho, double *f, double *Gx, double *Gy, const double *tau, const double *w,
              const int *cx, const int *cy, int nx, int ny)
{
    RANGE(update_bary_velocity(ub, vb, rho, f, Gx, Gy, tau, w, cx, cy, nx, ny, 1, 9))
}
void drv_feq(double *feq, double *rho, double *ub, double *vb, const double *par, const double *w, const int *cx, const int *cy,
             int nx, int ny)
{
    RANGE(update_feq_pourous(feq, rho, ub, vb, par[0], w, cx, cy, par[5], nx, ny, 0, 1, 9))
}
void drv_collide(double *f, double *feq, double *rho, double *ub, double *vb, double *Gx, double *Gy, const double *par,
                 const double *w, const int *cx, const int *cy, int nx, int ny)
{
    RANGE(collide_particles_pourous(f, feq, rho, ub, vb, Gx, Gy, par[0], par[4], w, cx, cy, nx, ny, 0, 1, 9, par[5]))
}
"""


def build_driver(ref, tmp, dtype):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "porous_media", "single_component.cl")
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    tag = "f32" if dtype == np.float32 else "f64"
    src, so = os.path.join(tmp, "drv_%s.c" % tag), os.path.join(tmp, "drv_%s.so" % tag)
    open(src, "w").write(DRIVER % {"cl": cl, "real": "#define double float" if dtype == np.float32 else ""})
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class RefFluid(object):
    """The reference's buffers with one population, its parameter arithmetic (single_component.py:55-66) and its run loop."""

    def __init__(self, lib, dtype, nx, ny, bc, nu_e, epsilon, nu_fluid, K, Fe, g=(0., 0.), radial=None):
        T = self.T = dtype
        self.lib, self.nx, self.ny, self.bc = lib, nx, ny, bc
        cs = T(1. / np.sqrt(3))
        tau = T(.5 + T(nu_e) / (cs ** 2))
        self.omega = T(tau ** -1.)
        self.tau = np.array([tau], T)
        # (epsilon, nu_fluid, K, Fe, omega, cs)
        self.par = np.array([epsilon, nu_fluid, K, Fe, self.omega, cs], T)
        self.w = W.astype(T)
        self.g = np.array(g, T)
        self.radial = radial
        z2, z3 = (lambda: np.zeros((nx, ny), T, order="F")), (lambda: np.zeros((nx, ny, 9), T, order="F"))
        self.f, self.fs, self.feq = z3(), z3(), z3()
        self.rho, self.u, self.v, self.Gx, self.Gy, self.ub, self.vb = z2(), z2(), z2(), z2(), z2(), z2(), z2()

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ct.c_void_p)

    def set_f(self, f0):
        self.f = np.asfortranarray(f0, dtype=self.T).copy(order="F")
        self.fs = self.f.copy(order="F")

    def move(self):
        self.lib.drv_move(int(self.bc == "periodic"), self._p(self.f), self._p(self.fs), self._p(CX), self._p(CY), self.nx, self.ny)

    def move_bcs(self):
        if self.bc == "zero_gradient":
            self.lib.drv_move_bcs(self._p(self.f), self.nx, self.ny)

    def update_hydro(self):
        self.lib.drv_hydro(self._p(self.f), self._p(self.rho), self._p(self.u), self._p(self.v), self._p(self.Gx), self._p(self.Gy),
                           self._p(self.par), self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)

    def body_force(self):
        self.Gx[...] = 0
        self.Gy[...] = 0
        self.lib.drv_const_force(self._p(self.g), self._p(self.Gx), self._p(self.Gy), self.nx, self.ny)
        if self.radial:
            cx, cy, pref, scal = self.radial
            self.lib.drv_radial_force(int(cx), int(cy), self._p(np.array([pref, scal], self.T)), self._p(self.Gx), self._p(self.Gy), self.nx, self.ny)

    def update_forces(self):
        self.lib.drv_forces(self._p(self.rho), self._p(self.u), self._p(self.v), self._p(self.Gx), self._p(self.Gy), self._p(self.par),
                            self.nx, self.ny)

    def update_bary(self):
        self.lib.drv_bary(self._p(self.ub), self._p(self.vb), self._p(self.rho), self._p(self.f), self._p(self.Gx), self._p(self.Gy),
                          self._p(self.tau), self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)

    def update_feq(self):
        self.lib.drv_feq(self._p(self.feq), self._p(self.rho), self._p(self.ub), self._p(self.vb), self._p(self.par), self._p(self.w),
                         self._p(CX), self._p(CY), self.nx, self.ny)

    def collide(self):
        self.lib.drv_collide(self._p(self.f), self._p(self.feq), self._p(self.rho), self._p(self.ub), self._p(self.vb), self._p(self.Gx),
                             self._p(self.Gy), self._p(self.par), self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)

    STAGES = ("move", "move_bcs", "update_hydro", "body_force", "update_forces", "update_bary", "update_feq", "collide")

    def step(self):
        for name in self.STAGES:
            getattr(self, name)()

    def initialize(self, rho_arr, ub, vb):
        """Pourous_Media.initialize with f_amp = 0, the barycentric velocity set before (single_component.py:70-89)."""
        self.ub, self.vb = (np.asfortranarray(a, dtype=self.T).copy(order="F") for a in (ub, vb))
        self.rho = np.asfortranarray(rho_arr, dtype=self.T).copy(order="F")
        self.update_feq()
        self.f = self.feq.copy(order="F")
        self.update_hydro()
        self.update_forces()

    def state(self):
        return dict(f=self.f, feq=self.feq, rho=self.rho, u=self.u, v=self.v, Gx=self.Gx, Gy=self.Gy, ub=self.ub, vb=self.vb)


def noisy_f0(nx, ny, seed, rho0=1.):
    """W rho0 (1 + 0.01 uniform) under a +-5 % density wave"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    wave = 1. + 0.05 * np.sin(2. * np.pi * x / nx) * np.cos(2. * np.pi * y / ny)
    return np.asfortranarray(W[None, None, :] * (rho0 * wave)[:, :, None] * (1. + 0.01 * rng.uniform(-1., 1., (nx, ny, 9))))


def save(name, out):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


def accept(name, n, s64, s32):
    """The conditions under which a fixture is written (module docstring)."""
    tol = contract_tol(n)
    bound = dict(f=tol["f"], feq=tol["f"], rho=tol["rho"], u=tol["u"], v=tol["v"], ub=tol["u"], vb=tol["v"])
    for k, b in bound.items():
        d = float(np.abs(s64[k] - s32[k].astype(np.float64)).max())
        if not d <= b:
            raise SystemExit("%s: step %d: the reference's float32 build is %.3g from its float64 build in %s (contract %.3g): not written" % (name, n, d, k, b))
    speed = float(np.sqrt(s64["u"] ** 2 + s64["v"] ** 2).max())
    if not (s64["rho"].min() > 0.5 and speed < 0.15):
        raise SystemExit("%s: step %d: min rho %.3g, max |u| %.3g: not written" % (name, n, s64["rho"].min(), speed))


def header(box, nu_e, f0):
    out = dict(nx=box.nx, ny=box.ny, bc=np.array(box.bc), nu_e=np.float64(nu_e), omega=np.float64(box.omega), epsilon=box.par[0],
               nu_fluid=box.par[1], K=box.par[2], Fe=box.par[3], g=box.g.copy(), f0=np.asfortranarray(f0))
    if box.radial:
        out["radial"] = np.array(box.radial, np.float64)
        probe = RefFluid(box.lib, box.T, box.nx, box.ny, box.bc, nu_e, 1., 0., 1., 0., (0., 0.), box.radial)
        probe.body_force()
        out["field_x"], out["field_y"] = probe.Gx.copy(order="F"), probe.Gy.copy(order="F")
    return out


def pair(libs, *args, **kwargs):
    return RefFluid(libs[0], np.float64, *args, **kwargs), RefFluid(libs[1], np.float32, *args, **kwargs)


def record_run(libs, name, nx, ny, bc, nu_e, epsilon, nu_fluid, K, Fe, g, seed, steps, radial=None):
    b64, b32 = pair(libs, nx, ny, bc, nu_e, epsilon, nu_fluid, K, Fe, g, radial)
    f0 = noisy_f0(nx, ny, seed)
    b64.set_f(f0)
    b32.set_f(f0)
    out = header(b64, nu_e, f0)
    out["steps"] = np.array(steps, np.int32)
    for n in range(1, max(steps) + 1):
        b64.step()
        b32.step()
        if n in steps:
            s64, s32 = b64.state(), b32.state()
            accept(name, n, s64, s32)
            for k in s64:
                out["%s_%d" % (k, n)] = s64[k].copy(order="F")
                if k != "feq":
                    out["%s_%d_f32" % (k, n)] = s32[k].copy(order="F")
    print("%s: omega %.6f, max |u| at %d: %.4g" % (name, b64.omega, max(steps), np.abs(b64.u).max()))
    save(name, out)


# what each stage writes
WRITES = dict(move=("f",), move_bcs=("f",), update_hydro=("rho", "u", "v"), body_force=("Gx", "Gy"), update_forces=("Gx", "Gy"),
              update_bary=("ub", "vb"), update_feq=("feq",), collide=("f",))


def record_phases(libs, name, nx, ny, seed):
    """One step in the zero-gradient box with a radial force, the buffers after each of the eight stages."""
    args = (nx, ny, "zero_gradient", 0.1, 0.8, 0.15, 30., 0.3, (5e-4, 2e-4), (nx // 2, ny // 2, 1e-5, 1.))
    b64, b32 = pair(libs, *args)
    f0 = noisy_f0(nx, ny, seed)
    out = header(b64, 0.1, f0)
    for b, tag in ((b64, ""), (b32, "_f32")):
        b.set_f(f0)
        for stage in RefFluid.STAGES:
            getattr(b, stage)()
            for k in WRITES[stage]:
                out["%s_after_%s%s" % (k, stage, tag)] = b.state()[k].copy(order="F")
    accept(name, 1, b64.state(), b32.state())
    save(name, out)


def record_init(libs, name, nx, ny, seed):
    """Pourous_Media.initialize(rho_arr, f_amp = 0) from a given rho and barycentric velocity."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    rho = 1. + 0.05 * np.sin(2. * np.pi * x / nx) * np.cos(2. * np.pi * y / ny)
    ub, vb = 0.03 * np.cos(2. * np.pi * y / ny) + 0.002 * rng.uniform(-1., 1., (nx, ny)), 0.02 * np.sin(2. * np.pi * x / nx)
    b64, b32 = pair(libs, nx, ny, "periodic", 0.1, 0.7, 1. / 6., 50., 0.2)
    out = header(b64, 0.1, np.zeros((nx, ny, 9)))
    del out["f0"]
    out.update(rho_in=np.asfortranarray(rho), ub_in=np.asfortranarray(ub), vb_in=np.asfortranarray(vb))
    for b, tag in ((b64, ""), (b32, "_f32")):
        b.initialize(rho, ub, vb)
        for k, a in b.state().items():
            out["%s%s" % (k, tag)] = a.copy(order="F")
    accept(name, 1, b64.state(), b32.state())
    save(name, out)


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        libs = (build_driver(ref, tmp, np.float64), build_driver(ref, tmp, np.float32))
        steps = (1, 10, 200)
        # nu_e = 0.1 (omega = 1.25) and 0.3 (omega = 0.714); never 1/6: omega = 1 wipes the carried f and hides errors
        record_run(libs, "pm_darcy_37x23", 37, 23, "periodic", 0.1, 0.7, 1. / 6., 50., 0., (1e-4, 0.), 31, steps)
        record_run(libs, "pm_forch_37x23", 37, 23, "periodic", 0.3, 0.5, 0.1, 20., 1.75 / np.sqrt(150. * 0.5 ** 3), (2e-3, -1e-3), 32, steps)
        record_run(libs, "pm_open_37x23", 37, 23, "zero_gradient", 0.1, 0.8, 0.15, 30., 0.3, (5e-4, 2e-4), 33, steps)
        record_run(libs, "pm_open_5x4", 5, 4, "zero_gradient", 0.3, 0.8, 0.15, 30., 0.3, (5e-4, 2e-4), 34, steps)
        record_run(libs, "pm_open_3x3", 3, 3, "zero_gradient", 0.1, 0.8, 0.15, 30., 0.3, (5e-4, 2e-4), 35, steps)
        record_run(libs, "pm_radial_21x13", 21, 13, "zero_gradient", 0.3, 0.8, 0.15, 30., 0.3, (0., 0.), 36, steps, radial=(10, 6, 1e-4, 1.))
        record_phases(libs, "pm_phases_21x13", 21, 13, 37)
        record_init(libs, "pm_init_21x13", 21, 13, 38)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
