#!/usr/bin/env python3
"""Fixtures for multicomponent Shan-Chen fluids, recorded from the reference's own OpenCL C.

    python tools/make_golden_multifluid.py <reference dir>      # -> tests/golden/mc_*.npz

The reference's LB_D2Q9/multicomponent_multiphase/multi.cl is plain C apart from the address-space qualifiers and the work-item
built-ins.  This tool writes a small C driver into a temporary directory that #includes that file BY PATH behind a handful of
#defines, builds it with gcc (-std=gnu99 -O1 -ffp-contract=off) TWICE -- as it stands (float64, what the reference runs) and
with `#define double float` in front of the include (the reference's own float32 statement) -- and drives the kernels in the
order of multi.py's Simulation_Runner.run: per fluid move[_periodic] -> copy_streamed_onto_f, per fluid move_open_bcs, per
fluid update_hydro_fluid, Gx, Gy = 0 -> the additional forces -> update_bary_velocity -> per fluid update_feq_fluid -> per
fluid collide_particles_fluid -> the additional collisions.  Only the recorded arrays are written; the driver and the
libraries built from it live and die in the temporary directory.  Nothing at test time needs the reference.

add_interaction_force loads a tile of rho into local memory cooperatively, between two barriers: run one work-item at a time
it would read a half-filled tile.  The driver gives get_local_id / get_local_size real values (4 x 4 groups, 6 x 6 tiles) and
runs every work-item of a group -- those outside the grid too -- TWICE over the same tiles, restoring Gx, Gy to their state
before the group in between: after the first pass the tiles are complete, and the second pass's increments are the kernel's.

A fixture is refused unless, at every recorded step, the float32 build is within the project's parity contract
(tests/scalar_model.py: contract_tol) of the float64 build in f, feq, rho, u, v, u_b, within the bound that follows from rho's
through the stencil in Gx, Gy (tests/multifluid_model.py: force_bound), min rho > 0.5 and max |u_b| < 0.15: the bounds the tests
hold this project to are then conditions the reference itself satisfies.  The measured gaps are printed.

Arrays are the reference's host arrays: F-ordered (nx, ny, NP) / (nx, ny, NP, 9), u_b and v_b (nx, ny).  Every run file holds
nx, ny, bc, nu, omega (NP), g (NP, 2), interactions (rows fluid_1, fluid_2, G_int, potential 0 linear / 1 shan_chen / 2 pow,
parameter), reactions (rows kind 0 eat / 1 grow, fluid_a, fluid_b, p0, p1, p2 -- eat: rate, cutoff; grow: min, max, rate), f0,
steps and, for each n in steps, f_n, rho_n, u_n, v_n, Gx_n, Gy_n, ub_n, vb_n (and feq_n at the last; mc_sc_open_37x23: f at the last only, no feq, u, v): the float64 build's
buffers after n iterations, and the same names with _f32 appended: the float32 build's (feq left out).  mc_phases_21x13 holds
<array>_after_<stage> for the arrays each stage writes; mc_init_21x13 the buffers after Fluid.initialize of every fluid.
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
from multifluid_model import POTENTIALS, force_bound  # noqa: E402
from scalar_model import contract_tol  # noqa: E402

W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1], dtype=np.int32)
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1], dtype=np.int32)

DRIVER = r"""
#include <math.h>
#include <stdbool.h>
#include <stdlib.h>
#include <string.h>
static int g_gid[3], g_lid[3];
#define cl_khr_fp64 1
#define __kernel
#define __global
#define __constant const
#define __local
#define __read_only
#define __write_only
#define CLK_LOCAL_MEM_FENCE 0
#define GROUP 4
static inline int get_global_id(int d) { return g_gid[d]; }
static inline int get_local_id(int d) { return g_lid[d]; }
static inline int get_local_size(int d) { (void)d; return GROUP; }
static inline void barrier(int f) { (void)f; }
%(real)s
#include "%(cl)s"

#define RANGE(CALL)                                              \
    for (g_gid[1] = 0; g_gid[1] < ny; ++g_gid[1])                \
        for (g_gid[0] = 0; g_gid[0] < nx; ++g_gid[0]) { CALL; }

void drv_move(int periodic, int i, int np, double *f, double *fs, const int *cx, const int *cy, int nx, int ny)
{
    if (periodic) { RANGE(move_periodic(f, fs, cx, cy, nx, ny, i, np, 9)) }
    else { RANGE(move(f, fs, cx, cy, nx, ny, i, np, 9)) }
    RANGE(copy_streamed_onto_f(fs, f, cx, cy, nx, ny, i, np, 9))
}
void drv_move_bcs(int i, int np, double *f, int nx, int ny) { RANGE(move_open_bcs(f, nx, ny, i, np, 9)) }
void drv_hydro(int i, int np, double *f, double *rho, double *u, double *v, double *Gx, double *Gy, const double *w,
               const int *cx, const int *cy, int nx, int ny)
{
    RANGE(update_hydro_fluid(f, rho, u, v, Gx, Gy, w, cx, cy, nx, ny, i, np, 9))
}
void drv_const_force(int i, const double *g, double *Gx, double *Gy, double *rho, int nx, int ny)
{
    RANGE(add_constant_g_force(i, g[0], g[1], Gx, Gy, rho, nx, ny))
}
/* par: G_int, cs, parameter */
void drv_interaction(int f1, int f2, int np, int bc, int potential, const double *par, double *rho, double *Gx, double *Gy,
                     const int *cx, const int *cy, const double *w, int nx, int ny)
{
    double tile1[(GROUP + 2) * (GROUP + 2)], tile2[(GROUP + 2) * (GROUP + 2)];
    const size_t bytes = sizeof(double) * (size_t)np * nx * ny;
    double *sx = malloc(bytes), *sy = malloc(bytes);
    const double parameters[4] = {par[2], 0, 0, 0};
    for (int by = 0; by < ny; by += GROUP)
        for (int bx = 0; bx < nx; bx += GROUP) {
            memcpy(sx, Gx, bytes);
            memcpy(sy, Gy, bytes);
            for (int pass = 0; pass < 2; ++pass) {
                if (pass) { memcpy(Gx, sx, bytes); memcpy(Gy, sy, bytes); }
                for (g_lid[1] = 0; g_lid[1] < GROUP; ++g_lid[1])
                    for (g_lid[0] = 0; g_lid[0] < GROUP; ++g_lid[0]) {
                        g_gid[0] = bx + g_lid[0];
                        g_gid[1] = by + g_lid[1];
                        add_interaction_force(f1, f2, par[0], tile1, tile2, rho, Gx, Gy, par[1], cx, cy, w, nx, ny, GROUP + 2,
                                              GROUP + 2, 1, 9, bc, potential, parameters);
                    }
            }
        }
    free(sx);
    free(sy);
}
void drv_bary(int np, double *ub, double *vb, double *rho, double *f, double *Gx, double *Gy, const double *tau, const double *w,
              const int *cx, const int *cy, int nx, int ny)
{
    RANGE(update_bary_velocity(ub, vb, rho, f, Gx, Gy, tau, w, cx, cy, nx, ny, np, 9))
}
void drv_feq(int i, int np, double *feq, double *rho, double *ub, double *vb, const double *par, const double *w, const int *cx,
             const int *cy, int nx, int ny)
{
    RANGE(update_feq_fluid(feq, rho, ub, vb, w, cx, cy, par[0], nx, ny, i, np, 9))
}
/* par: cs, omega */
void drv_collide(int i, int np, double *f, double *feq, double *rho, double *ub, double *vb, double *Gx, double *Gy,
                 const double *par, const double *w, const int *cx, const int *cy, int nx, int ny)
{
    RANGE(collide_particles_fluid(f, feq, rho, ub, vb, Gx, Gy, par[1], w, cx, cy, nx, ny, i, np, 9, par[0]))
}
/* par: rate, cutoff, cs */
void drv_eat(int a, int b, int np, const double *par, double *f, double *rho, const double *w, const int *cx, const int *cy, int nx, int ny)
{
    RANGE(add_eating_collision(a, b, par[0], par[1], f, rho, w, cx, cy, nx, ny, np, 9, par[2]))
}
/* par: min, max, rate, cs */
void drv_grow(int a, int np, const double *par, double *f, double *rho, const double *w, const int *cx, const int *cy, int nx, int ny)
{
    RANGE(add_growth(a, par[0], par[1], par[2], f, rho, w, cx, cy, nx, ny, np, 9, par[3]))
}
"""


def build_driver(ref, tmp, dtype):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "multicomponent_multiphase", "multi.cl")
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    tag = "f32" if dtype == np.float32 else "f64"
    src, so = os.path.join(tmp, "drv_%s.c" % tag), os.path.join(tmp, "drv_%s.so" % tag)
    open(src, "w").write(DRIVER % {"cl": cl, "real": "#define double float" if dtype == np.float32 else ""})
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class RefFluids(object):
    """The reference's buffers, its parameter arithmetic (multi.py:55-63) and its run loop."""

    def __init__(self, lib, dtype, nx, ny, bc, nus, g=None, interactions=(), reactions=()):
        T = self.T = dtype
        self.lib, self.nx, self.ny, self.bc, self.n = lib, nx, ny, bc, len(nus)
        self.cs = T(1. / np.sqrt(3))
        self.nus = list(nus)
        self.tau = np.array([T(.5 + T(nu) / (self.cs ** 2)) for nu in nus], T)
        self.omega = np.array([T(t ** -1.) for t in self.tau], T)
        self.w = W.astype(T)
        self.g = np.zeros((self.n, 2), T) if g is None else np.array(g, T).reshape(self.n, 2)
        self.interactions, self.reactions = list(interactions), list(reactions)
        n = self.n
        z2, z3, z4 = (lambda: np.zeros((nx, ny), T, order="F")), (lambda: np.zeros((nx, ny, n), T, order="F")), (lambda: np.zeros((nx, ny, n, 9), T, order="F"))
        self.f, self.fs, self.feq = z4(), z4(), z4()
        self.rho, self.u, self.v, self.Gx, self.Gy = z3(), z3(), z3(), z3(), z3()
        self.ub, self.vb = z2(), z2()

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ct.c_void_p)

    def _arr(self, *vals):
        return np.array(vals, self.T)

    def set_f(self, f0):
        self.f = np.asfortranarray(f0, dtype=self.T).copy(order="F")
        self.fs = self.f.copy(order="F")

    def move(self):
        for i in range(self.n):
            self.lib.drv_move(int(self.bc == "periodic"), i, self.n, self._p(self.f), self._p(self.fs), self._p(CX), self._p(CY), self.nx, self.ny)

    def move_bcs(self):
        if self.bc == "zero_gradient":
            for i in range(self.n):
                self.lib.drv_move_bcs(i, self.n, self._p(self.f), self.nx, self.ny)

    def update_hydro(self):
        for i in range(self.n):
            self.lib.drv_hydro(i, self.n, self._p(self.f), self._p(self.rho), self._p(self.u), self._p(self.v), self._p(self.Gx),
                               self._p(self.Gy), self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)

    def forces(self):
        self.Gx[...] = 0
        self.Gy[...] = 0
        for i in range(self.n):
            if self.g[i].any():
                self.lib.drv_const_force(i, self._p(self.g[i].copy()), self._p(self.Gx), self._p(self.Gy), self._p(self.rho), self.nx, self.ny)
        for (i, j, G_int, potential, par) in self.interactions:
            self.lib.drv_interaction(int(i), int(j), self.n, int(self.bc == "zero_gradient"), POTENTIALS.index(potential),
                                     self._p(self._arr(G_int, self.cs, par)), self._p(self.rho), self._p(self.Gx), self._p(self.Gy),
                                     self._p(CX), self._p(CY), self._p(self.w), self.nx, self.ny)

    def update_bary(self):
        self.lib.drv_bary(self.n, self._p(self.ub), self._p(self.vb), self._p(self.rho), self._p(self.f), self._p(self.Gx), self._p(self.Gy),
                          self._p(self.tau), self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)

    def update_feq(self, only=None):
        for i in range(self.n) if only is None else (only,):
            self.lib.drv_feq(i, self.n, self._p(self.feq), self._p(self.rho), self._p(self.ub), self._p(self.vb), self._p(self._arr(self.cs)),
                             self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)

    def collide(self):
        for i in range(self.n):
            self.lib.drv_collide(i, self.n, self._p(self.f), self._p(self.feq), self._p(self.rho), self._p(self.ub), self._p(self.vb),
                                 self._p(self.Gx), self._p(self.Gy), self._p(self._arr(self.cs, self.omega[i])), self._p(self.w),
                                 self._p(CX), self._p(CY), self.nx, self.ny)

    def react(self):
        for r in self.reactions:
            if r[0] == "eat":
                self.lib.drv_eat(int(r[1]), int(r[2]), self.n, self._p(self._arr(r[3], r[4], self.cs)), self._p(self.f), self._p(self.rho),
                                 self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)
            else:
                self.lib.drv_grow(int(r[1]), self.n, self._p(self._arr(r[2], r[3], r[4], self.cs)), self._p(self.f), self._p(self.rho),
                                  self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)

    STAGES = ("move", "move_bcs", "update_hydro", "forces", "update_bary", "update_feq", "collide", "react")

    def step(self):
        for name in self.STAGES:
            getattr(self, name)()

    def initialize(self, i, rho_arr):
        """Fluid.initialize with f_amp = 0, the barycentric velocity set before (multi.py:66-81)."""
        self.rho[:, :, i] = rho_arr
        self.update_feq(only=i)
        self.f[:, :, i, :] = self.feq[:, :, i, :]

    def state(self):
        return dict(f=self.f, feq=self.feq, rho=self.rho, u=self.u, v=self.v, Gx=self.Gx, Gy=self.Gy, ub=self.ub, vb=self.vb)


def noisy_f0(nx, ny, rhos, seed):
    """W rho_i (1 +- 0.05 sin cos)(1 + 0.01 uniform): the waves of neighbouring fluids in antiphase"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    wave = 0.05 * np.sin(2. * np.pi * x / nx) * np.cos(2. * np.pi * y / ny)
    f = np.zeros((nx, ny, len(rhos), 9), order="F")
    for i, r in enumerate(rhos):
        f[:, :, i, :] = W[None, None, :] * (r * (1. + (-1) ** i * wave))[:, :, None] * (1. + 0.01 * rng.uniform(-1., 1., (nx, ny, 9)))
    return f


def save(name, out):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


def accept(name, n, b64, b32):
    """The conditions under which a fixture is written (module docstring).  Returns the largest fraction of a bound used."""
    s64, s32 = b64.state(), b32.state()
    tol = contract_tol(n)
    bound = dict(f=tol["f"], feq=tol["f"], rho=tol["rho"], u=tol["u"], v=tol["v"], ub=tol["u"], vb=tol["v"])
    worst = 0.
    for k, b in bound.items():
        d = float(np.abs(s64[k] - s32[k].astype(np.float64)).max())
        worst = max(worst, d / b)
        if not d <= b:
            raise SystemExit("%s: step %d: the reference's float32 build is %.3g from its float64 build in %s (contract %.3g): not written" % (name, n, d, k, b))
    gb = force_bound(b64.interactions, b64.g, b64.n, float(s64["rho"].max()), tol["rho"])
    gfrac = 0.
    for i in range(b64.n):
        for k in ("Gx", "Gy"):
            d = float(np.abs(s64[k][:, :, i] - s32[k][:, :, i].astype(np.float64)).max())
            gfrac = max(gfrac, d / gb[i] if gb[i] > 0 else (0. if d == 0 else np.inf))
            if not d <= gb[i]:
                raise SystemExit("%s: step %d: the reference's float32 build is %.3g from its float64 build in %s of fluid %d (force_bound %.3g): not written" % (name, n, d, k, i, gb[i]))
    speed = float(np.sqrt(s64["ub"] ** 2 + s64["vb"] ** 2).max())
    if not (s64["rho"].min() > 0.5 and speed < 0.15):
        raise SystemExit("%s: step %d: min rho %.3g, max |u_b| %.3g: not written" % (name, n, s64["rho"].min(), speed))
    print("  %s step %d: float32 build at %.2f of the contract, G at %.3f of force_bound, min rho %.3f, max |u_b| %.4f"
          % (name, n, worst, gfrac, s64["rho"].min(), speed))
    return worst


def tables(box):
    inter = np.array([[i, j, G, POTENTIALS.index(p), par] for (i, j, G, p, par) in box.interactions], np.float64).reshape(-1, 5)
    react = np.array([[0, r[1], r[2], r[3], r[4], 0.] if r[0] == "eat" else [1, r[1], 0, r[2], r[3], r[4]] for r in box.reactions],
                     np.float64).reshape(-1, 6)
    return inter, react


def header(box, f0=None):
    inter, react = tables(box)
    out = dict(nx=box.nx, ny=box.ny, bc=np.array(box.bc), nu=np.array(box.nus, np.float64), omega=box.omega.astype(np.float64),
               g=box.g.astype(np.float64), interactions=inter, reactions=react)
    if f0 is not None:
        out["f0"] = np.asfortranarray(f0)
    return out


def pair(libs, *args, **kwargs):
    return RefFluids(libs[0], np.float64, *args, **kwargs), RefFluids(libs[1], np.float32, *args, **kwargs)


STEPS = (1, 5, 20)


def record_run(libs, name, nx, ny, bc, nus, rhos, seed, light=False, **kw):
    """light: the populations at the last step only and no u, v (the larger box, to stay under the size of the porous fixtures)"""
    b64, b32 = pair(libs, nx, ny, bc, nus, **kw)
    f0 = noisy_f0(nx, ny, rhos, seed)
    b64.set_f(f0)
    b32.set_f(f0)
    out = header(b64, f0)
    out["steps"] = np.array(STEPS, np.int32)
    for n in range(1, max(STEPS) + 1):
        b64.step()
        b32.step()
        if n in STEPS:
            accept(name, n, b64, b32)
            s64, s32 = b64.state(), b32.state()
            for k in s64:
                if k == "feq" and (light or n != max(STEPS)):
                    continue
                if light and (k in ("u", "v") or (k == "f" and n != max(STEPS))):
                    continue
                out["%s_%d" % (k, n)] = s64[k].copy(order="F")
                if k != "feq":
                    out["%s_%d_f32" % (k, n)] = s32[k].copy(order="F")
    save(name, out)


# what each stage writes
WRITES = dict(move=("f",), move_bcs=("f",), update_hydro=("rho", "u", "v"), forces=("Gx", "Gy"), update_bary=("ub", "vb"),
              update_feq=("feq",), collide=("f",), react=("f",))


def record_phases(libs, name, nx, ny, seed):
    """One step of two fluids in the zero-gradient box with a body force, a shan_chen pair force and both reactions: the
    buffers after each of the eight stages."""
    kw = dict(g=[(5e-4, 2e-4), (0., -3e-4)], interactions=[(0, 1, 0.9, "shan_chen", 1.)],
              reactions=[("eat", 0, 1, 1e-3, 0.5), ("grow", 1, 0.5, 1.5, 1e-3)])
    b64, b32 = pair(libs, nx, ny, "zero_gradient", (0.1, 0.2), **kw)
    f0 = noisy_f0(nx, ny, (1., 1.), seed)
    out = header(b64, f0)
    for b, tag in ((b64, ""), (b32, "_f32")):
        b.set_f(f0)
        for stage in RefFluids.STAGES:
            getattr(b, stage)()
            for k in WRITES[stage]:
                out["%s_after_%s%s" % (k, stage, tag)] = b.state()[k].copy(order="F")
    accept(name, 1, b64, b32)
    save(name, out)


def record_init(libs, name, nx, ny, seed):
    """Fluid.initialize(rho_arr, f_amp = 0) of two fluids from given densities and a given barycentric velocity."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    wave = 0.05 * np.sin(2. * np.pi * x / nx) * np.cos(2. * np.pi * y / ny)
    rho = np.stack([1. + wave, 0.8 - wave], axis=2)
    ub, vb = 0.03 * np.cos(2. * np.pi * y / ny) + 0.002 * rng.uniform(-1., 1., (nx, ny)), 0.02 * np.sin(2. * np.pi * x / nx)
    b64, b32 = pair(libs, nx, ny, "periodic", (0.1, 0.2))
    out = header(b64)
    out.update(rho_in=np.asfortranarray(rho), ub_in=np.asfortranarray(ub), vb_in=np.asfortranarray(vb))
    for b, tag in ((b64, ""), (b32, "_f32")):
        b.ub, b.vb = (np.asfortranarray(a, dtype=b.T).copy(order="F") for a in (ub, vb))
        for i in range(2):
            b.initialize(i, rho[:, :, i])
        for k in ("f", "feq", "rho"):
            out["%s%s" % (k, tag)] = b.state()[k].copy(order="F")
    for k in ("f", "feq"):
        d = float(np.abs(out[k] - out[k + "_f32"].astype(np.float64)).max())
        if not d <= contract_tol(1)["f"]:
            raise SystemExit("%s: the reference's float32 build is %.3g from its float64 build in %s: not written" % (name, d, k))
    save(name, out)


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        libs = (build_driver(ref, tmp, np.float64), build_driver(ref, tmp, np.float32))
        # nu = 0.1 / 0.2 / 0.15 (omega = 1.25 / 0.909 / 1.053); never 1/6: omega = 1 wipes the carried f and hides errors
        lin = [(0, 1, 1., "linear", 0.)]
        record_run(libs, "mc_pair_21x13", 21, 13, "periodic", (0.1, 0.2), (1., 1.), 41, interactions=lin)
        record_run(libs, "mc_pair_open_21x13", 21, 13, "zero_gradient", (0.1, 0.2), (1., 1.), 42, interactions=lin, g=[(3e-4, 0.), (0., -2e-4)])
        record_run(libs, "mc_pair_open_5x4", 5, 4, "zero_gradient", (0.1, 0.2), (1., 1.), 43, interactions=lin)
        record_run(libs, "mc_pair_open_3x3", 3, 3, "zero_gradient", (0.1, 0.2), (1., 1.), 44, interactions=lin)
        record_run(libs, "mc_sc_open_37x23", 37, 23, "zero_gradient", (0.1, 0.2), (1., 1.), 45, light=True, interactions=[(0, 1, 0.9, "shan_chen", 1.)])
        record_run(libs, "mc_pow_21x13", 21, 13, "periodic", (0.1, 0.2), (1., 1.), 46, interactions=[(0, 1, 0.8, "pow", 1.5)])
        record_run(libs, "mc_three_21x13", 21, 13, "periodic", (0.1, 0.2, 0.15), (1., 0.9, 0.8), 47,
                   interactions=[(0, 1, 1., "linear", 0.), (0, 2, 0.7, "linear", 0.), (1, 2, 0.5, "shan_chen", 1.), (2, 2, -0.3, "linear", 0.)])
        record_run(libs, "mc_self_21x13", 21, 13, "periodic", (0.1,), (0.7,), 48, interactions=[(0, 0, -1.5, "shan_chen", 1.)])
        record_run(libs, "mc_self_open_21x13", 21, 13, "zero_gradient", (0.2,), (0.7,), 49, interactions=[(0, 0, -2., "shan_chen", 1.)])
        record_run(libs, "mc_react_21x13", 21, 13, "periodic", (0.1, 0.2), (1., 1.), 50, interactions=lin,
                   reactions=[("eat", 0, 1, 1e-3, 0.5), ("grow", 1, 0.5, 1.5, 1e-3)])
        record_phases(libs, "mc_phases_21x13", 21, 13, 51)
        record_init(libs, "mc_init_21x13", 21, 13, 52)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
