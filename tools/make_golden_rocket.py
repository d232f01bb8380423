#!/usr/bin/env python3
"""Fixtures for surfactant-propelled colonies, recorded from the reference's own OpenCL C.

    python tools/make_golden_rocket.py <reference dir>      # -> tests/golden/ry_*.npz

The reference's LB_D2Q9/rocket_yeast/rocket_yeast.cl and rocket_yeast_forces_only.cl are plain C apart from the address-space
qualifiers and the work-item built-ins.  This tool writes a small C driver into a temporary directory that #includes one of
them BY PATH behind a handful of #defines, builds it with gcc (-std=gnu99 -O1 -ffp-contract=off) TWICE -- as written (float32;
`exp` and `pow`, which OpenCL resolves by argument type, mapped to expf and powf) and with `#define float double` in front of the
include -- and drives the kernels in the order of Rocket_Yeast.run (rocket_yeast.py:469-483) / Rocket_Yeast_Forces_Only.run:
move_periodic -> copy -> update_hydro / update_rho -> [flow: update_u_and_v -> update_psi -> update_pseudo_force | forces:
update_surf_tension -> update_surface_forces -> update_pressure_force -> update_u_and_v] -> update_feq -> collide_particles.
Only the recorded arrays are written; the drivers and the libraries built from them live and die in the temporary directory.
Nothing at test time needs the reference.

The three stencil kernels load a tile into local memory cooperatively, between two barriers: run one work-item at a time they
would read a half-filled tile.  The driver gives get_local_id / get_local_size real values (4 x 4 groups, 6 x 6 tiles) and runs
every work-item of a group -- those outside the grid too -- TWICE over the same tile: after the first pass the tile is complete,
and what the second pass writes is the kernel's.  The reference allocates psi and the pseudo-force as (ny, ny), which its
kernels overrun when nx > ny; the driver allocates (nx, ny) buffers of its own.

A fixture is refused unless, at every recorded step, the float32 build is within the project's parity contract
(tests/scalar_model.py: contract_tol) of the float64 build in f, rho, u, v and within the bounds that follow from rho's through
the stencil in psi / S and the forces (tests/rocket_model.py: rocket_bounds); the phase fixtures also unless at least 1 % of
the population's links are floored at 0 in their collision, the same links in both builds.  The measured gaps are printed.

Arrays are the reference's host arrays: F-ordered (nx, ny, 2) / (nx, ny, 2, 9), population first; u, v, op (psi / S), Fx, Fy (the
pseudo-force / the pressure force), Sx, Sy (the surface force, mode 'forces') (nx, ny).  Every file holds nx, ny, mode, omega (2),
params (G, G_c, epsilon, rho_o, G_chen, c_o, alpha: lb units, float32 values), f0.  A run file: steps and, for each n in steps,
rho_n, u_n, v_n, op_n, Fx_n, Fy_n [, Sx_n, Sy_n] -- those of step n before its collision -- and the same names with _f32
appended; f_n at the first and the last step, f_n_f32 at the last.  A phase file: <array>_after_<stage> [_f32] for the arrays each
stage writes, and clamped: the (nx, ny, 9) mask of the population links the collision floored.
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
from rocket_model import CS32, PARAMS, rocket_bounds  # noqa: E402
from scalar_model import contract_tol  # noqa: E402

W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1], dtype=np.int32)
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1], dtype=np.int32)

PRELUDE = r"""
#include <math.h>
#include <stdlib.h>
#include <string.h>
static int g_gid[3], g_lid[3];
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
/* whole work-groups with real local ids, every group twice (the tile is complete after the first pass) */
#define GROUPS(CALL)                                                                         \
    for (int by = 0; by < ny; by += GROUP)                                                   \
        for (int bx = 0; bx < nx; bx += GROUP)                                               \
            for (int pass = 0; pass < 2; ++pass)                                             \
                for (g_lid[1] = 0; g_lid[1] < GROUP; ++g_lid[1])                             \
                    for (g_lid[0] = 0; g_lid[0] < GROUP; ++g_lid[0]) {                       \
                        g_gid[0] = bx + g_lid[0];                                            \
                        g_gid[1] = by + g_lid[1];                                            \
                        CALL;                                                                \
                    }
static float tile[(GROUP + 2) * (GROUP + 2)];

void drv_move(float *f, float *fs, const int *cx, const int *cy, int nx, int ny)
{
    RANGE(move_periodic(f, fs, cx, cy, nx, ny, 2))
    memcpy(f, fs, sizeof(float) * 18 * (size_t)nx * ny);
}
void drv_feq(float *feq, float *rho, float *u, float *v, const float *w, const int *cx, const int *cy, const float *par, int nx, int ny)
{
    RANGE(update_feq(feq, rho, u, v, w, cx, cy, par[0], nx, ny, 2))
}
"""

# par: cs, omega, omega_c, G, Gc, epsilon, rho_o, G_chen, c_o, alpha
FLOW = r"""
void drv_hydro(float *f, float *u, float *v, float *rho, int nx, int ny) { RANGE(update_hydro(f, u, v, rho, nx, ny, 2)) }
void drv_velocity(float *rho, float *u, float *v, const float *par, const int *cx, const int *cy, const float *w, int nx, int ny)
{
    GROUPS(update_u_and_v(rho, u, v, 1, par[0], par[5], cx, cy, w, tile, nx, ny, GROUP + 2, GROUP + 2, 1))
}
void drv_forces(float *rho, float *op, float *Fx, float *Fy, float *Sx, float *Sy, const float *par, const int *cx, const int *cy,
                const float *w, int nx, int ny)
{
    (void)Sx; (void)Sy;
    RANGE(update_psi(op, rho, par[6], nx, ny, 0))
    GROUPS(update_pseudo_force(op, Fx, Fy, par[7], par[0], cx, cy, w, tile, nx, ny, GROUP + 2, GROUP + 2, 1))
}
void drv_collide(float *f, float *feq, float *rho, float *Fx, float *Fy, const float *par, const float *w, const int *cx, const int *cy,
                 int nx, int ny)
{
    RANGE(collide_particles(f, feq, rho, par[1], par[2], par[3], par[4], Fx, Fy, w, cx, cy, par[0], nx, ny, 2))
}
"""

FORCES = r"""
void drv_hydro(float *f, float *u, float *v, float *rho, int nx, int ny) { (void)u; (void)v; RANGE(update_rho(f, rho, nx, ny, 2)) }
void drv_velocity(float *rho, float *u, float *v, float *Fx, float *Fy, float *Sx, float *Sy, int nx, int ny)
{
    (void)rho;
    RANGE(update_u_and_v(u, v, Fx, Fy, Sx, Sy, nx, ny, 2))
}
void drv_forces(float *rho, float *op, float *Fx, float *Fy, float *Sx, float *Sy, const float *par, const int *cx, const int *cy,
                const float *w, int nx, int ny)
{
    RANGE(update_surf_tension(op, rho, par[8], par[9], nx, ny, 1))
    GROUPS(update_surface_forces(op, Sx, Sy, 1, par[0], par[5], cx, cy, w, tile, nx, ny, GROUP + 2, GROUP + 2, 1))
    GROUPS(update_pressure_force(rho, 0, Fx, Fy, par[7], par[6], par[0], cx, cy, w, tile, nx, ny, GROUP + 2, GROUP + 2, 1))
}
void drv_collide(float *f, float *feq, float *rho, float *Fx, float *Fy, const float *par, const float *w, const int *cx, const int *cy,
                 int nx, int ny)
{
    (void)Fx; (void)Fy; (void)cx; (void)cy;
    RANGE(collide_particles(f, feq, rho, par[1], par[2], par[3], par[4], w, nx, ny, 2))
}
"""

CL = {"flow": "rocket_yeast.cl", "forces": "rocket_yeast_forces_only.cl"}


def build_driver(ref, tmp, mode, dtype):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "rocket_yeast", CL[mode])
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    tag = "%s_%s" % (mode, "f32" if dtype == np.float32 else "f64")
    src, so = os.path.join(tmp, "drv_%s.c" % tag), os.path.join(tmp, "drv_%s.so" % tag)
    real = "#define exp(x) expf(x)\n#define pow(x, y) powf(x, y)" if dtype == np.float32 else "#define float double"
    open(src, "w").write(PRELUDE % {"cl": cl, "real": real} + (FLOW if mode == "flow" else FORCES))
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class RefColony(object):
    """The reference's buffers ((nx, ny) ones where it allocates (ny, ny)) and its run loop."""

    def __init__(self, lib, dtype, nx, ny, mode, omega, omega_c, params):
        T = self.T = dtype
        self.lib, self.nx, self.ny, self.mode = lib, nx, ny, mode
        self.omega = np.array([np.float32(omega), np.float32(omega_c)], np.float32)
        self.params = {k: np.float32(params[k]) for k in PARAMS}
        p = self.params
        self.par = np.array([CS32, self.omega[0], self.omega[1], p["G"], p["G_c"], p["epsilon"], p["rho_o"], p["G_chen"], p["c_o"], p["alpha"]], T)
        self.w = W.astype(T)
        z2, z3, z4 = (lambda: np.zeros((nx, ny), T, order="F")), (lambda: np.zeros((nx, ny, 2), T, order="F")), (lambda: np.zeros((nx, ny, 2, 9), T, order="F"))
        self.f, self.fs, self.feq, self.rho = z4(), z4(), z4(), z3()
        self.u, self.v, self.op, self.Fx, self.Fy, self.Sx, self.Sy = z2(), z2(), z2(), z2(), z2(), z2(), z2()
        self.clamped = None

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ct.c_void_p)

    def set_f(self, f0):
        self.f = np.asfortranarray(f0, dtype=self.T).copy(order="F")
        self.fs = self.f.copy(order="F")

    def move(self):
        self.lib.drv_move(self._p(self.f), self._p(self.fs), self._p(CX), self._p(CY), self.nx, self.ny)

    def update_hydro(self):
        self.lib.drv_hydro(self._p(self.f), self._p(self.u), self._p(self.v), self._p(self.rho), self.nx, self.ny)

    def update_velocity(self):
        if self.mode == "flow":
            self.lib.drv_velocity(self._p(self.rho), self._p(self.u), self._p(self.v), self._p(self.par), self._p(CX), self._p(CY),
                                  self._p(self.w), self.nx, self.ny)
        else:
            self.lib.drv_velocity(self._p(self.rho), self._p(self.u), self._p(self.v), self._p(self.Fx), self._p(self.Fy),
                                  self._p(self.Sx), self._p(self.Sy), self.nx, self.ny)

    def update_forces(self):
        self.lib.drv_forces(self._p(self.rho), self._p(self.op), self._p(self.Fx), self._p(self.Fy), self._p(self.Sx), self._p(self.Sy),
                            self._p(self.par), self._p(CX), self._p(CY), self._p(self.w), self.nx, self.ny)

    def update_feq(self):
        self.lib.drv_feq(self._p(self.feq), self._p(self.rho), self._p(self.u), self._p(self.v), self._p(self.w), self._p(CX), self._p(CY),
                         self._p(self.par), self.nx, self.ny)

    def collide(self):
        self.lib.drv_collide(self._p(self.f), self._p(self.feq), self._p(self.rho), self._p(self.Fx), self._p(self.Fy), self._p(self.par),
                             self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)
        # (the floor writes +0: a link at exactly 0 behind a collision with growth or a force was floored)
        self.clamped = np.ascontiguousarray(self.f[:, :, 0, :] == 0)

    @property
    def STAGES(self):
        third = ("update_velocity", "update_forces") if self.mode == "flow" else ("update_forces", "update_velocity")
        return ("move", "update_hydro") + third + ("update_feq", "collide")

    def step(self):
        for name in self.STAGES:
            getattr(self, name)()

    def state(self):
        d = dict(f=self.f, rho=self.rho, u=self.u, v=self.v, op=self.op, Fx=self.Fx, Fy=self.Fy)
        if self.mode == "forces":
            d.update(Sx=self.Sx, Sy=self.Sy)
        return d


def lb_constants(mode, N, time_prefactor=1., epsilon=1., Dc=1., Gc=2., rho_o=1., G_chen=-1., c_o=0.25, alpha=2.):
    """omega, omega_c and the float32 parameters as the two classes derive them (rocket_yeast.py:84-142; the forces-only class rounds
    delta_x and delta_t to float32 on the way).  A float32 scalar combined with a Python float is a float64 there."""
    f32, f64 = np.float32, np.float64
    cs2 = f64(CS32) ** 2                            # cs ** 2: a float32 scalar and a Python int
    delta_x = 1. / N
    if mode == "forces":
        delta_x = f64(f32(delta_x))
    delta_t = time_prefactor * delta_x ** 2
    if mode == "forces":
        delta_t = f64(f32(delta_t))
    lb_D = f32(0.25 * (delta_t / delta_x ** 2))
    omega = f32((.5 + f64(lb_D) / cs2) ** -1.)
    lb_G = f32(1. * delta_t)
    lb_Dc = f32(0.25 * f64(f32(Dc)) * (delta_t / delta_x ** 2))
    omega_c = f32((.5 + f64(lb_Dc) / cs2) ** -1.)
    lb_Gc = f32(f64(f32(Gc)) * delta_t)
    params = dict(G=lb_G, G_c=lb_Gc, epsilon=np.float32(epsilon), rho_o=np.float32(rho_o), G_chen=np.float32(G_chen),
                  c_o=np.float32(c_o), alpha=np.float32(alpha))
    return omega, omega_c, params


def droplet_f0(nx, ny, N, R0, seed):
    """init_hydro's noisy droplet at equilibrium (u = v = 0, no surfactant): f0 = w rho, rounded to float32"""
    rng = np.random.default_rng(seed)
    X, Y = np.meshgrid((np.arange(nx) - nx // 2) / float(N), (np.arange(ny) - ny // 2) / float(N), indexing="ij")
    rho = np.zeros((nx, ny, 2), np.float32)
    rho[:, :, 0] = 1.0 * np.exp(-(X ** 2 + Y ** 2) / R0 ** 2) * (1 + .05 * rng.standard_normal((nx, ny)))
    return np.asfortranarray((W[None, None, None, :] * rho[:, :, :, None].astype(np.float64)).astype(np.float32))


def rough_f0(nx, ny, seed):
    """w rho_i (1 +- 5 %), rho_p uniform in [0.2, 1.4], rho_c in [0, 1], rounded to float32"""
    rng = np.random.default_rng(seed)
    rho = np.stack([rng.uniform(0.2, 1.4, (nx, ny)), rng.uniform(0., 1., (nx, ny))], axis=2)
    return np.asfortranarray((W[None, None, None, :] * rho[:, :, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 2, 9)))).astype(np.float32))


def save(name, out):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(GOLDEN, n)) for n in os.listdir(GOLDEN) if not n.startswith("ry_"))
    print("%s: %d bytes" % (path, size))
    if size > largest:
        os.remove(path)
        raise SystemExit("%s: %d bytes, more than the largest other fixture (%d): not kept" % (name, size, largest))


def accept(name, n, b64, b32, which=None):
    """The conditions under which a fixture is written (module docstring).  Returns the largest fraction of a bound used."""
    s64, s32 = b64.state(), b32.state()
    tol = contract_tol(n)
    rb = rocket_bounds(b64.mode, b64.params, float(s64["rho"].max()), tol["rho"])
    bound = dict(f=tol["f"], rho=tol["rho"], u=tol["u"], v=tol["v"], op=rb["op"], Fx=rb["F"], Fy=rb["F"], Sx=rb["S"], Sy=rb["S"])
    worst, where = 0., ""
    for k in (which or s64):
        d = float(np.abs(s64[k] - s32[k].astype(np.float64)).max())
        frac = d / bound[k] if bound[k] > 0 else (0. if d == 0 else np.inf)
        if frac > worst:
            worst, where = frac, k
        if not d <= bound[k]:
            raise SystemExit("%s: step %d: the reference's float32 build is %.3g from its float64 build in %s (bound %.3g): not written" % (name, n, d, k, bound[k]))
    if not np.isfinite(s64["f"]).all():
        raise SystemExit("%s: step %d: not finite: not written" % (name, n))
    print("  %s step %d: float32 build at %.2f of its bound (%s); max rho %.3f %.3f, max |u| %.4f"
          % (name, n, worst, where, s64["rho"][:, :, 0].max(), s64["rho"][:, :, 1].max(), np.sqrt(s64["u"] ** 2 + s64["v"] ** 2).max()))
    return worst


def header(b, f0):
    return dict(nx=b.nx, ny=b.ny, mode=np.array(b.mode), omega=b.omega.astype(np.float64),
                params=np.array([b.params[k] for k in PARAMS], np.float64), f0=np.asfortranarray(f0))


def pair(libs, mode, nx, ny, omega, omega_c, params):
    return (RefColony(libs[mode, np.float64], np.float64, nx, ny, mode, omega, omega_c, params),
            RefColony(libs[mode, np.float32], np.float32, nx, ny, mode, omega, omega_c, params))


def record_run(libs, name, mode, nx, ny, N, steps, seed):
    omega, omega_c, params = lb_constants(mode, N)
    b64, b32 = pair(libs, mode, nx, ny, omega, omega_c, params)
    f0 = droplet_f0(nx, ny, N, 1., seed)
    out = header(b64, f0)
    out["steps"] = np.array(steps, np.int32)
    for b in (b64, b32):
        b.set_f(f0)
    for n in range(1, max(steps) + 1):
        for b in (b64, b32):
            # (the fields of step n BEFORE its collision and f behind it: what a run of n steps leaves)
            b.step()
        if n in steps:
            accept(name, n, b64, b32)
            s64, s32 = b64.state(), b32.state()
            for k in s64:
                if k == "f" and n not in (min(steps), max(steps)):
                    continue
                out["%s_%d" % (k, n)] = s64[k].copy(order="F")
                if k != "f" or n == max(steps):
                    out["%s_%d_f32" % (k, n)] = s32[k].copy(order="F")
    save(name, out)


def writes(mode, stage):
    if stage == "update_forces":
        return ("op", "Fx", "Fy") + (("Sx", "Sy") if mode == "forces" else ())
    return dict(move=("f",), update_hydro=("rho",), update_velocity=("u", "v"), update_feq=("feq",), collide=("f",))[stage]


def record_phases(libs, name, mode, nx, ny, seed):
    """One step from a rough state with epsilon = 2, the buffers after every stage; the collision floors >= 1 % of the population's
    links, the same ones in both builds."""
    omega, omega_c, params = lb_constants(mode, 10, epsilon=2.)
    b64, b32 = pair(libs, mode, nx, ny, omega, omega_c, params)
    f0 = rough_f0(nx, ny, seed)
    out = header(b64, f0)
    for b, tag in ((b64, ""), (b32, "_f32")):
        b.set_f(f0)
        for stage in b.STAGES:
            getattr(b, stage)()
            for k in writes(mode, stage):
                a = b.feq if k == "feq" else b.state()[k]
                out["%s_after_%s%s" % (k, stage, tag)] = a.copy(order="F")
    accept(name, 1, b64, b32)
    d = float(np.abs(b64.feq - b32.feq.astype(np.float64)).max())
    if not d <= contract_tol(1)["f"]:
        raise SystemExit("%s: feq: %.3g: not written" % (name, d))
    n_links, n_clamped = b64.clamped.size, int(b64.clamped.sum())
    if not (np.array_equal(b64.clamped, b32.clamped) and n_clamped >= 0.01 * n_links):
        raise SystemExit("%s: %d of %d links floored (float32 build: %d): not written" % (name, n_clamped, n_links, int(b32.clamped.sum())))
    print("  %s: %d of %d population links floored at 0 (%.1f %%), the same in both builds" % (name, n_clamped, n_links, 100. * n_clamped / n_links))
    out["clamped"] = b64.clamped
    save(name, out)


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        libs = {(mode, T): build_driver(ref, tmp, mode, T) for mode in ("flow", "forces") for T in (np.float64, np.float32)}
        record_run(libs, "ry_flow_37x23", "flow", 37, 23, 10, (1, 10, 50, 100), 61)
        record_run(libs, "ry_forces_37x23", "forces", 37, 23, 10, (1, 10, 50, 100), 62)
        record_run(libs, "ry_flow_5x4", "flow", 5, 4, 4, (1, 10), 63)
        record_run(libs, "ry_flow_3x3", "flow", 3, 3, 3, (1, 10), 64)
        record_phases(libs, "ry_phases_21x13", "flow", 21, 13, 65)
        record_phases(libs, "ry_forces_phases_21x13", "forces", 21, 13, 66)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
