#!/usr/bin/env python3
"""Fixtures for a population and its nutrient under a spectral velocity, recorded from the reference's own OpenCL C.

    python tools/make_golden_nutrient.py <reference dir>      # -> tests/golden/sn_*.npz

The reference's LB_D2Q9/reaction_diffusion/surfactant_nutrient_waves.cl is plain C apart from the address-space qualifiers and the
work-item built-ins.  This tool writes a small C driver into a temporary directory that #includes it BY PATH behind a handful of
#defines, builds it with gcc (-std=gnu99 -O1 -ffp-contract=off) TWICE -- as written (float32; `exp`, which OpenCL resolves by
argument type, mapped to expf) and with `#define float double` in front of the include -- and drives the kernels in the order of
Surfactant_Nutrient_Wave.run / Clumpy_Surfactant_Nutrient_Wave.run: move_periodic -> copy -> update_hydro -> [the velocity] ->
[clumpy: update_psi -> update_pseudo_force] -> update_feq -> collide_particles / collide_particles_attraction.  The velocity between
update_hydro and update_feq is tests/spectral_model.py's solve in complex64 / complex128 to match the build, times the float32
scale: the reference's solver is gpyfft and numpy, it has no C to drive.  Only the recorded arrays are written; the drivers and the
libraries built from them live and die in the temporary directory.  Nothing at test time needs the reference.

update_pseudo_force loads a tile into local memory cooperatively, between two barriers: run one work-item at a time it would read a
half-filled tile.  The driver gives get_local_id / get_local_size real values (4 x 4 groups, 6 x 6 tiles) and runs every work-item
of a group -- those outside the grid too -- TWICE over the same tile: after the first pass the tile is complete, and what the second
pass writes is the kernel's.  The reference allocates psi and the pseudo-force as (ny, ny), which its kernels overrun when nx > ny;
the driver allocates (nx, ny) buffers of its own.

A fixture is refused unless, at every recorded step, the float32 build is within the project's parity contract
(tests/scalar_model.py: contract_tol) of the float64 build in f, rho, u, v, within the bounds that follow from rho's through exp and
the stencil in psi and F (tests/nutrient_model.py: nutrient_bounds), and max |u| < 0.15.  The measured gaps are printed.

Arrays are the reference's host arrays: F-ordered (nx, ny, 2) / (nx, ny, 2, 9), population first; u, v, psi, Fx, Fy (nx, ny).  A run
file holds nx, ny, clumpy, omega (2), params (G, scale, rho_o, G_chen, lam: lb units, float32 values), rho0 (the initial densities),
f0 (their equilibrium under the velocity they imply, float64 arithmetic rounded to float32), steps and, for each n in steps, rho_n,
u_n, v_n [, psi_n, Fx_n, Fy_n] -- those of step n before its collision -- and the same names with _f32 appended; f_n at every step,
f_n_f32 at the last.  The phase file holds nx, ny, omega, f0 and, for each variant v in ('plain', 'clumpy'), v_clumpy, v_params and
v_<array>_after_<stage> [_f32] for the arrays each stage writes.
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
from nutrient_model import CS32, PARAMS, NutrientModel, lattice_parameters, nutrient_bounds  # noqa: E402
from scalar_model import contract_tol  # noqa: E402
from spectral_model import noisy_droplet, solve  # noqa: E402

W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1], dtype=np.int32)
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1], dtype=np.int32)
MAX_SPEED = 0.15
LIMIT = 1 << 20         # bytes of a committed file

DRIVER = r"""
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

/* par: cs, omega, omega_n, G, rho_o, G_chen */
void drv_move(float *f, float *fs, const int *cx, const int *cy, int nx, int ny)
{
    RANGE(move_periodic(f, fs, cx, cy, nx, ny, 2))
    memcpy(f, fs, sizeof(float) * 18 * (size_t)nx * ny);
}
void drv_hydro(float *f, float *u, float *v, float *rho, int nx, int ny) { RANGE(update_hydro(f, u, v, rho, nx, ny, 2)) }
void drv_forces(float *rho, float *psi, float *Fx, float *Fy, const float *par, const int *cx, const int *cy, const float *w, int nx, int ny)
{
    RANGE(update_psi(psi, rho, par[4], nx, ny, 0))
    GROUPS(update_pseudo_force(psi, Fx, Fy, par[5], par[0], cx, cy, w, tile, nx, ny, GROUP + 2, GROUP + 2, 1))
}
void drv_feq(float *feq, float *rho, float *u, float *v, const float *w, const int *cx, const int *cy, const float *par, int nx, int ny)
{
    RANGE(update_feq(feq, rho, u, v, w, cx, cy, par[0], nx, ny, 2))
}
void drv_collide(float *f, float *feq, float *rho, const float *par, const float *w, int nx, int ny)
{
    RANGE(collide_particles(f, feq, rho, par[1], par[2], par[3], w, nx, ny, 2))
}
void drv_collide_attraction(float *f, float *feq, float *rho, float *Fx, float *Fy, const float *par, const float *w, const int *cx,
                            const int *cy, int nx, int ny)
{
    RANGE(collide_particles_attraction(f, feq, rho, par[1], par[2], par[3], Fx, Fy, w, cx, cy, par[0], nx, ny, 2))
}
"""


def build_driver(ref, tmp, dtype):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "reaction_diffusion", "surfactant_nutrient_waves.cl")
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    tag = "f32" if dtype == np.float32 else "f64"
    src, so = os.path.join(tmp, "drv_%s.c" % tag), os.path.join(tmp, "drv_%s.so" % tag)
    real = "#define exp(x) expf(x)" if dtype == np.float32 else "#define float double"
    open(src, "w").write(DRIVER % {"cl": cl, "real": real})
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class RefWave(object):
    """The reference's buffers ((nx, ny) ones where it allocates (ny, ny)) and its run loop."""
    STAGES = NutrientModel.STAGES

    def __init__(self, lib, dtype, nx, ny, clumpy, omega, omega_n, params):
        T = self.T = dtype
        self.lib, self.nx, self.ny, self.clumpy = lib, nx, ny, bool(clumpy)
        self.omega = np.array([np.float32(omega), np.float32(omega_n)], np.float32)
        self.params = {k: (float(params[k]) if k == "lam" else np.float32(params[k])) for k in PARAMS}
        p = self.params
        self.par = np.array([CS32, self.omega[0], self.omega[1], p["G"], p["rho_o"], p["G_chen"]], T)
        self.scale = T(p["scale"])
        self.ctype = np.complex64 if T == np.float32 else np.complex128
        self.w = W.astype(T)
        z2, z3, z4 = (lambda: np.zeros((nx, ny), T, order="F")), (lambda: np.zeros((nx, ny, 2), T, order="F")), (lambda: np.zeros((nx, ny, 2, 9), T, order="F"))
        self.f, self.fs, self.feq, self.rho = z4(), z4(), z4(), z3()
        self.u, self.v, self.psi, self.Fx, self.Fy = z2(), z2(), z2(), z2(), z2()

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
        _, xg, yg = solve(self.rho[:, :, 0], self.params["lam"], self.ctype)
        self.u = np.asfortranarray((self.scale * xg.real).astype(self.T))
        self.v = np.asfortranarray((self.scale * yg.real).astype(self.T))

    def update_forces(self):
        if self.clumpy:
            self.lib.drv_forces(self._p(self.rho), self._p(self.psi), self._p(self.Fx), self._p(self.Fy), self._p(self.par), self._p(CX),
                                self._p(CY), self._p(self.w), self.nx, self.ny)

    def update_feq(self):
        self.lib.drv_feq(self._p(self.feq), self._p(self.rho), self._p(self.u), self._p(self.v), self._p(self.w), self._p(CX), self._p(CY),
                         self._p(self.par), self.nx, self.ny)

    def collide(self):
        if self.clumpy:
            self.lib.drv_collide_attraction(self._p(self.f), self._p(self.feq), self._p(self.rho), self._p(self.Fx), self._p(self.Fy),
                                            self._p(self.par), self._p(self.w), self._p(CX), self._p(CY), self.nx, self.ny)
        else:
            self.lib.drv_collide(self._p(self.f), self._p(self.feq), self._p(self.rho), self._p(self.par), self._p(self.w), self.nx, self.ny)

    def step(self):
        for name in self.STAGES:
            getattr(self, name)()

    def state(self):
        d = dict(f=self.f, rho=self.rho, u=self.u, v=self.v)
        if self.clumpy:
            d.update(psi=self.psi, Fx=self.Fx, Fy=self.Fy)
        return d


def save(name, out):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    if size > LIMIT:
        os.remove(path)
        raise SystemExit("%s: %d bytes, more than a committed file may have (%d): not kept" % (name, size, LIMIT))


def accept(name, n, b64, b32):
    """The conditions under which a fixture is written (module docstring); prints the gaps."""
    s64, s32 = b64.state(), b32.state()
    tol = contract_tol(n)
    nb = nutrient_bounds(b64.params, float(s64["rho"][:, :, 0].max()), tol["rho"])
    bound = dict(f=tol["f"], rho=tol["rho"], u=tol["u"], v=tol["v"], psi=nb["psi"], Fx=nb["F"], Fy=nb["F"])
    gaps = []
    for k in s64:
        d = float(np.abs(s64[k] - s32[k].astype(np.float64)).max())
        gaps.append("%s %.2g" % (k, d))
        if not d <= bound[k]:
            raise SystemExit("%s: step %d: the reference's float32 build is %.3g from its float64 build in %s (bound %.3g): not written" % (name, n, d, k, bound[k]))
    speed = float(np.sqrt(s64["u"] ** 2 + s64["v"] ** 2).max())
    if not np.isfinite(s64["f"]).all() or not speed < MAX_SPEED:
        raise SystemExit("%s: step %d: max |u| = %.4f (limit %.2f) or not finite: not written" % (name, n, speed, MAX_SPEED))
    print("  %s step %d: float32 build from float64 build: %s; max |u| %.4f; sum rho %.9g" % (name, n, ", ".join(gaps), speed, s64["rho"].sum()))


def pair(libs, nx, ny, clumpy, omega, omega_n, params):
    return (RefWave(libs[np.float64], np.float64, nx, ny, clumpy, omega, omega_n, params),
            RefWave(libs[np.float32], np.float32, nx, ny, clumpy, omega, omega_n, params))


def case_parameters(Lx, Ly, N, clumpy):
    p = lattice_parameters(Lx, Ly, N, vc=0.5, Dn=0.1)
    params = dict(G=p["lb_G"], scale=p["scale"], rho_o=np.float32(1.), G_chen=np.float32(-1. if clumpy else 0.), lam=1.)
    return p["nx"], p["ny"], p["omega"], p["omega_n"], params


def record_run(libs, name, Lx, Ly, N, clumpy, steps, seed):
    nx, ny, omega, omega_n, params = case_parameters(Lx, Ly, N, clumpy)
    b64, b32 = pair(libs, nx, ny, clumpy, omega, omega_n, params)
    rho0 = np.zeros((nx, ny, 2), np.float32, order="F")
    rho0[:, :, 0] = np.float32(1.2) * noisy_droplet(nx, ny, N, 0.5, seed)
    rho0[:, :, 1] = 1.
    m = NutrientModel(nx, ny, omega, omega_n, clumpy=clumpy, dtype=np.float64, **params)
    m.redo_initial_condition(rho0)
    f0 = np.asfortranarray(m.f.astype(np.float32))
    out = dict(nx=nx, ny=ny, clumpy=int(clumpy), omega=b64.omega.astype(np.float64), params=np.array([float(params[k]) for k in PARAMS], np.float64),
               rho0=rho0, f0=f0, steps=np.array(steps, np.int32))
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
                out["%s_%d" % (k, n)] = s64[k].copy(order="F")
                if k != "f" or n == max(steps):
                    out["%s_%d_f32" % (k, n)] = s32[k].copy(order="F")
    save(name, out)


def writes(stage):
    return dict(move=("f",), update_hydro=("rho",), update_velocity=("u", "v"), update_forces=("psi", "Fx", "Fy"), update_feq=("feq",),
                collide=("f",))[stage]


def record_phases(libs, name, Lx, Ly, N, seed):
    """One step from a rough state, the buffers after every stage, both variants"""
    rng = np.random.default_rng(seed)
    nx, ny = lattice_parameters(Lx, Ly, N)["nx"], lattice_parameters(Lx, Ly, N)["ny"]
    rho = np.stack([rng.uniform(0.2, 1.4, (nx, ny)), rng.uniform(0., 1., (nx, ny))], axis=2)
    f0 = np.asfortranarray((W[None, None, None, :] * rho[:, :, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 2, 9)))).astype(np.float32))
    out = dict(nx=nx, ny=ny, f0=f0)
    for clumpy in (False, True):
        v = "clumpy_" if clumpy else "plain_"
        _, _, omega, omega_n, params = case_parameters(Lx, Ly, N, clumpy)
        b64, b32 = pair(libs, nx, ny, clumpy, omega, omega_n, params)
        out.update({"omega": b64.omega.astype(np.float64), v + "clumpy": int(clumpy), v + "params": np.array([float(params[k]) for k in PARAMS], np.float64)})
        for b, tag in ((b64, ""), (b32, "_f32")):
            b.set_f(f0)
            for stage in b.STAGES:
                getattr(b, stage)()
                if stage == "update_forces" and not clumpy:
                    continue
                for k in writes(stage):
                    a = b.feq if k == "feq" else b.state()[k]
                    out["%s%s_after_%s%s" % (v, k, stage, tag)] = a.copy(order="F")
        accept(name + " " + v[:-1], 1, b64, b32)
        d = float(np.abs(b64.feq - b32.feq.astype(np.float64)).max())
        if not d <= contract_tol(1)["f"]:
            raise SystemExit("%s: feq: %.3g: not written" % (name, d))
    save(name, out)


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        libs = {T: build_driver(ref, tmp, T) for T in (np.float64, np.float32)}
        record_run(libs, "sn_plain_30x18", 3., 1.8, 10, False, (1, 10, 50), 20240611)
        record_run(libs, "sn_clumpy_30x18", 3., 1.8, 10, True, (1, 10, 50), 20240611)
        record_run(libs, "sn_clumpy_5x4", .5, .4, 10, True, (1, 10, 50), 20240611)
        record_run(libs, "sn_clumpy_3x3", .3, .3, 10, True, (1, 10, 50), 20240611)
        record_phases(libs, "sn_phases_20x12", 2., 1.2, 10, 20240612)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
