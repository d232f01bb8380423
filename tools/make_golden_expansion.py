#!/usr/bin/env python3
"""Fixtures for noisy strains on a shared nutrient, recorded from the reference's own OpenCL C.

    python tools/make_golden_expansion.py <reference dir>      # -> tests/golden/ex_*.npz

As tools/make_golden_multifield.py and tools/make_golden_noisy.py: a small C driver that #includes the reference's
LB_D2Q9/D2Q9_multifield_diffusion.cl BY PATH behind a handful of #defines, built with gcc (-std=gnu99 -O1 -ffp-contract=off) in a
temporary directory, drives the kernels in the order of advecting_range_expansion/stochastic_nutrients.py's run (:478-496): move ->
copy_buffer -> (move_bcs: pass) -> update_hydro -> update_feq -> collide_particles.  `sqrt` of a float is OpenCL's float32 square root:
the driver maps it to sqrtf.  The reference refills its random_normal buffer between steps from pyopencl's unseeded generator; here the
normals of strain i at step t are the project's stream (tests/noise_model.py: normals32) under the recorded seed of that strain at noise
counter t -- and stored in the fixture, so a test can feed the very same numbers.  Nothing of the reference's text is copied.

The reference's box is the OPEN family.  For the PERIODIC family only the streaming differs, and streaming computes nothing: the tool
rolls the arrays itself and runs the reference's C for update_hydro, update_feq and the collision.

zero_cutoff is a discontinuity: a cell whose post-stream sum f lies closer to the cutoff than the comparison's own rho tolerance can
flip, and no tolerance holds that.  So in every step, member and cell |sum f - zero_cutoff| must exceed contract_tol(n)['rho']
(tests/scalar_model.py; at most 1e-5).  The tool searches start seeds 1, 2, ... and records the first that holds (and that meets the
fixture's own conditions below); it refuses to write if none of the first 64 does.

Files (arrays as the reference's host arrays: float32, F-ordered (nx, ny) / (nx, ny, NP + 1) / (nx, ny, NP + 1, 9), nutrient last).
Every file holds nx, ny, bc, omega[NP], omega_nutrient, G[NP], Dg[NP], seeds[NP] (strain i's stream), zero_cutoff, start_seed, f0, u, v,
edge_zero (1: f_streamed starts as zeros, which is what the class's all-zero f_temporary amounts to; 0: as a copy of f, lb_set_f's
convention) and z (steps, nx, ny, NP).
  ex_run_open_37x23, ex_run_periodic_37x23   50 steps (f_n, rho_n for n in steps = 1, 10, 50), NP = 2, non-uniform u, v <= 0.07.
                        Every density stays >= 2 zero_cutoff, so no threshold is near, and in every step the Milstein term moves some
                        link by more than 10 x the f tolerance.
  ex_front_21x13        OPEN, 8 steps (1, 8), NP = 2, the class's inoculum (well-mixed strains in the first rows, zeros ahead, nutrient
                        everywhere, edge state zero): cells cross the cutoff.
  ex_three_5x4, ex_one_3x3   OPEN, 7 steps (1, 7), NP = 3 and NP = 1: the smallest lanes.
  ex_phases_21x13       one step, the buffers after each phase, from groups of cells that decide each branch clearly: sum f = cutoff / 2
                        and 2 cutoff in a strain, NaN in f, links whose new value is clearly negative (the fixture's own z: in [-5, -4]
                        there, at rho = 2 cutoff), the nutrient below the cutoff; zeroed = the links the reference set to 0; z_is_stream
                        = the cells whose normals are the stream's own (all but those given that z).  Every link's new value is
                        clear of 0 before the floor.
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
from make_golden_multifield import CS, CX, CY, GOLDEN, W       # noqa: E402
from noise_model import normals32                               # noqa: E402
from scalar_model import contract_tol                           # noqa: E402



def largest_other_fixture():
    """A new fixture is to be no larger than the largest one the suite already has."""
    return max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if not f.startswith("ex_"))


DRIVER = r"""
#include <math.h>
#include <stdbool.h>
static int g_gid[3];
#define __kernel
#define __global
#define __constant const
#define __read_only
#define __write_only
#define sqrt(x) sqrtf(x)
static inline int get_global_id(int d) { return g_gid[d]; }
#include "%(cl)s"

#define RANGE(CALL)                                              \
    for (g_gid[1] = 0; g_gid[1] < ny; ++g_gid[1])                \
        for (g_gid[0] = 0; g_gid[0] < nx; ++g_gid[0]) { CALL; }

void drv_move(float *f, float *fs, const int *cx, const int *cy, int nx, int ny, int np)
{
    RANGE(move(f, fs, cx, cy, nx, ny, np))
    RANGE(copy_buffer(fs, f, nx, ny, np))
}
void drv_hydro(float *f, float *u, float *v, float *rho, int nx, int ny, int np, float cut) { RANGE(update_hydro(f, u, v, rho, nx, ny, np, cut)) }
void drv_feq(float *feq, float *rho, float *u, float *v, const float *w, const int *cx, const int *cy, float cs, int nx, int ny, int np, float cut)
{
    RANGE(update_feq(feq, rho, u, v, w, cx, cy, cs, nx, ny, np, cut))
}
void drv_collide(float *f, float *feq, float *rho, float *normal, const float *omega, const float *G, const float *Dg, float omega_n,
                 const float *w, int nx, int ny, int np, float cut)
{
    RANGE(collide_particles(f, feq, rho, normal, omega, G, Dg, omega_n, w, nx, ny, np, cut))
}
"""


def build_driver(ref, tmp):
    cl = os.path.join(os.path.abspath(ref), "LB_D2Q9", "D2Q9_multifield_diffusion.cl")
    if not os.path.exists(cl):
        raise SystemExit("%s not found" % cl)
    src, so = os.path.join(tmp, "drv.c"), os.path.join(tmp, "drv.so")
    open(src, "w").write(DRIVER % {"cl": cl})
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-w", src, "-o", so, "-lm"])
    return ct.CDLL(so)


class Unclear(Exception):
    """A cell came too close to a threshold, or a fixture's own condition failed: try the next start seed."""


class RefBox(object):
    """The reference's buffers and stochastic_nutrients.py's run loop; periodic: the streaming is a roll made here."""

    def __init__(self, lib, f0, u, v, omega, omega_n, G, Dg, seeds, cut, periodic=False, edge_zero=False):
        self.lib = lib
        self.nx, self.ny, self.nf = f0.shape[:3]
        self.np_ = self.nf - 1
        self.f = np.asfortranarray(f0, dtype=np.float32).copy(order="F")
        self.fs = np.zeros_like(self.f, order="F") if edge_zero else self.f.copy(order="F")
        self.feq = np.zeros_like(self.f, order="F")
        self.rho = np.zeros((self.nx, self.ny, self.nf), np.float32, order="F")
        self.u = np.asfortranarray(u, dtype=np.float32).copy(order="F")
        self.v = np.asfortranarray(v, dtype=np.float32).copy(order="F")
        self.omega, self.G, self.Dg = (np.array(a, np.float32) for a in (omega, G, Dg))
        self.omega_n, self.cut, self.seeds, self.periodic = np.float32(omega_n), np.float32(cut), [int(s) for s in seeds], periodic
        self.t, self.z, self.z_override = 0, [], None
        self.margin = np.inf        # min |sum f - cut| seen behind a streaming step, before the cut

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ct.c_void_p)

    def move(self):
        if self.periodic:
            for k in range(9):
                self.f[:, :, :, k] = np.roll(self.f[:, :, :, k], (CX[k], CY[k]), axis=(0, 1))
            self.fs[...] = self.f
        else:
            self.lib.drv_move(self._p(self.f), self._p(self.fs), self._p(CX), self._p(CY), self.nx, self.ny, self.np_)

    def hydro(self):
        total = self.f[:, :, :, 0].copy()
        for k in range(1, 9):
            total = total + self.f[:, :, :, k]
        with np.errstate(invalid="ignore"):
            gap = np.abs(total.astype(np.float64) - np.float64(self.cut))
        self.margin = min(self.margin, float(np.nanmin(gap)))
        self.lib.drv_hydro(self._p(self.f), self._p(self.u), self._p(self.v), self._p(self.rho), self.nx, self.ny, self.np_, ct.c_float(self.cut))

    def update_feq(self):
        self.lib.drv_feq(self._p(self.feq), self._p(self.rho), self._p(self.u), self._p(self.v), self._p(W), self._p(CX), self._p(CY),
                         ct.c_float(CS), self.nx, self.ny, self.np_, ct.c_float(self.cut))

    def collide(self):
        z = np.zeros((self.nx, self.ny, self.np_), np.float32, order="F")
        for i in range(self.np_):
            z[:, :, i] = normals32(self.nx, self.ny, self.seeds[i], self.t)
        if self.z_override is not None:
            z = np.asfortranarray(self.z_override(z))
        self.z.append(z)
        self.t += 1
        self.lib.drv_collide(self._p(self.f), self._p(self.feq), self._p(self.rho), self._p(z), self._p(self.omega), self._p(self.G),
                             self._p(self.Dg), ct.c_float(self.omega_n), self._p(W), self.nx, self.ny, self.np_, ct.c_float(self.cut))

    def step(self):
        self.move()
        self.hydro()
        self.update_feq()
        self.collide()


def flow(nx, ny):
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    u = 0.07 * np.sin(2. * np.pi * y / ny + 0.3) * np.cos(np.pi * x / nx)
    v = 0.07 * np.cos(2. * np.pi * x / nx) * np.sin(np.pi * (y + 0.5) / ny)
    return np.asfortranarray(u.astype(np.float32)), np.asfortranarray(v.astype(np.float32))


def blobs(nx, ny, n_strains, seed, noise=0.02):
    """Strains as blobs in [0.15, 0.55], the nutrient in [0.7, 1.0], a little noise on the populations."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    f0 = np.zeros((nx, ny, n_strains + 1, 9), np.float32, order="F")
    for i in range(n_strains + 1):
        cxi, cyi = (0.25 + 0.5 * i / max(1, n_strains)) * nx, (0.6 - 0.25 * (i % 2)) * ny
        bump = np.exp(-(((x - cxi) / (0.3 * nx + 1.)) ** 2 + ((y - cyi) / (0.35 * ny + 1.)) ** 2))
        rho = 0.7 + 0.3 * bump if i == n_strains else 0.15 + 0.4 * bump
        f0[:, :, i, :] = (W[None, None, :] * rho[:, :, None] * (1. + noise * rng.uniform(-1., 1., (nx, ny, 9)))).astype(np.float32)
    return f0


def inoculum(nx, ny, n_strains, depth, rho_amp=1., concentration_amp=1.):
    """stochastic_nutrients.py's init_hydro and init_f: well-mixed strains in rows y < depth, zeros ahead, nutrient everywhere."""
    rho = np.zeros((nx, ny, n_strains + 1), np.float32, order="F")
    rho[:, :depth, :n_strains] = rho_amp / n_strains
    rho[:, :, n_strains] = concentration_amp
    return np.asfortranarray((W[None, None, None, :] * rho[:, :, :, None]).astype(np.float32))


def header(box, bc, f0, start_seed, edge_zero):
    return dict(nx=box.nx, ny=box.ny, bc=np.array(bc), omega=box.omega, omega_nutrient=box.omega_n, G=box.G, Dg=box.Dg,
                seeds=np.array(box.seeds, np.uint64), zero_cutoff=box.cut, start_seed=np.int32(start_seed), f0=f0, u=box.u, v=box.v,
                edge_zero=np.int32(edge_zero))


def save(name, out):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("%s: %d bytes" % (path, size))
    assert size <= largest_other_fixture(), "fixture too large"


def search(name, attempt):
    for start_seed in range(1, 65):
        try:
            out = attempt(start_seed)
        except Unclear as e:
            print("%s: start seed %d: %s" % (name, start_seed, e))
            continue
        print("%s: start seed %d" % (name, start_seed))
        return save(name, out)
    raise SystemExit("%s: none of the start seeds 1..64 keeps every cell clear of the cutoff: not written" % name)


def run_and_record(box, out, steps, check_step=None):
    for n in range(1, max(steps) + 1):
        box.margin = np.inf
        box.step()
        if not box.margin > contract_tol(n)["rho"]:
            raise Unclear("step %d: a cell has |sum f - zero_cutoff| = %.2e" % (n, box.margin))
        if check_step:
            check_step(n)
        if n in steps:
            out["f_%d" % n], out["rho_%d" % n] = box.f.copy(order="F"), box.rho.copy(order="F")
    out["steps"] = np.array(steps, np.int32)
    out["z"] = np.stack(box.z)


def record_run(lib, name, nx, ny, periodic, steps=(1, 10, 50)):
    omega, omega_n, G, Dg, cut = (1.1, 0.9), 1.3, (0.01, 0.014), (2.0e-3, 1.0e-3), 0.01
    u, v = flow(nx, ny)

    def attempt(start_seed):
        f0 = blobs(nx, ny, 2, start_seed)
        box = RefBox(lib, f0, u, v, omega, omega_n, G, Dg, (100 * start_seed, 100 * start_seed + 1), cut, periodic)

        def check_step(n):
            if not (float(box.rho.min()) >= 2. * cut and np.isfinite(box.f).all() and (box.f > 0).all()):
                raise Unclear("step %d: a density fell below 2 zero_cutoff (min %.4f) or a link was set to 0" % (n, float(box.rho.min())))
            z, c = box.z[-1].astype(np.float64), box.rho[:, :, 2].astype(np.float64)
            mil = max(float(np.max(np.abs(W[0] * (box.Dg[i] * c / 4.) * (z[:, :, i] ** 2 - 1.)))) for i in range(2))
            if not mil > 10. * contract_tol(n)["f"]:
                raise Unclear("step %d: the Milstein term moves no link by more than 10 x the f tolerance (%.2e)" % (n, mil))

        out = header(box, "periodic" if periodic else "open", f0, start_seed, False)
        run_and_record(box, out, steps, check_step)
        return out

    search(name, attempt)


def record_small(lib, name, nx, ny, n_strains, steps=(1, 7)):
    omega, G, Dg = (1.05, 0.95, 1.2)[:n_strains], (0.01, 0.015, 0.012)[:n_strains], (1.0e-3, 2.0e-3, 5.0e-4)[:n_strains]
    u, v = flow(nx, ny)

    def attempt(start_seed):
        f0 = blobs(nx, ny, n_strains, start_seed)
        box = RefBox(lib, f0, u, v, omega, 1.3, G, Dg, [100 * start_seed + i for i in range(n_strains)], 0.01)
        out = header(box, "open", f0, start_seed, False)
        run_and_record(box, out, steps)
        if not np.isfinite(box.f).all():
            raise Unclear("not finite")
        return out

    search(name, attempt)


def record_front(lib, name, nx, ny, steps=(1, 8)):
    omega, omega_n, G, Dg, cut = (1.0, 1.15), 1.25, (0.02, 0.025), (2.0e-3, 2.0e-3), 0.01
    u, v = np.zeros((nx, ny), np.float32, order="F"), np.full((nx, ny), 0.02, np.float32, order="F")

    def attempt(start_seed):
        f0 = inoculum(nx, ny, 2, 4)
        box = RefBox(lib, f0, u, v, omega, omega_n, G, Dg, (100 * start_seed, 100 * start_seed + 1), cut, edge_zero=True)
        out = header(box, "open", f0, start_seed, True)
        crossed = []

        def check_step(n):
            crossed.append((box.rho[:, :, :2] > 0).sum())

        run_and_record(box, out, steps, check_step)
        if not (np.isfinite(box.f).all() and (box.rho[:, :, :2] == 0).any() and crossed[-1] > crossed[0]):
            raise Unclear("no cell crossed the cutoff")
        print("%s: cells above the cutoff per step: %s" % (name, crossed))
        return out

    search(name, attempt)


def record_phases(lib, name, nx, ny):
    """One step from a start made of columns of cells that decide each branch: x < 4: strain 0 at sum f = cutoff / 2; x < 8: strain 0 at
    2 cutoff with z in [-5, -4], where (sqrt(rho) + sqrt(Dg c) z / 2)^2 < Dg c / 4 - G rho c (clearly negative links); x < 12: NaN in a link of strain 1; x < 16: the nutrient at cutoff / 2; the rest:
    everything well above the cutoff.  u = v = 0 in the first 16 columns keeps streaming from mixing what the groups are made of more
    than the margins below allow; the tool verifies each group did what it is there for."""
    omega, omega_n, G, Dg, cut = (1.2, 0.95), 1.1, (0.01, 0.015), (4.4e-3, 1.0e-3), 0.01
    u, v = flow(nx, ny)
    u[:16], v[:16] = 0., 0.

    def attempt(start_seed):
        rng = np.random.default_rng(start_seed)
        rho = np.zeros((nx, ny, 3))
        rho[:, :, 0], rho[:, :, 1], rho[:, :, 2] = 0.3, 0.25, 0.9
        rho[0:4, :, 0] = 0.5 * cut
        rho[4:8, :, 0] = 2. * cut
        rho[12:16, :, 2] = 0.5 * cut
        rho *= 1. + 0.002 * rng.uniform(-1., 1., rho.shape)
        f0 = np.asfortranarray((W[None, None, None, :] * rho[:, :, :, None]).astype(np.float32))
        f0[9:11, 2:ny - 2, 1, 0] = np.nan           # (the rest link: it stays where it is)
        box = RefBox(lib, f0, u, v, omega, omega_n, G, Dg, (100 * start_seed, 100 * start_seed + 1), cut)

        def z_override(z):
            z = z.copy()
            z[5:7, :, 0] = -4.5 + 0.5 * np.tanh(z[5:7, :, 0])     # in [-5, -4]
            return z

        box.z_override = z_override
        out = header(box, "open", f0, start_seed, False)
        box.move()
        out["f_move"] = box.f.copy(order="F")
        box.hydro()
        out["rho_hydro"] = box.rho.copy(order="F")
        if not box.margin > contract_tol(1)["rho"]:
            raise Unclear("a cell has |sum f - zero_cutoff| = %.2e" % box.margin)
        box.update_feq()
        out["feq_feq"] = box.feq.copy(order="F")
        moved = box.f.astype(np.float64)
        box.collide()
        out["f_collide"], out["z"] = box.f.copy(order="F"), np.stack(box.z)
        zeroed = box.f == 0.
        out["zeroed"] = zeroed
        # the cells whose normals are the stream's own (the rest were given the z above): what a run that draws for itself can be held to
        out["z_is_stream"] = np.stack([box.z[0][:, :, i] == normals32(nx, ny, box.seeds[i], 0) for i in range(2)], axis=2).all(axis=2)
        # `new value < 0` is a threshold as well: every link of a member above the cutoff must be clear of 0 before the floor, in float64
        # from the recorded buffers, by more than 4 x the f tolerance
        D = np.float64
        c, z = box.rho[:, :, 2].astype(D), box.z[0].astype(D)
        react = [box.G[i] * box.rho[:, :, i].astype(D) * c + np.sqrt(box.Dg[i] * box.rho[:, :, i].astype(D) * c) * z[:, :, i]
                 + (box.Dg[i] * c / 4.) * (z[:, :, i] ** 2 - 1.) for i in range(2)]
        react.append(-react[0] - react[1])
        for i, om in enumerate(list(box.omega) + [box.omega_n]):
            new = moved[:, :, i, :] * (1. - D(om)) + D(om) * box.feq[:, :, i, :].astype(D) + W[None, None, :].astype(D) * react[i][:, :, None]
            live = (box.rho[:, :, i] >= cut)[:, :, None] & np.isfinite(new)
            if live.any() and not float(np.abs(new[np.broadcast_to(live, new.shape)]).min()) > 4. * contract_tol(1)["f"]:
                raise Unclear("a link's new value lies within 4 x the f tolerance of 0")
        rho_h = box.rho
        ok = ((rho_h[1:3, :, 0] == 0).all() and zeroed[1:3, :, 0, :].all()                  # strain 0 cut: all nine links 0
              and (rho_h[5:7, :, 0] > 0).all() and zeroed[5:7, 1:-1, 0, :].any(axis=2).all()     # clearly negative links
              and (rho_h[9:11, 2:ny - 2, 1] == 0).all() and zeroed[9:11, 2:ny - 2, 1, :].all()     # NaN: rho cut, links 0
              and (rho_h[13:15, :, 2] == 0).all() and zeroed[13:15, :, 2, :].all()             # the nutrient below the cutoff
              and not zeroed[17:, :, :, :].any() and np.isfinite(box.f).all())
        if not ok:
            raise Unclear("a group did not decide its branch")
        print("%s: %d links set to 0 in %d cells" % (name, zeroed.sum(), zeroed.any(axis=(2, 3)).sum()))
        return out

    search(name, attempt)


def main(ref):
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(ref, tmp)
        record_run(lib, "ex_run_open_37x23", 37, 23, False)
        record_run(lib, "ex_run_periodic_37x23", 37, 23, True)
        record_front(lib, "ex_front_21x13", 21, 13)
        record_small(lib, "ex_three_5x4", 5, 4, 3)
        record_small(lib, "ex_one_3x3", 3, 3, 1)
        record_phases(lib, "ex_phases_21x13", 21, 13)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
