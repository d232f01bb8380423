"""The noisy collision without a GPU: known answers of Philox4x32-10 for the numpy model (tests/noise_model.py) and for csrc/philox.h
compiled into a host program, the model against the fixtures recorded from the reference's C (tests/golden/nf_*.npz), the class's
parameter arithmetic, the new ABI symbols."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
from noise_model import NoisyScalarModel, normals32, normals64, philox4x32_10, uniform
from scalar_model import contract_tol

# (counter, key) -> words: the Random123 known answers for Philox4x32-10
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

PHILOX_DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "philox.h"
int main(int argc, char **argv)     /* six hex words per case: c0 c1 c2 c3 k0 k1 */
{
    for (int i = 1; i + 5 < argc; i += 6) {
        uint32_t a[6], r[4];
        for (int j = 0; j < 6; ++j) a[j] = (uint32_t)strtoul(argv[i + j], NULL, 16);
        philox4x32_10(a[0], a[1], a[2], a[3], a[4], a[5], r);
        printf("%08x %08x %08x %08x\n", r[0], r[1], r[2], r[3]);
    }
    uint32_t r[4];
    philox_lane_words(0x0123456789abcdefULL, 9, 5, 0x100000002ULL, r);     /* lane 2 of row 5 */
    printf("%08x %08x %08x %08x\n", r[0], r[1], r[2], r[3]);
    printf("%.9g %.9g\n", philox_uniform(0u), philox_uniform(0xffffffffu));
    return 0;
}
"""


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@pytest.mark.parametrize("counter, key, words", KNOWN)
def test_model_philox_known_answers(counter, key, words):
    assert tuple(int(x) for x in philox4x32_10(counter, key)) == words


@pytest.fixture(scope="module")
def philox_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    d = tmp_path_factory.mktemp("philox")
    (d / "drv.cpp").write_text(PHILOX_DRIVER)
    exe = str(d / "drv")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "2d-lb_amd", "csrc"), str(d / "drv.cpp"), "-o", exe])
    return exe


def run_cases(exe, cases):
    args = ["%08x" % w for c, k in cases for w in tuple(c) + tuple(k)]
    out = subprocess.check_output([exe] + args).decode().splitlines()
    return [tuple(int(w, 16) for w in line.split()) for line in out[:len(cases)]], out[len(cases):]


def test_header_philox_known_answers(philox_exe):
    got, _ = run_cases(philox_exe, [(c, k) for c, k, _ in KNOWN])
    assert got == [w for _, _, w in KNOWN]


def test_header_philox_equals_the_model_on_64_cases(philox_exe):
    rng = np.random.default_rng(2024)
    cases = [(tuple(int(x) for x in rng.integers(0, 2 ** 32, 4)), tuple(int(x) for x in rng.integers(0, 2 ** 32, 2))) for _ in range(60)]
    cases += [((0xffffffff,) * 4, (0xffffffff,) * 2), ((1, 0, 0, 0), (0, 0)), ((0, 0, 0, 1), (0, 1)), ((0, 0, 0xffffffff, 0), (1, 0))]
    assert len(cases) == 64
    got, rest = run_cases(philox_exe, cases)
    want = [tuple(int(x) for x in philox4x32_10(c, k)) for c, k in cases]
    assert got == want
    # the lane's counter and key: (x >> 2, y, t_lo, t_hi), (seed_lo, seed_hi)
    assert tuple(int(w, 16) for w in rest[0].split()) == tuple(int(x) for x in philox4x32_10((2, 5, 2, 1), (0x89abcdef, 0x01234567)))
    lo, hi = (np.float32(x) for x in rest[1].split())           # (nine digits name a float32)
    assert lo == np.float32(2. ** -24) == uniform(0) and hi == np.float32(1. - 2. ** -24) == uniform(0xffffffff)


def test_model_stream_layout_and_moments():
    z = normals64(130, 9, seed=7, t=(1 << 32) + 3)
    assert z.shape == (130, 9) and np.isfinite(z).all()
    # cells 4j, 4j+1 share a radius: z0^2 + z1^2 = -2 ln u(r0); the partial last lane is the head of a whole one
    r = philox4x32_10((np.arange(33, dtype=np.uint64)[:, None], np.arange(9, dtype=np.uint64)[None, :], 3, 1), (7, 0))
    assert np.allclose(z[0::4] ** 2 + z[1::4] ** 2, -2. * np.log(uniform(r[0])), rtol=1e-12)
    assert np.array_equal(z, normals64(132, 9, 7, (1 << 32) + 3)[:130])
    assert not np.array_equal(z, normals64(130, 9, 7, 3)) and not np.array_equal(z, normals64(130, 9, 8, (1 << 32) + 3))
    big = normals64(512, 512, seed=1, t=0)
    n = big.size
    assert abs(big.mean()) < 5. / np.sqrt(n) and abs(big.var() - 1.) < 5. * np.sqrt(2. / n)
    assert normals32(5, 3, 1, 0).dtype == np.float32


def model_of(d, bc):
    m = NoisyScalarModel(int(d["nx"]), int(d["ny"]), d["omega"], d["G"], d["Dg"], int(d["seed"]), bc)
    m.set_fields(np.zeros_like(d["u"]), d["u"], d["v"])
    m.set_f(d["f0"])
    return m


@pytest.mark.parametrize("bc", ["open", "periodic"])
def test_model_follows_noisy_reference_fixture(bc):
    d = golden("nf_run_%s_37x23" % bc)
    m = model_of(d, bc)
    done = 0
    for n in [int(s) for s in d["steps"]]:
        for t in range(done, n):
            assert np.array_equal(normals32(m.nx, m.ny, m.seed, t), d["z"][t])      # the stored normals are the stream's
            m.step()
        done = n
        tol = contract_tol(n)
        meas = dict(f=maxdiff(m.f, d["f_%d" % n]), rho=maxdiff(m.rho, d["rho_%d" % n]), feq=maxdiff(m.feq, d["feq_%d" % n]))
        print("%s after %d steps, measured / bound: f %.2e / %.1e, rho %.2e / %.1e, feq %.2e / %.1e"
              % (bc, n, meas["f"], tol["f"], meas["rho"], tol["rho"], meas["feq"], tol["f"]))
        assert meas["f"] <= tol["f"] and meas["rho"] <= tol["rho"] and meas["feq"] <= tol["f"]
    assert m.t == 50 and float(d["rho_50"].min()) >= 0.02 and float(d["rho_50"].max()) <= 0.98


def test_model_follows_noisy_phases_fixture_nan_and_clamp_exactly():
    d = golden("nf_phases_21x13")
    m = model_of(d, "open")
    tol = contract_tol(1)
    m.move()
    assert np.array_equal(m.f, d["f_move"])
    m.update_hydro()
    assert maxdiff(m.rho, d["rho_hydro"]) <= tol["rho"]
    m.update_feq()
    assert maxdiff(m.feq, d["feq_feq"]) <= tol["f"]
    m.collide_particles()
    nan_cells, clamped, want = d["nan_cells"], d["clamped"], d["f_collide"]
    room = d["rho_hydro"].astype(np.float64) * (1. - d["rho_hydro"].astype(np.float64))
    assert np.array_equal(nan_cells, room < -1e-3) and np.all((room > 1e-3) | nan_cells | (d["rho_hydro"] < 2e-4))
    assert nan_cells.any() and clamped.any() and (~nan_cells).any()
    assert np.array_equal(np.isnan(m.f), np.repeat(nan_cells[:, :, None], 9, axis=2))           # NaN in all nine links, nowhere else
    assert np.array_equal((m.f == 0.) & ~np.isnan(m.f), clamped)                                  # the clamped links: exactly 0
    ok = ~np.isnan(want)
    assert maxdiff(m.f[ok], want[ok]) <= tol["f"]


def test_class_parameters_worked_example():
    from LB_D2Q9.reaction_diffusion.noisy_fisher_wave import noisy_fisher_parameters
    p = noisy_fisher_parameters(z=0.1, D=1., g=1., Nc=10., N=10, time_prefactor=1.)
    assert p["lb_D"] == pytest.approx(1.) and p["omega"] == pytest.approx(1. / 3.5)
    assert p["lb_Gd"] == pytest.approx(1e-4) and p["lb_Dg"] == pytest.approx(1e-3)
    assert (p["nx"], p["ny"]) == (102, 102)
    assert p["lb_Gd"].dtype == np.float32 and p["lb_Dg"].dtype == np.float32 and p["omega"].dtype == np.float32
    assert p["Pe"] == 0.                                  # the reference's default vc = 0 (its init_hydro then divides by it)


def test_class_has_the_reference_surface():
    import inspect
    from LB_D2Q9.reaction_diffusion.noisy_fisher_wave import Noisy_Advected_Fisher_Wave as cls
    for m in ("init_hydro", "update_feq", "init_pop", "move", "move_bcs", "update_hydro", "collide_particles", "run", "get_fields",
              "set_pde_constants", "set_characteristic_length_time", "initialize_grid_dims"):
        assert callable(getattr(cls, m)), m
    names = list(inspect.signature(cls.__init__).parameters)
    assert names[1:15] == ["Lx", "Ly", "D", "z", "vx", "vy", "vc", "g", "Nc", "time_prefactor", "N", "two_d_local_size",
                           "three_d_local_size", "use_interop"]
    assert "seed" in names and "perturb" in names


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lb_set_noise", "lb_get_noise", "lb_set_noise_counter", "lb_noise_fill", "lb_set_noise_field")


def test_header_binding_and_library_agree_on_the_new_names(lbhip):
    from LB_D2Q9 import _native
    assert lbhip.lb_abi_version() == 11 == _native.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    assert re.search(r"#define\s+LB_ABI_VERSION\s+11\b", header)
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(lb_sim \*s[,)]" % name, header, re.M), name
        assert name in _native.EXPORTS and getattr(lbhip, name).argtypes is not None, name
        fn = getattr(lbhip, name)                          # a null handle is an argument error, not a crash
        args = [0 if t in (ct.c_uint64, ct.c_int, ct.c_float) else None for t in fn.argtypes]
        assert fn(*args) == -1 and b"null" in lbhip.lb_last_error()
    assert _native.SIGNATURES["lb_set_noise"][0][2] is ct.c_uint64 and _native.SIGNATURES["lb_noise_fill"][0][1] is ct.c_uint64
