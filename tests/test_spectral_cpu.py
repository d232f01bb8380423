"""The spectral screened-Poisson solver without a GPU: the numpy model (tests/spectral_model.py) against closed forms, the fixtures
against what they claim, the parameter arithmetic against hand values, the C ABI's new symbols and the refusals that come before any
device is touched, and the transform's plan (2d-lb_amd/csrc/spectral_plan.cpp) swept on a host -- tests/spectral_plan_props.cpp, its own
main, linked with spectral_plan.cpp only, built plain and with -fsanitize=address,undefined (a stand-alone program: nothing is
preloaded).  tests/test_gpu_spectral.py holds the kernels to the model.
"""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import spectral_model as M
from conftest import ROOT, golden
from scalar_model import contract_tol

CSRC = os.path.join(ROOT, "2d-lb_amd", "csrc")
NEW_SYMBOLS = ("lb_spectral_create", "lb_spectral_destroy", "lb_spectral_set_lambda", "lb_spectral_set", "lb_spectral_get",
               "lb_spectral_transform", "lb_spectral_screen", "lb_spectral_grad_multiply", "lb_spectral_solve",
               "lb_spectral_velocity", "lb_run_screened")


# ---- the model against closed forms ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny,lam", [(30, 18, 1.0), (8, 6, 0.5), (5, 3, 2.0)])
def test_a_delta_charge_has_the_screening_as_its_spectrum(nx, ny, lam):
    charge = np.zeros((nx, ny))
    charge[0, 0] = 1.
    spec, _, _ = M.solve(charge, lam)
    kx, ky = M.wave_grids(nx, ny)
    assert np.abs(spec - 1. / (1. + lam ** 2 * (kx ** 2 + ky ** 2))).max() <= 1e-14
    assert kx.min() == -(nx // 2) and kx.max() == (nx - 1) // 2            # (the Nyquist index of an even axis is -n/2)


@pytest.mark.parametrize("nx,ny,a,b,lam", [(30, 18, 2, 1, 1.0), (30, 18, 0, 3, 0.7), (8, 6, 1, -2, 1.0), (50, 50, 7, 5, 0.3)])
def test_a_single_mode_gives_the_closed_form_gradient(nx, ny, a, b, lam):
    X, Y = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    phase = 2 * np.pi * (a * X / float(nx) + b * Y / float(ny))
    _, xg, yg = M.solve(np.cos(phase), lam)
    screen = 1. + lam ** 2 * (a ** 2 + b ** 2)
    assert np.abs(xg - (-2 * np.pi * a * np.sin(phase) / screen)).max() <= 1e-12
    assert np.abs(yg - (-2 * np.pi * b * np.sin(phase) / screen)).max() <= 1e-12


def test_the_nyquist_mode_has_no_real_x_gradient_but_an_imaginary_one():
    nx, ny = 30, 18
    X, _ = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    charge = np.cos(np.pi * X)                                              # the mode kx = -nx/2
    _, xg, yg = M.solve(charge, 1.0)
    assert np.abs(xg.real).max() <= 1e-12 and np.abs(yg).max() <= 1e-12
    want = 2 * np.pi * (nx // 2) / (1. + (nx // 2) ** 2)
    assert abs(np.abs(xg.imag).max() - want) <= 1e-12 and want > 0.4


def test_the_wave_indices_are_the_references():
    for n, dx in ((30, 0.1), (18, 0.1), (5, 1.0), (4096, 0.02)):
        L = dx * n
        assert np.abs(L * np.fft.fftfreq(n, d=dx) - M.wave_index(n)).max() <= 4e-12 * n


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 8, 18, 30, 48, 50, 64, 96, 250, 360])
def test_the_devices_passes_are_a_fourier_transform(n):
    """The index scheme of csrc/kernels_spectral.h (sp_pass), restated in numpy, against numpy's fft for every radix mix."""
    rng = np.random.RandomState(n)
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    assert np.abs(M.stockham(x) - np.fft.fft(x)).max() <= 1e-12 * max(1, n)


# ---- the fixtures -----------------------------------------------------------------------------------------------------------
def test_the_solve_fixture_is_the_float64_model_of_its_charge():
    g = golden("sp_solve_30x18")
    assert g["charge"].shape == (30, 18) and g["charge"].dtype == np.float32
    spec, xg, yg = M.solve(g["charge"], float(g["lam"]))
    for got, key in ((spec, "spec"), (xg, "xgrad"), (yg, "ygrad")):
        assert g[key].dtype == np.complex128 and np.abs(got - g[key]).max() <= 1e-13 * np.abs(g[key]).max()
    # the noisy droplet's Nyquist column leaves an imaginary part the reference drops with .real
    assert 1e-3 < np.abs(g["xgrad"].imag).max() / np.abs(g["xgrad"].real).max() < 0.1


@pytest.mark.parametrize("bc", ["open", "periodic"])
def test_the_fisher_fixture_is_the_float64_model_and_the_float32_model_follows_it(bc):
    g = golden("sp_fisher_30x18")
    nx, ny = int(g["nx"]), int(g["ny"])
    assert (nx, ny) == (30, 18) and list(g["steps"]) == [1, 10, 50]
    p = M.fisher_lattice_parameters(3., 1.8, 1., 1., 10)
    assert p["omega"] == g["omega"] and p["lb_G"] == g["G"] and p["scale"] == g["scale"]
    assert np.array_equal(g["rho0"], M.noisy_droplet(nx, ny, 10, 0.5, 20240611))
    m64, m32 = (M.ScreenedFisherModel(nx, ny, g["omega"], g["G"], float(g["lam"]), g["scale"], bc=bc, dtype=t)
                for t in (np.float64, np.float32))
    done = 0
    for m in (m64, m32):
        m.redo_initial_condition(g["rho0"])
    for n in g["steps"]:
        for m in (m64, m32):
            m.run(n - done)
        done = int(n)
        tol = contract_tol(n)
        for k in ("f", "rho", "u", "v"):
            want = g["%s_%s_%d" % (bc, k, n)]
            assert np.array_equal(getattr(m64, k), want), (k, n)
            assert np.abs(getattr(m32, k) - want).max() <= tol[k], (k, n)
        assert max(np.abs(m64.u).max(), np.abs(m64.v).max()) < 0.15 and 0. <= m64.rho.min() and m64.rho.max() <= 1.5
    # growth: in the periodic box, where streaming and relaxation conserve it, the total mass rises, by exactly G sum rho (1 - rho) a
    # step (the open box also loses what leaves through its edges); the velocity is not negligible: the coupling is exercised
    rho50 = g["%s_rho_50" % bc]
    if bc == "periodic":
        assert rho50.sum() > g["%s_rho_10" % bc].sum() > g["rho0"].sum()
        m64.step()
        assert abs(m64.rho.sum() - rho50.sum() - float(g["G"]) * (rho50 * (1. - rho50)).sum()) <= 1e-11
    assert np.abs(g["%s_u_50" % bc]).max() > 1e-3


# ---- parameter arithmetic ---------------------------------------------------------------------------------------------------
def test_screened_fisher_parameters_against_hand_values():
    from LB_D2Q9.reaction_diffusion.screened_poisson_waves import gaussian_droplet, screened_fisher_parameters
    p = screened_fisher_parameters(Lx=3., Ly=1.8, vc=1., time_prefactor=1., N=10)
    assert (p["nx"], p["ny"]) == (30, 18)                                   # round(N L): no "+ 2"
    assert p["delta_x"] == 0.1 and abs(p["delta_t"] - 0.01) < 1e-15 and abs(p["ulb"] - 0.1) < 1e-15
    assert p["lb_D"] == np.float32(0.25) and abs(float(p["omega"]) - 0.8) < 2e-7 and p["omega"].dtype == np.float32
    assert p["lb_G"] == np.float32(0.01) and abs(p["velocity_scale"] + 0.1) < 1e-15
    q = screened_fisher_parameters(Lx=1., Ly=1., vc=2.5, time_prefactor=0.5, N=50)
    assert (q["nx"], q["ny"]) == (50, 50) and abs(q["delta_t"] - 2e-4) < 1e-18 and abs(q["velocity_scale"] + 0.025) < 1e-15
    assert abs(float(q["omega"]) - 1. / (.5 + 3 * .125)) < 2e-7
    m = M.fisher_lattice_parameters(3., 1.8, 1., 1., 10)
    assert m["omega"] == p["omega"] and m["lb_G"] == p["lb_G"] and m["scale"] == np.float32(p["velocity_scale"])
    # the droplet on a box that is not square: (nx, ny), centred on (nx // 2, ny // 2), indexing='ij'
    xc, yc, X, Y, rho = gaussian_droplet(30, 18, 10, 0.5)
    assert (xc, yc) == (15, 9) and rho.shape == (30, 18) and rho[15, 9] == 1. and rho.dtype == np.float32
    assert abs(rho[20, 9] - np.exp(-(0.5 ** 2) / 0.25)) < 1e-7 and abs(rho[15, 12] - np.exp(-(0.3 ** 2) / 0.25)) < 1e-7


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_exported_declared_and_bound(lbhip):
    from LB_D2Q9 import _native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lb_hip.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert hasattr(lbhip, name), name
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in _native.SIGNATURES and list(getattr(lbhip, name).argtypes) == list(_native.SIGNATURES[name][0]), name
    assert re.search(r"#define LB_ABI_VERSION 11\b", text) and lbhip.lb_abi_version() == 11
    assert "typedef struct lb_spectral lb_spectral;" in text


@pytest.mark.parametrize("nx,ny", [(7, 8), (8, 4097), (0, 4)])
def test_create_refuses_other_lengths_with_the_rule_before_any_device(lbhip, nx, ny):
    h = ct.c_void_p()
    assert lbhip.lb_spectral_create(nx, ny, 0, 1.0, ct.byref(h)) == -1 and not h.value        # LB_ERR_ARG
    msg = lbhip.lb_last_error().decode()
    assert "2^a 3^b 5^c" in msg and "4096" in msg and "%d x %d" % (nx, ny) in msg, msg


def test_null_arguments_are_status_codes(lbhip):
    assert lbhip.lb_spectral_create(8, 8, 0, 1.0, None) == -1
    assert lbhip.lb_spectral_destroy(None) == 0
    for call in (lambda: lbhip.lb_spectral_solve(None), lambda: lbhip.lb_spectral_screen(None),
                 lambda: lbhip.lb_spectral_transform(None, 0, 1), lambda: lbhip.lb_spectral_velocity(None, None, 1.0, 0),
                 lambda: lbhip.lb_run_screened(None, None, 1.0, 1)):
        assert call() == -1 and b"null" in lbhip.lb_last_error()


# ---- the plan on a host ----------------------------------------------------------------------------------------------------
PROPERTIES = ("S1_admissible", "S2_radix_product", "S3_lds", "S4_coverage", "S5_twiddles")


def _compile(out, extra):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + extra +
                          [os.path.join(ROOT, "tests", "spectral_plan_props.cpp"), os.path.join(CSRC, "spectral_plan.cpp"), "-o", out])
    return out


def _assert_all_hold(run):
    print(run.stdout)
    print(run.stderr[-3000:])
    found = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\w+) cases=(\d+) bad=(\d+)$", run.stdout, re.M)}
    for name in PROPERTIES:
        assert name in found, (name, "not reported")
        cases, bad = found[name]
        assert cases > 0 and bad == 0, (name, cases, bad)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])


def test_the_plan_keeps_its_invariants(tmp_path):
    exe = _compile(str(tmp_path / "spectral_plan_props"), ["-O2"])
    _assert_all_hold(subprocess.run([exe], capture_output=True, text=True, timeout=600))


def test_the_plan_keeps_its_invariants_under_the_sanitizers(tmp_path):
    exe = _compile(str(tmp_path / "spectral_plan_props_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run = subprocess.run([exe, "--thin"], capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    _assert_all_hold(run)


# (nx, ny) -> (rows, cols, ny % rows, nx % cols, x passes, y passes): what tests/test_gpu_spectral.py's docstring says of its batched shapes
# and tests/test_gpu_nutrient.py's of its two wide boxes
BATCHED_PLANS = {
    (1, 1): (1, 1, 0, 0, [], []), (1, 6): (1, 1, 0, 0, [], [3, 2]), (6, 1): (1, 1, 0, 0, [3, 2], []),
    (625, 48): (1, 2, 0, 1, [5, 5, 5, 5], [3, 4, 4]), (1000, 30): (1, 3, 0, 1, [5, 5, 5, 4, 2], [5, 3, 2]),
    (800, 640): (1, 3, 0, 2, [5, 5, 4, 4, 2], [5, 4, 4, 4, 2]), (48, 1000): (3, 1, 1, 0, [3, 4, 4], [5, 5, 5, 4, 2]),
    (250, 625): (2, 1, 1, 0, [5, 5, 5, 2], [5, 5, 5, 5]), (64, 3750): (14, 1, 12, 0, [4, 4, 4], [5, 5, 5, 5, 3, 2]),
    (6, 2187): (8, 1, 3, 0, [3, 2], [3] * 7), (3125, 6): (1, 12, 0, 5, [5] * 5, [3, 2]),
    (3600, 3): (1, 14, 0, 2, [5, 5, 3, 3, 4, 4], [3]), (4096, 250): (1, 16, 0, 0, [4] * 6, [5, 5, 5, 2]),
    (512, 2048): (2, 2, 0, 0, [4, 4, 4, 4, 2], [4, 4, 4, 4, 4, 2]),
    (4096, 4): (1, 16, 0, 0, [4] * 6, [4]), (4, 4096): (16, 1, 0, 0, [4], [4] * 6),
    (1000, 12): (1, 3, 0, 1, [5, 5, 5, 4, 2], [3, 4]), (12, 1000): (3, 1, 1, 0, [3, 4], [5, 5, 5, 4, 2]),
}


def test_the_batched_shapes_of_the_gpu_tests_have_the_plans_their_docstrings_state(tmp_path):
    """sp_plan itself (spectral_plan_props --plan), not a restatement: rows, cols, what the last block lacks, the passes of both axes and
    the LDS of each batched shape the GPU tests list; every other shape of theirs has no batch."""
    import test_gpu_nutrient as TN
    import test_gpu_spectral as TG
    assert set(TG.BATCHED) <= set(BATCHED_PLANS) and set(TG.SHAPES) == set(TG.PLAIN) | set(TG.BATCHED)
    assert {(1000, 12), (12, 1000)} <= set(TN.BOXES)
    shapes = sorted(set(BATCHED_PLANS) | set(TG.SHAPES) | set(TN.BOXES))
    exe = _compile(str(tmp_path / "spectral_plan_props"), ["-O2"])
    run = subprocess.run([exe, "--plan"] + [str(n) for s in shapes for n in s], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    print(run.stdout)
    got = {}
    for m in re.finditer(r"^PLAN (\d+) (\d+) rows (\d+) cols (\d+) row_lds (\d+) col_lds (\d+) x (\S+) y (\S+)$", run.stdout, re.M):
        nx, ny, rows, cols, row_lds, col_lds = (int(m.group(i)) for i in range(1, 7))
        px, py = ([] if m.group(i) == "-" else [int(r) for r in m.group(i).split(",")] for i in (7, 8))
        got[(nx, ny)] = (rows, cols, ny % rows, nx % cols, px, py)
        assert row_lds == 16 * rows * nx <= 65536 and col_lds == 16 * cols * ny <= 65536
        assert px == M.radix_passes(nx) and py == M.radix_passes(ny)
    assert sorted(got) == shapes
    for s in shapes:
        if s in BATCHED_PLANS:
            assert got[s] == BATCHED_PLANS[s], (s, got[s])
        else:
            assert got[s][:2] == (1, 1), (s, got[s])


def test_the_model_restates_the_plans_passes():
    """radix_passes (the model's) is the order spectral_plan.cpp writes: 5s, 3s, 4s, a 2."""
    src = open(os.path.join(CSRC, "spectral_plan.cpp")).read()
    assert "for (int r : {5, 3, 4, 2})" in src
    assert M.radix_passes(4096) == [4] * 6 and M.radix_passes(30) == [5, 3, 2] and M.radix_passes(96) == [3, 4, 4, 2]
