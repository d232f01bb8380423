"""Scalar lattices without a GPU: the numpy model against the fixtures recorded from the reference's C, the drop-in classes'
parameter arithmetic, the new ABI symbols, lb_create's refusals as status codes, the planner's launch split."""
import ctypes as ct
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden
from scalar_model import ScalarModel, contract_tol

RUN_FIXTURES = ("ad_diffusion_37x23", "ad_advection_37x23", "ad_fisher_37x23")


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def model_of(d, bc="open"):
    m = ScalarModel(int(d["nx"]), int(d["ny"]), d["omega"], d["G"], bc)
    m.set_fields(np.zeros_like(d["u"]), d["u"], d["v"])
    m.set_f(d["f0"])
    return m


@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_model_follows_reference_fixture(name):
    d = golden(name)
    m = model_of(d)
    done = 0
    for n in [int(s) for s in d["steps"]]:
        m.run(n - done)
        done = n
        tol = contract_tol(n)
        meas = dict(f=maxdiff(m.f, d["f_%d" % n]), rho=maxdiff(m.rho, d["rho_%d" % n]), feq=maxdiff(m.feq, d["feq_%d" % n]))
        print("%s after %d steps, measured / bound: f %.2e / %.1e, rho %.2e / %.1e, feq %.2e / %.1e"
              % (name, n, meas["f"], tol["f"], meas["rho"], tol["rho"], meas["feq"], tol["f"]))
        assert meas["f"] <= tol["f"] and meas["rho"] <= tol["rho"] and meas["feq"] <= tol["f"]


def test_model_phases_follow_reference_fixture():
    d = golden("ad_phases_21x13")
    m = model_of(d)
    tol = contract_tol(1)
    m.move()
    assert np.array_equal(m.f, d["f_move"])                   # streaming moves values, it computes nothing
    m.update_hydro()
    assert maxdiff(m.rho, d["rho_hydro"]) <= tol["rho"]
    m.update_feq()
    assert maxdiff(m.feq, d["feq_feq"]) <= tol["f"]
    m.collide_particles()
    assert maxdiff(m.f, d["f_collide"]) <= tol["f"]


def test_open_box_keeps_its_edge_links_frozen():
    """The fact the edge state rests on: in the reference's box a link that enters from outside holds, at every step's
    moments, the value it had when the populations were set (the fixture's f after `move` shows it)."""
    d = golden("ad_phases_21x13")
    f0, fm = d["f0"], d["f_move"]
    assert np.array_equal(fm[0, :, [1, 5, 8]], f0[0, :, [1, 5, 8]])
    assert np.array_equal(fm[-1, :, [3, 6, 7]], f0[-1, :, [3, 6, 7]])
    assert np.array_equal(fm[:, 0, [2, 5, 6]], f0[:, 0, [2, 5, 6]])
    assert np.array_equal(fm[:, -1, [4, 7, 8]], f0[:, -1, [4, 7, 8]])
    m = model_of(d)
    e = m.get_edge_state()
    assert e.shape == (6 * (21 + 13),)
    m2 = model_of(d)
    m2.set_edge_state(e)
    assert np.array_equal(m2.frozen[0, :, 5], m.frozen[0, :, 5]) and np.array_equal(m2.get_edge_state(), e)


# ---- the classes' parameter arithmetic (worked out from the formulas of reaction_diffusion/diffusion.py) -----------------
def test_diffusion_parameters():
    from LB_D2Q9.reaction_diffusion import diffusion as rd
    p = rd.diffusion_parameters(D=1., z=0.1, N=50)
    assert p["L"] == pytest.approx(0.1) and p["T"] == pytest.approx(0.01)
    assert p["delta_x"] == pytest.approx(0.02) and p["delta_t"] == pytest.approx(4e-4) and p["ulb"] == pytest.approx(0.02)
    assert p["lb_D"] == pytest.approx(1.) and p["omega"] == pytest.approx(1. / 3.5)
    assert (p["lx"], p["ly"], p["nx"], p["ny"]) == (500, 500, 502, 502)
    q = rd.diffusion_parameters(Lx=0.5, Ly=0.3, D=2., z=0.1, time_prefactor=0.5, N=20)
    # T = z^2 / D = 0.005; delta_t = 0.5 / 400; lb_D = 0.5; omega = 1 / (0.5 + 1.5)
    assert q["T"] == pytest.approx(0.005) and q["delta_t"] == pytest.approx(1.25e-3) and q["lb_D"] == pytest.approx(0.5)
    assert q["omega"] == pytest.approx(0.5)
    assert (q["nx"], q["ny"]) == (20 * int(0.5 / 0.1) + 2, 20 * int(0.3 / 0.1) + 2)


def test_advection_diffusion_parameters():
    from LB_D2Q9.reaction_diffusion import diffusion as rd
    p = rd.advection_diffusion_parameters(vx=2., vy=-1., vc=4., D=0.2, z=0.1, N=25, Lx=0.4, Ly=0.2)
    # L = 0.1, T = z / vc = 0.025, Pe = z vc / D = 2, delta_x = 0.04, delta_t = 1.6e-3, lb_D = 1 / Pe = 0.5, omega = 1 / 2
    assert p["T"] == pytest.approx(0.025) and p["Pe"] == pytest.approx(2.)
    assert p["lb_D"] == pytest.approx(0.5) and p["omega"] == pytest.approx(0.5)
    assert p["lb_vx"] == pytest.approx(0.04 * 0.5) and p["lb_vy"] == pytest.approx(0.04 * -0.25)
    assert (p["nx"], p["ny"]) == (102, 52)


def test_fisher_parameters():
    from LB_D2Q9.reaction_diffusion import diffusion as rd
    p = rd.reaction_diffusion_parameters(g=3., D=1., z=0.1, N=50)
    # G_dim = T g = 0.03; G = G_dim delta_t = 1.2e-5
    assert p["G_dim"] == pytest.approx(0.03) and p["G"] == pytest.approx(1.2e-5) and p["omega"] == pytest.approx(1. / 3.5)
    q = rd.reaction_advection_diffusion_parameters(g=8., vx=1., vy=0., vc=2., D=0.1, z=0.1, N=10)
    # T = 0.05, Pe = 2, G_dim = 0.4, delta_t = 0.01, G = 4e-3, vf = 2 sqrt(0.4 / 2)
    assert q["G_dim"] == pytest.approx(0.4) and q["G"] == pytest.approx(4e-3)
    assert q["vf_dim"] == pytest.approx(2. * np.sqrt(0.2)) and q["lb_vx"] == pytest.approx(0.1 * 0.5)


def test_gaussian_fits_boxes_that_are_not_square():
    from LB_D2Q9.reaction_diffusion import diffusion as rd
    xc, yc, X, Y, rho = rd.gaussian_blob(12, 7, 5)
    assert rho.shape == (12, 7) and rho.dtype == np.float32 and (xc, yc) == (6, 3)
    assert rho[6, 3] == 1. and rho[7, 3] == pytest.approx(np.exp(-0.04), rel=1e-6) and X[7, 3] == pytest.approx(0.2)
    _, _, _, _, sq = rd.gaussian_blob(9, 9, 5)
    assert np.array_equal(sq, sq.T)                 # square boxes: what the reference's (ny, nx) meshgrid gives


def test_classes_have_the_reference_surface():
    from LB_D2Q9.reaction_diffusion import diffusion as rd
    for cls in (rd.Diffusion, rd.Advection_Diffusion, rd.Reaction_Diffusion, rd.Reaction_Advection_Diffusion):
        for m in ("init_hydro", "update_feq", "init_pop", "move", "move_bcs", "update_hydro", "collide_particles", "run",
                  "get_fields", "get_nondim_fields", "get_physical_fields", "step", "set_D_and_omega",
                  "set_characteristic_length_time", "initialize_grid_dims"):
            assert callable(getattr(cls, m)), (cls.__name__, m)
    assert not hasattr(rd, "Reaction_Advection_Diffusion_Stochastic")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lb_set_reaction", "lb_edge_floats", "lb_get_edge_state", "lb_set_edge_state", "lb_set_velocity_from")


def test_new_symbols_exported_and_bound(lbhip):
    from LB_D2Q9 import _native
    assert lbhip.lb_abi_version() == 11 == _native.ABI_VERSION
    assert _native.LB_SEM_DIFFUSION == 3 and _native.LB_BC_OPEN == 4 and _native.BC_NAMES["open"] == 4
    for name in NEW_SYMBOLS:
        assert name in _native.EXPORTS and getattr(lbhip, name).argtypes is not None, name
    assert ct.sizeof(_native.LbParams) == 64
    for name in NEW_SYMBOLS:                          # a null handle is an argument error, not a crash
        fn = getattr(lbhip, name)
        args = [None] * len(fn.argtypes)
        if name == "lb_set_reaction":
            args[1] = 0.
        assert fn(*args) == -1 and b"null" in lbhip.lb_last_error()


def _params(**kw):
    from LB_D2Q9 import _native
    p = _native.LbParams()
    p.nx, p.ny, p.y0, p.local_ny, p.omega = 16, 12, 0, 12, 1.0
    p.semantics, p.bc_mode, p.device = _native.LB_SEM_DIFFUSION, _native.LB_BC_PERIODIC, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, word", [
    (dict(local_ny=6), b"slab"),                                   # a slab
    (dict(y0=2, local_ny=10), b"slab"),
    (dict(flags=1), b"halo"),                                      # LB_FLAG_HALO
    (dict(device=-1), b"CPU"),                                     # LB_DEVICE_CPU
    (dict(bc_mode=0), b"LB_BC_PERIODIC and LB_BC_OPEN"),           # the other three families with this semantics
    (dict(bc_mode=2), b"LB_BC_PERIODIC and LB_BC_OPEN"),
    (dict(bc_mode=3), b"LB_BC_PERIODIC and LB_BC_OPEN"),
    (dict(bc_mode=4, semantics=0), b"LB_BC_OPEN"),                 # LB_BC_OPEN with any other semantics
    (dict(bc_mode=4, semantics=1), b"LB_BC_OPEN"),
    (dict(bc_mode=4, semantics=2), b"LB_BC_OPEN"),
    (dict(bc_mode=5), b"bc_mode"),
])
def test_create_refusals_are_status_codes_with_messages(lbhip, kw, word):
    """Refused before any device is touched: these hold on a box without a GPU."""
    h = ct.c_void_p()
    p = _params(**kw)
    assert lbhip.lb_create(ct.byref(p), ct.byref(h)) == -1 and not h.value          # LB_ERR_ARG
    msg = lbhip.lb_last_error()
    assert word.lower() in msg.lower(), msg


# ---- the planner -----------------------------------------------------------------------------------------------------------
PLAN_DRIVER = r"""
#include <stdio.h>
#include "plan.h"
int main()
{
    PlanInputs s;
    s.p = lb_params();
    s.p.nx = 512; s.p.ny = 512; s.p.local_ny = 512; s.p.semantics = LB_SEM_DIFFUSION; s.p.bc_mode = LB_BC_OPEN; s.p.omega = 1.f;
    s.H = 512; s.pitch = 512; s.rowp = 9 * 512; s.plane = 512;
    const int variants[3] = {1 << 9, 0, -1};       // the tile bit; k_ad_step; automatic
    for (int v : variants) {
        s.variant = v;
        const int ns[5] = {0, 1, 5, 10, 13};
        for (int n : ns) {
            int d[32];
            const int c = plan_launches(&s, n, d, 32);
            printf("%d:", n);
            for (int i = 0; i < c; ++i) printf(" %d", d[i]);
            printf("\n");
        }
        char name[256];
        hot_kernel(&s, name, sizeof(name));
        printf("%d %s\n", steps_per_launch(&s), name);
    }
    s.variant = (1 << 9) | (3 << 2);
    printf("%d\n", scalar_tile_shape(&s));
    s.variant = 1 << 9;
    printf("%d\n", scalar_tile_shape(&s));
    // the size rule of the automatic choice: boxes of n x n cells on which k_ad_tile4 is taken
    s.variant = -1;
    const int sizes[8] = {64, 256, 512, 1024, 2048, 4096, 8192, 16384};
    for (int n : sizes) { s.p.nx = s.p.ny = s.p.local_ny = s.H = n; printf("%d", scalar_use_tiles(&s) ? 1 : 0); }
    printf("\n");
    return 0;
}
"""


# boxes of 64^2, 256^2, 512^2 ... 8192^2, 16384^2 cells on which the automatic choice takes k_ad_tile4: the sizes at which
# profiles/scalar_bench.txt measured it faster than four launches of k_ad_step -- all it measured, 256^2 ... 8192^2
SIZE_RULE = "01111110"


def test_launch_split_of_the_planner(tmp_path):
    """plan.cpp is plain C++: compiled here with the host compiler and asked how a scalar run is split: n = 4a + r as a launches
    of k_ad_tile4, then r of k_ad_step, where the tiles are chosen; single steps otherwise."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    csrc = os.path.join(ROOT, "2d-lb_amd", "csrc")
    (tmp_path / "drv.cpp").write_text(PLAN_DRIVER)
    exe = str(tmp_path / "drv")
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-I" + csrc, str(tmp_path / "drv.cpp"), os.path.join(csrc, "plan.cpp"), "-o", exe])
    out = subprocess.check_output([exe]).decode().splitlines()
    assert out[0:5] == ["0:", "1: 1", "5: 4 1", "10: 4 4 1 1", "13: 4 4 4 1"]
    assert out[5].startswith("4 k_ad_tile4") and out[5].endswith("<OPEN>")
    assert out[6:11] == ["0:", "1: 1", "5:" + " 1" * 5, "10:" + " 1" * 10, "13:" + " 1" * 13]
    assert out[11].startswith("1 k_ad_step") and out[11].endswith("<OPEN>")
    auto = out[12:18]                                # 512^2 open, automatic: one of the two plans, consistently
    assert auto[:5] in (out[0:5], out[6:11]) and auto[5][0] == ("4" if auto[2] == "5: 4 1" else "1")
    assert out[18] == "2" and out[19] == "1"         # forced shape 3 -> 16 x 16; none forced: by size as for k_tile4 (512^2: 32 x 16, one cell per thread)
    assert out[20] == SIZE_RULE, out[20]
