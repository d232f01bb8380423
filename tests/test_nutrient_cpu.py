"""A population and its nutrient under a spectral velocity, without a GPU: the numpy model against the fixtures recorded from the
reference's C (float64 to rounding, float32 within the parity contract), what the fixtures claim to be, the parameter arithmetic
against hand values, the drop-in classes' constants, the five ABI symbols, the collision's conservation law."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from nutrient_model import CS32, PARAMS, NutrientModel, from_fixture, lattice_parameters, nutrient_bounds
from scalar_model import contract_tol

RUN_FIXTURES = ("sn_plain_30x18", "sn_clumpy_30x18", "sn_clumpy_5x4", "sn_clumpy_3x3")
PHASES = "sn_phases_20x12"
STEPS = [1, 10, 50]
NAMES = ("f", "feq", "rho", "u", "v", "psi", "Fx", "Fy")
ENTRY_POINTS = ("lb_run_nutrient", "lb_nutrient_velocity", "lb_update_forces_nutrient", "lb_collide_nutrient", "lb_get_nutrient_fields")


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def bounds(params, n, rho_max):
    """The parity contract for n steps in f, feq, rho, u, v; psi and F take the bounds that follow from rho's (nutrient_bounds)."""
    tol = contract_tol(n)
    nb = nutrient_bounds(params, rho_max, tol["rho"])
    return dict(f=tol["f"], feq=tol["f"], rho=tol["rho"], u=tol["u"], v=tol["v"], psi=nb["psi"], Fx=nb["F"], Fy=nb["F"])


def compare(label, params, n, have, want):
    """Print measured / bound for every array, then hold each to its bound."""
    b = bounds(params, n, float(np.max(np.asarray(want["rho"])[:, :, 0])))
    for k in [k for k in NAMES if k in want and k in have]:
        d = maxdiff(have[k], want[k])
        print("%s: %s %.2e / %.1e" % (label, k, d, b[k]))
        assert d <= b[k], (label, k, d, b[k])


def close64(label, have, want):
    """float64 against float64: 1e-12 of the array's size"""
    for k in [k for k in NAMES if k in want and k in have]:
        d, size = maxdiff(have[k], want[k]), max(float(np.max(np.abs(want[k]))), 1e-30)
        assert d <= 1e-12 * max(size, 1e-3), (label, k, d, size)


def recorded(d, n, tag=""):
    return {k: d["%s_%d%s" % (k, n, tag)] for k in NAMES if "%s_%d%s" % (k, n, tag) in d.files}


@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_model_reproduces_the_reference(name):
    d = golden(name)
    assert [int(n) for n in d["steps"]] == STEPS
    m64, m32 = from_fixture(d, np.float64), from_fixture(d, np.float32)
    done = 0
    for n in STEPS:
        m64.run(n - done), m32.run(n - done)
        done = n
        close64("%s step %d" % (name, n), m64.state(), recorded(d, n))
        have32 = m32.state()
        if n != STEPS[-1]:
            have32.pop("f")                     # (f of the float32 build is recorded at the last step only)
        compare("%s step %d float32 model / float32 build" % (name, n), m32.params, n, have32, recorded(d, n, "_f32"))
        compare("%s step %d float32 model / float64 build" % (name, n), m32.params, n, m32.state(), recorded(d, n))


@pytest.mark.parametrize("variant", ("plain", "clumpy"))
def test_model_reproduces_the_reference_stage_by_stage(variant):
    d = golden(PHASES)
    assert (int(d["nx"]), int(d["ny"])) == (20, 12)
    m64, m32 = from_fixture(d, np.float64, variant + "_"), from_fixture(d, np.float32, variant + "_")
    seen = 0
    for stage in NutrientModel.STAGES:
        for m, tag in ((m64, ""), (m32, "_f32")):
            getattr(m, stage)()
            have = dict(m.state(), feq=m.feq)
            want = {k: d[key] for k in NAMES for key in ["%s_%s_after_%s%s" % (variant, k, stage, tag)] if key in d.files}
            seen += len(want)
            if tag:
                compare("%s after %s" % (variant, stage), m.params, 1, {k: have[k] for k in want}, dict(want, rho=m64.rho))
            else:
                close64("%s after %s" % (variant, stage), {k: have[k] for k in want}, want)
    assert seen == 2 * (6 + 3 * (variant == "clumpy"))       # f, rho, u, v, feq, f [+ psi, Fx, Fy], both builds


@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_fixture_is_what_it_claims(name):
    """The recorder's acceptance conditions, re-checked on the file; the header is the issue's case; the start is the float32
    equilibrium of 1.2 x the seeded droplet on a uniform nutrient under the velocity it implies."""
    d = golden(name)
    nx, ny = int(d["nx"]), int(d["ny"])
    assert name.endswith("%dx%d" % (nx, ny)) and bool(d["clumpy"]) == ("clumpy" in name)
    p = lattice_parameters(nx / 10., ny / 10., 10, vc=0.5, Dn=0.1)
    assert (p["nx"], p["ny"]) == (nx, ny)
    assert np.float32(d["omega"][0]) == p["omega"] == np.float32(0.8) and np.float32(d["omega"][1]) == p["omega_n"] == np.float32(1.25)
    params = dict(zip(PARAMS, d["params"]))
    assert np.float32(params["G"]) == np.float32(0.01) and np.float32(params["scale"]) == np.float32(-0.05) and params["lam"] == 1.
    assert params["rho_o"] == 1. and params["G_chen"] == (-1. if "clumpy" in name else 0.)
    assert d["f0"].dtype == np.float32 and d["rho0"].dtype == np.float32 and np.all(d["rho0"][:, :, 1] == 1.)
    m = from_fixture(d, np.float64)
    m.redo_initial_condition(d["rho0"])
    assert np.array_equal(m.f.astype(np.float32), d["f0"])
    for n in STEPS:
        want, f32 = recorded(d, n), recorded(d, n, "_f32")
        compare("%s step %d builds" % (name, n), params, n, f32, want)
        assert float(np.sqrt(want["u"] ** 2 + want["v"] ** 2).max()) < 0.15
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < (1 << 20)


def test_collision_conserves_population_plus_nutrient():
    """+ w_k G rho_p rho_n and - w_k G rho_p rho_n cancel, the force term sums to zero over the links, the stream and the solve move
    nothing out of the periodic box: sum(rho_p + rho_n) stays, in float64 to rounding, while each part changes."""
    rng = np.random.default_rng(5)
    for clumpy in (False, True):
        m = NutrientModel(12, 10, 0.8, 1.25, clumpy=clumpy, dtype=np.float64, G=0.05, scale=-0.05, rho_o=1., G_chen=-1., lam=1.)
        rho = np.stack([rng.uniform(0.2, 1.2, (12, 10)), rng.uniform(0.5, 1., (12, 10))], axis=2)
        m.redo_initial_condition(rho)
        m.update_hydro()
        total, parts = m.rho.sum(), m.rho.sum(axis=(0, 1))
        m.run(20)
        m.move(), m.update_hydro()
        assert abs(m.rho.sum() - total) <= 1e-12 * total
        assert m.rho[:, :, 0].sum() > parts[0] * 1.01 and m.rho[:, :, 1].sum() < parts[1]


def test_bounds_follow_from_the_density():
    """psi's is the density's plus rounding; F's is (2 / 9) |G_chen| psi_max of it plus rounding; both grow with the tolerance."""
    b = nutrient_bounds(dict(rho_o=1., G_chen=-1.), 1.4, 1e-5)
    assert 1e-5 < b["psi"] < 1.1e-5 and (2. / 9.) * 1e-5 < b["F"] < 0.3e-5
    assert nutrient_bounds(dict(rho_o=1., G_chen=-1.), 1.4, 1e-6)["F"] < b["F"]
    assert nutrient_bounds(dict(rho_o=1., G_chen=0.), 1.4, 1e-5)["F"] == 0.


# ---- the parameter arithmetic and the drop-in classes --------------------------------------------------------------------------
def test_parameters_against_hand_values():
    from LB_D2Q9.reaction_diffusion.surfactant_nutrient_waves import surfactant_nutrient_parameters
    p = surfactant_nutrient_parameters(Lx=3, Ly=1.8, N=10, time_prefactor=1, lam=1, R0=0.5, Dn=0.1, vc=0.5)
    cs2 = np.float64(CS32) ** 2
    assert (p["nx"], p["ny"]) == (30, 18)
    assert p["omega"] == np.float32(1. / (.5 + .25 / cs2)) == np.float32(0.8) and isinstance(p["omega"], np.float32)
    assert p["omega_n"] == np.float32(1. / (.5 + np.float64(np.float32(.1)) / cs2)) == np.float32(1.25)
    assert p["lb_G"] == np.float32(0.01) and isinstance(p["lb_G"], np.float32)
    assert p["scale"] == -0.5 * ((1. / 10) ** 2 / (1. / 10)) and abs(p["scale"] + 0.05) < 1e-15
    q = surfactant_nutrient_parameters(Lx=1.3, Ly=2.9, N=7, time_prefactor=0.7, Dn=0.3, vc=2.)
    dx, dt = 1. / 7, 0.7 * (1. / 7) ** 2
    assert (q["nx"], q["ny"], q["delta_x"], q["delta_t"], q["ulb"]) == (9, 20, dx, dt, dt / dx)
    assert q["omega"] == np.float32((.5 + np.float64(np.float32(.25 * (dt / dx ** 2))) / cs2) ** -1.)
    assert q["omega_n"] == np.float32((.5 + np.float64(np.float32(.3 * (dt / dx ** 2))) / cs2) ** -1.)
    assert q["lb_G"] == np.float32(dt) and q["scale"] == -2. * (dt / dx)
    r = lattice_parameters(1.3, 2.9, 7, vc=2., Dn=0.3, time_prefactor=0.7)
    assert (r["omega"], r["omega_n"], r["lb_G"], r["scale"]) == (q["omega"], q["omega_n"], q["lb_G"], np.float32(q["scale"]))


class _NoEngine(object):
    """stands in for Nutrient_Set: the constants are derived before any handle exists"""

    def __init__(self, *a, **kw):
        self.args, self.kw, self.params = a, kw, {}

    def set_params(self, **kw):
        self.params.update(kw)

    def __getattr__(self, name):
        return lambda *a, **kw: None


@pytest.mark.parametrize("clumpy", (False, True))
def test_dropin_constants_with_the_engine_away(monkeypatch, clumpy):
    from LB_D2Q9.reaction_diffusion import surfactant_nutrient_waves as snw
    monkeypatch.setattr(snw, "Nutrient_Set", _NoEngine)
    kw = dict(Lx=3, Ly=1.8, N=10, time_prefactor=1, lam=1, R0=0.5, Dn=0.1, vc=0.5)
    sim = snw.Clumpy_Surfactant_Nutrient_Wave(rho_o=1.5, G_chen=-0.7, rng=3, **kw) if clumpy else snw.Surfactant_Nutrient_Wave(rng=3, **kw)
    assert (int(sim.nx), int(sim.ny)) == (30, 18) and isinstance(sim.nx, np.int32)
    assert sim.omega == np.float32(0.8) and sim.omega_n == np.float32(1.25) and sim.lb_G == np.float32(0.01)
    assert sim.delta_x == 0.1 and sim.delta_t == 0.1 ** 2 and sim.ulb == sim.delta_t / sim.delta_x
    assert (sim.pop_index, sim.nut_index, sim.num_populations) == (0, 1, 2)
    e = sim.engine
    assert e.args == (30, 18, sim.omega, sim.omega_n) and e.kw["lam"] == 1 and e.kw["dx"] == sim.delta_x and e.kw["device"] == 0
    assert e.params["G"] == sim.lb_G and e.params["scale"] == np.float32(-0.05) and e.params["clumpy"] is clumpy
    if clumpy:
        assert e.params["rho_o"] == np.float32(1.5) and e.params["G_chen"] == np.float32(-0.7)
        assert sim.rho_o == np.float32(1.5) and sim.G_chen == np.float32(-0.7)
    assert snw.cs == CS32 and snw.w.dtype == np.float32
    names = ["rho", "u", "v", "f", "feq", "poisson_solver"] + (["psi", "pseudo_force_x", "pseudo_force_y"] if clumpy else [])
    for name in names:
        assert hasattr(sim, name), name
    assert not hasattr(snw.Surfactant_Nutrient_Wave(rng=3, **kw), "psi") or clumpy
    for name in ("init_hydro", "redo_initial_condition", "update_feq", "init_pop", "move", "move_bcs", "update_u_and_v", "update_hydro",
                 "collide_particles", "update_force", "run"):
        assert callable(getattr(sim, name)), name


def test_engine_is_built_on_the_shared_bases():
    from LB_D2Q9 import coupled, nutrient_set
    assert issubclass(nutrient_set.Nutrient_Set, coupled._Lattice_Set) and issubclass(nutrient_set.Nutrient_Set, coupled._Shared_Velocity)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_exported_bound_and_refuse_null(lbhip):
    from LB_D2Q9 import _native
    assert lbhip.lb_abi_version() == 11 == _native.ABI_VERSION
    text = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    assert re.search(r"#define LB_ABI_VERSION 11\b", text)
    for name in ENTRY_POINTS:
        fn = getattr(lbhip, name)
        assert name in _native.EXPORTS and fn.argtypes is not None and re.search(r"\bint %s\(" % name, text), name
        args = [0 if a in (ct.c_int, ct.c_float) else None for a in fn.argtypes]
        assert fn(*args) == -1 and b"null" in lbhip.lb_last_error(), name      # null arguments: an argument error, not a crash


def test_params_struct_is_the_headers():
    from LB_D2Q9 import _native
    text = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    m = re.search(r"typedef struct \{ float (\w+), (\w+); int32_t (\w+); float (\w+), (\w+); \} lb_nutrient_params;", text)
    assert m and list(m.groups()) == [n for n, _ in _native.NutrientParams._fields_]
    assert ct.sizeof(_native.NutrientParams) == 20
    p = _native.NutrientParams(np.float32(0.01), np.float32(-0.05), 1, np.float32(1.), np.float32(-1.))
    assert (np.float32(p.G), np.float32(p.scale), p.clumpy, p.rho_o, p.G_chen) == (np.float32(0.01), np.float32(-0.05), 1, 1., -1.)


def test_build_lists_the_unit_and_the_documents_no_longer_refuse_it():
    build = open(os.path.join(ROOT, "2d-lb_amd", "build.py")).read()
    assert '"nutrient.cpp"' in build
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    refused = [line for line in text.splitlines() if "Still refused" in line]
    assert refused and all("surfactant_nutrient_waves.py" not in line for line in refused)
    assert any("add_screened_poisson_force" in line for line in refused)
