"""Multicomponent Shan-Chen fluids without a GPU: the numpy model against the fixtures recorded from the reference's C (float32
within the parity contract, float64 to rounding), what the fixtures claim to be, conservation laws of the model, the new ABI
symbols, lb_create's refusals, the drop-in surface."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from multifluid_model import MultifluidModel, force_bound, from_fixture
from scalar_model import contract_tol

RUN_FIXTURES = ("mc_pair_21x13", "mc_pair_open_21x13", "mc_pair_open_5x4", "mc_pair_open_3x3", "mc_sc_open_37x23", "mc_pow_21x13",
                "mc_three_21x13", "mc_self_21x13", "mc_self_open_21x13", "mc_react_21x13")
# fixture name -> model attribute
NAMES = dict(f="f", feq="feq", rho="rho", u="u", v="v", ub="ub", vb="vb", Gx="Gx", Gy="Gy")


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def bounds(m, n, want):
    """The parity contract for n steps (tests/scalar_model.py); u_b takes u's bound, feq takes f's; the bound on G follows from
    rho's through the stencil (multifluid_model.force_bound), per fluid."""
    tol = contract_tol(n)
    out = dict(f=tol["f"], feq=tol["f"], rho=tol["rho"], u=tol["u"], v=tol["v"], ub=tol["u"], vb=tol["v"])
    gb = force_bound(m.interactions, m.g, m.np_, float(np.max(want["rho"])), tol["rho"])
    out["Gx"] = out["Gy"] = gb[None, None, :]
    return out


def compare(label, m, n, have, want, which=None):
    """Print measured / bound for every array, then hold each to its bound."""
    b = bounds(m, n, want)
    keys = [k for k in (which or NAMES) if k in want]
    for k in keys:
        d = np.abs(np.asarray(have[k], np.float64) - np.asarray(want[k], np.float64))
        print("%s: %s %.2e / %.1e" % (label, k, d.max(), np.max(b[k])))
        assert np.all(d <= b[k]), (label, k, float(d.max()), float(np.max(b[k])))


def state(m):
    return {k: getattr(m, a) for k, a in NAMES.items()}


def recorded(d, n, tag=""):
    return {k: d["%s_%d%s" % (k, n, tag)] for k in NAMES if "%s_%d%s" % (k, n, tag) in d}


# what each stage writes (tools/make_golden_multifluid.py)
WRITES = dict(move=("f",), move_bcs=("f",), update_hydro=("rho", "u", "v"), forces=("Gx", "Gy"), update_bary=("ub", "vb"),
              update_feq=("feq",), collide=("f",), react=("f",))


# ---- the model against the fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_model_reproduces_the_reference(name):
    d = golden(name)
    m64, m32 = from_fixture(d, np.float64), from_fixture(d, np.float32)
    done = 0
    for n in d["steps"]:
        m64.run(n - done)
        m32.run(n - done)
        done = int(n)
        want = recorded(d, n)
        for k, a in want.items():
            assert maxdiff(getattr(m64, NAMES[k]), a) <= 1e-12, (name, k, n)
        compare("%s step %d" % (name, n), m32, n, state(m32), want)


def test_model_reproduces_the_reference_stage_by_stage():
    d = golden("mc_phases_21x13")
    m64, m32 = from_fixture(d, np.float64), from_fixture(d, np.float32)
    for stage in MultifluidModel.STAGES:
        for m in (m64, m32):
            with np.errstate(invalid="ignore"):
                getattr(m, stage)()
        want = {k: d["%s_after_%s" % (k, stage)] for k in WRITES[stage]}
        for k, a in want.items():
            assert maxdiff(getattr(m64, NAMES[k]), a) <= 1e-12, (stage, k)
        if "rho" not in want:
            want["rho"] = d["rho_after_update_hydro"]               # (force_bound reads its maximum)
        compare("after " + stage, m32, 1, state(m32), want, which=WRITES[stage])


def test_model_initialize_is_the_references():
    d = golden("mc_init_21x13")
    for T, tag, tol in ((np.float64, "", 1e-12), (np.float32, "", contract_tol(1)["f"])):
        m = MultifluidModel(int(d["nx"]), int(d["ny"]), d["omega"], str(d["bc"]), T)
        m.rho, m.ub, m.vb = d["rho_in"].astype(T), d["ub_in"].astype(T), d["vb_in"].astype(T)
        m.update_feq()
        assert maxdiff(m.feq, d["feq" + tag]) <= tol and maxdiff(d["f" + tag], d["feq" + tag]) == 0


# ---- the fixtures are what they claim to be ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_fixture_is_what_it_claims(name):
    """The recorder's acceptance conditions, re-checked on the file: the reference's own float32 build within the contract of its
    float64 build, G within force_bound, min rho > 0.5, max |u_b| < 0.15; omega from nu as the reference forms it."""
    d = golden(name)
    assert list(d["steps"]) == [1, 5, 20]
    assert np.allclose(d["omega"], 1. / (0.5 + 3. * d["nu"]), rtol=1e-6) and not np.any(np.isclose(d["omega"], 1.))
    m = from_fixture(d, np.float64)
    for n in d["steps"]:
        want, have = recorded(d, n), recorded(d, n, "_f32")
        assert set(have) == set(want) - {"feq"} and "rho" in want and "ub" in want
        compare("%s f32 build, step %d" % (name, n), m, n, have, want, which=list(have))
        assert want["rho"].min() > 0.5 and np.sqrt(want["ub"] ** 2 + want["vb"] ** 2).max() < 0.15
    assert "f_20" in d and d["f0"].shape == (int(d["nx"]), int(d["ny"]), len(d["omega"]), 9)
    if str(d["bc"]) == "zero_gradient":                            # every boundary cell is its interior neighbour's copy
        xs, ys = np.clip(np.arange(int(d["nx"])), 1, int(d["nx"]) - 2), np.clip(np.arange(int(d["ny"])), 1, int(d["ny"]) - 2)
        assert np.array_equal(d["rho_20"], d["rho_20"][xs][:, ys])


def test_fixture_sizes():
    size = lambda n: os.path.getsize(os.path.join(ROOT, "tests", "golden", n))
    largest_pm = max(size(n) for n in os.listdir(os.path.join(ROOT, "tests", "golden")) if n.startswith("pm_"))
    for n in RUN_FIXTURES + ("mc_phases_21x13", "mc_init_21x13"):
        assert size(n + ".npz") <= largest_pm, n


# ---- conservation and closed forms, float64 model --------------------------------------------------------------------------------
def noisy(nx, ny, rhos, seed):
    rng = np.random.default_rng(seed)
    w = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
    return w * np.asarray(rhos)[None, None, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, len(rhos), 9)))


def test_pair_forces_cancel_and_masses_stay():
    m = MultifluidModel(12, 9, (1.25, 0.9, 1.05), "periodic", np.float64)
    m.set_f(noisy(12, 9, (1., 0.9, 0.8), 1))
    m.interactions = [(0, 1, 1., "linear", 0.), (1, 2, 0.6, "shan_chen", 1.), (0, 2, 0.8, "pow", 1.5), (1, 1, -0.2, "linear", 0.)]
    mass0 = m.f.sum(axis=(0, 1, 3))
    for _ in range(5):
        m.step()
        assert abs(m.Gx.sum()) < 1e-13 and abs(m.Gy.sum()) < 1e-13
    assert np.abs(m.f.sum(axis=(0, 1, 3)) - mass0).max() < 1e-11


def test_eating_conserves_the_pair_and_growth_adds_rate_per_cell():
    m = MultifluidModel(10, 7, (1.25, 0.9), "periodic", np.float64)
    m.set_f(noisy(10, 7, (1., 0.9), 2))
    m.reactions = [("eat", 0, 1, 1e-3, 0.5)]
    total0, each0 = m.f.sum(), m.f.sum(axis=(0, 1, 3))
    m.run(4)
    assert abs(m.f.sum() - total0) < 1e-9 and m.f.sum(axis=(0, 1, 3))[0] > each0[0] + 1e-4      # (w rounded to float32: 1e-9)
    g = MultifluidModel(10, 7, (1.25, 0.9), "periodic", np.float64)
    f0 = noisy(10, 7, (1., 0.4), 3)
    g.set_f(f0)
    g.reactions = [("grow", 1, 0.397, 0.403, 2e-3)]
    mass = f0[:, :, 1].sum()
    for _ in range(3):
        g.step()
        inside = int(((g.rho[:, :, 1] > 0.397) & (g.rho[:, :, 1] < 0.403)).sum())
        assert 0 < inside < 70
        mass += 2e-3 * inside * float(g.w.astype(np.float32).astype(np.float64).sum())     # (the kernels round w to float32)
        assert abs(g.f[:, :, 1].sum() - mass) < 1e-9
    assert abs(g.f[:, :, 0].sum() - f0[:, :, 0].sum()) < 1e-11


def test_uniform_fluid_under_constant_g():
    """sum f c = n rho g and u_b = (n - 1/2) g after n steps."""
    m = MultifluidModel(8, 6, (1.25,), "periodic", np.float64)
    m.set_f(np.broadcast_to(0.8 * m.w, (8, 6, 1, 9)))
    m.set_body_force(0, 1e-3, -2e-3)
    for n in range(1, 6):
        m.step()
        _, mx, my = m.moments()
        assert np.abs(mx - n * 0.8 * 1e-3).max() < 1e-15 and np.abs(my + n * 0.8 * 2e-3).max() < 1e-15
        assert np.abs(m.ub - (n - 0.5) * 1e-3).max() < 1e-15 and np.abs(m.vb + (n - 0.5) * 2e-3).max() < 1e-15


def test_self_term_acts_twice():
    """(i, i, G) gives the force of one increment of (i, j, 2 G) between two copies of the fluid."""
    f0 = noisy(9, 8, (0.7,), 4)
    a = MultifluidModel(9, 8, (1.25,), "periodic", np.float64)
    a.set_f(f0)
    a.interactions = [(0, 0, -1.5, "shan_chen", 1.)]
    b = MultifluidModel(9, 8, (1.25, 1.25), "periodic", np.float64)
    b.set_f(np.concatenate([f0, f0], axis=2))
    b.interactions = [(0, 1, -3., "shan_chen", 1.)]
    for m in (a, b):
        m.update_hydro()
        m.forces()
    assert np.abs(a.Gx).max() > 1e-4 and maxdiff(a.Gx[:, :, 0], b.Gx[:, :, 0]) < 1e-15 and maxdiff(a.Gy[:, :, 0], b.Gy[:, :, 1]) < 1e-15


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lb_run_fluids", "lb_set_interactions", "lb_set_reactions", "lb_get_interactions", "lb_get_reactions",
               "lb_update_forces_fluids", "lb_update_bary_fluids", "lb_react_fluids")


def test_new_symbols_exported_and_bound(lbhip):
    from LB_D2Q9 import _native
    assert lbhip.lb_abi_version() == 11 == _native.ABI_VERSION and ct.sizeof(_native.LbParams) == 64
    assert _native.LB_SEM_MULTIFLUID == 9 and ct.sizeof(_native.Interaction) == 24 == ct.sizeof(_native.FluidReaction)
    text = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    assert re.search(r"\bLB_SEM_MULTIFLUID = 9\b", text)
    for name in NEW_SYMBOLS:
        fn = getattr(lbhip, name)
        assert name in _native.EXPORTS and fn.argtypes is not None and re.search(r"\bint %s\(" % name, text), name
        args = [None] + [0 if a is ct.c_int else None for a in fn.argtypes[1:]]
        assert fn(*args) == -1 and b"null" in lbhip.lb_last_error(), name      # a null handle: an argument error, not a crash


def _params(**kw):
    from LB_D2Q9 import _native
    p = _native.LbParams()
    p.nx, p.ny, p.y0, p.local_ny, p.omega = 16, 12, 0, 12, 1.25
    p.semantics, p.bc_mode, p.device = _native.LB_SEM_MULTIFLUID, _native.LB_BC_ZERO_GRADIENT, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, word", [
    (dict(bc_mode=0), b"LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT"),  # every other family with this semantics
    (dict(bc_mode=2), b"LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT"),
    (dict(bc_mode=3), b"LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT"),
    (dict(bc_mode=4), b"LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT"),
    (dict(bc_mode=5), b"LB_BC_PERIODIC and LB_BC_ZERO_GRADIENT"),
    (dict(bc_mode=6), b"LB_BC_DIRICHLET exists"),
    (dict(nx=2), b"at least 3x3"),
    (dict(ny=2, local_ny=2), b"at least 3x3"),
    (dict(bc_mode=1, nx=2), b"at least 3x3"),                      # the periodic box too: a cell needs eight neighbours
    (dict(local_ny=6), b"slab"),
    (dict(y0=2, local_ny=10), b"slab"),
    (dict(flags=1), b"halo"),
    (dict(device=-1), b"CPU"),
    (dict(bc_mode=1, device=-1), b"CPU"),
    (dict(bc_mode=8), b"unknown bc_mode"),
    (dict(semantics=6, bc_mode=1), b"unknown semantics"),          # the two unassigned values stay unknown
    (dict(semantics=8, bc_mode=1), b"unknown semantics"),
    (dict(semantics=10, bc_mode=1), b"unknown semantics"),
    (dict(semantics=3), b"LB_BC_ZERO_GRADIENT exists"),
    (dict(omega=2.5), b"omega"),
])
def test_create_refusals_are_status_codes_with_messages(lbhip, kw, word):
    """Refused before any device is touched: these hold on a box without a GPU."""
    h = ct.c_void_p()
    p = _params(**kw)
    assert lbhip.lb_create(ct.byref(p), ct.byref(h)) == -1 and not h.value          # LB_ERR_ARG
    msg = lbhip.lb_last_error()
    assert word.lower() in msg.lower(), msg
    if kw.get("semantics", 9) == 9 and b"unknown" not in word and b"DIRICHLET" not in word and b"omega" not in word:
        assert b"LB_SEM_MULTIFLUID" in msg, msg


def test_dropin_surface_and_unbuilt_calls():
    """The reference's names; what is not built says so before any handle exists."""
    from LB_D2Q9.multicomponent_multiphase import multi
    from LB_D2Q9.coupled import Shan_Chen_Fluids
    assert multi.num_type is np.float32
    for m in ("add_fluid", "complete_setup", "set_bary_velocity", "update_bary_velocity", "add_constant_g_force", "add_radial_g_force",
              "add_interaction_force", "add_eating_rate", "add_growth", "run", "get_fields", "add_interaction_force_second_belt",
              "add_screened_poisson_force"):
        assert callable(getattr(multi.Simulation_Runner, m)), m
    for m in ("initialize", "init_pop", "update_forces", "update_feq", "move_bcs", "move", "update_hydro", "collide_particles"):
        assert callable(getattr(multi.Fluid, m)), m
    for m in ("run", "set_interactions", "set_reactions", "move", "move_bcs", "update_hydro", "update_forces", "update_bary_velocity",
              "update_feq", "collide_particles", "react", "save_checkpoint", "from_checkpoint"):
        assert callable(getattr(Shan_Chen_Fluids, m)), m
    sim = multi.Simulation_Runner(nx=8, ny=8, num_populations=2)
    assert sim.two_d_global_size == (32, 32) and sim.num_jumpers == 9 and sim.num_populations == 2
    for call in (lambda: multi.Simulation_Runner(nx=8, ny=8, num_populations=4), lambda: multi.Simulation_RunnerD2Q25(nx=8, ny=8),
                 lambda: sim.add_interaction_force_second_belt(0, 1, 1.), lambda: sim.add_screened_poisson_force(0, 1, 2., 1.),
                 lambda: multi.Fluid(sim, 3, 0.1)):
        with pytest.raises(NotImplementedError, match="vdw.*second_belt.*screened_poisson.*D2Q25.*more than 3 fluids.*different"):
            call()
    with pytest.raises(RuntimeError, match="add_fluid"):
        sim.run(1)
