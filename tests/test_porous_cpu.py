"""Forced flow in a porous medium without a GPU: the numpy model against the fixtures recorded from the reference's C (float32
within the parity contract, float64 to rounding), what the fixtures claim to be, the zero-gradient family's defining property,
the new ABI symbols, lb_create's refusals."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from porous_model import PorousModel, force_bound
from scalar_model import contract_tol

RUN_FIXTURES = ("pm_darcy_37x23", "pm_forch_37x23", "pm_open_37x23", "pm_open_5x4", "pm_open_3x3", "pm_radial_21x13")
# fixture name -> model attribute
NAMES = dict(f="f", feq="feq", rho="rho", u="u", v="v", ub="ub", vb="vb", Gx="Gx", Gy="Gy")


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def model_of(d, dtype=np.float32):
    m = PorousModel(int(d["nx"]), int(d["ny"]), d["omega"], d["epsilon"], d["nu_fluid"], d["K"], d["Fe"], str(d["bc"]), dtype)
    if "f0" in d:
        m.set_f(d["f0"])
    m.set_body_force(*d["g"])
    if "field_x" in d:
        m.set_force_field(d["field_x"], d["field_y"])
    return m


def bounds(d, n, want):
    """The parity contract for n steps (tests/scalar_model.py); u_b takes u's bound, feq takes f's; the bound on G follows from
    u's (porous_model.force_bound) plus float32 rounding of G itself."""
    tol = contract_tol(n)
    speed = float(np.sqrt(np.asarray(want["u"], np.float64) ** 2 + np.asarray(want["v"], np.float64) ** 2).max())
    out = dict(f=tol["f"], feq=tol["f"], rho=tol["rho"], u=tol["u"], v=tol["v"], ub=tol["u"], vb=tol["v"])
    for k in ("Gx", "Gy"):
        if k in want:
            out[k] = force_bound(d, speed, tol["u"]) + 1e-7 * float(np.abs(want[k]).max())
    return out


def compare(label, d, n, have, want, which=None):
    """Print measured / bound for every array, then hold each to its bound."""
    b = bounds(d, n, want)
    keys = [k for k in (which or NAMES) if k in want]
    meas = {k: maxdiff(have[k], want[k]) for k in keys}
    print("%s: %s" % (label, ", ".join("%s %.2e / %.1e" % (k, meas[k], b[k]) for k in keys)))
    for k in keys:
        assert meas[k] <= b[k], (label, k, meas[k], b[k])


def state(m):
    return {k: getattr(m, a) for k, a in NAMES.items()}


# ---- the model against the fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_model_follows_reference_fixture(name):
    d = golden(name)
    m, m64 = model_of(d), model_of(d, np.float64)
    done = 0
    for n in [int(s) for s in d["steps"]]:
        m.run(n - done)
        m64.run(n - done)
        done = n
        want = {k: d["%s_%d" % (k, n)] for k in NAMES}
        compare("%s after %d steps, float32 model" % (name, n), d, n, state(m), want)
        for k in NAMES:                                         # float64 against float64: rounding only
            assert maxdiff(getattr(m64, NAMES[k]), want[k]) <= 1e-12, (k, n)


@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_fixture_is_what_it_claims(name):
    """The conditions the recorder accepts a fixture under (tools/make_golden_porous.py), checked on what was written."""
    d = golden(name)
    assert str(d["bc"]) in ("periodic", "zero_gradient") and abs(float(d["omega"]) - 1.) > 0.2
    assert abs(float(d["omega"]) - 1. / (0.5 + 3. * float(d["nu_e"]))) < 1e-12
    for n in [int(s) for s in d["steps"]]:
        want = {k: d["%s_%d" % (k, n)] for k in NAMES}
        assert want["f"].dtype == np.float64 and d["f_%d_f32" % n].dtype == np.float32
        assert want["rho"].min() > 0.5 and np.sqrt(want["u"] ** 2 + want["v"] ** 2).max() < 0.15
        own = {k: d["%s_%d_f32" % (k, n)] for k in NAMES if k != "feq"}
        compare("%s after %d steps, the reference's own float32 build" % (name, n), d, n, own, want, [k for k in NAMES if k != "feq"])


def test_phases_fixture_stage_by_stage():
    d = golden("pm_phases_21x13")
    m, m64 = model_of(d), model_of(d, np.float64)
    for stage in PorousModel.STAGES:
        getattr(m, stage)()
        getattr(m64, stage)()
        want = {k: d["%s_after_%s" % (k, stage)] for k in NAMES if "%s_after_%s" % (k, stage) in d}
        assert want, stage
        full = dict(u=d["u_after_update_hydro"], v=d["v_after_update_hydro"])
        full.update(want)
        if stage in ("move", "move_bcs"):
            for k in want:
                assert np.array_equal(getattr(m, NAMES[k]), want[k].astype(np.float32)), stage         # data movement: exact
        else:
            compare("after %s" % stage, d, 1, state(m), full, list(want))
        for k in want:
            assert maxdiff(getattr(m64, NAMES[k]), want[k]) <= 1e-12, (stage, k)


def test_init_fixture():
    """Pourous_Media.initialize(rho_arr, f_amp = 0): feq from rho and the given u_b, f = feq, then the component velocity and
    the drag alone (no additional force is in the buffers at that point)."""
    d = golden("pm_init_21x13")
    m = model_of(d)
    m.rho, m.ub, m.vb = (np.array(d[k], np.float32) for k in ("rho_in", "ub_in", "vb_in"))
    m.update_feq()
    m.set_f(m.feq)
    m.update_hydro()
    m.set_body_force(0., 0.)
    m.body_force()
    m.update_forces()
    compare("initialize", d, 1, state(m), {k: d[k] for k in NAMES})


@pytest.mark.parametrize("name", ("pm_open_37x23", "pm_open_5x4", "pm_open_3x3", "pm_radial_21x13"))
def test_zero_gradient_boundary_cells_equal_their_interior_source(name):
    """After every step rho, u, v, the populations before the collision -- everything -- of a boundary cell are those of the
    interior cell (clamp(x, 1, nx-2), clamp(y, 1, ny-2)); with a force that depends on position the collision then differs,
    so the claim is made on the moments."""
    d = golden(name)
    nx, ny = int(d["nx"]), int(d["ny"])
    xs, ys = np.clip(np.arange(nx), 1, nx - 2), np.clip(np.arange(ny), 1, ny - 2)
    m = model_of(d)
    for n in range(1, 13):
        m.step()
        for k in ("rho", "u", "v"):
            a = getattr(m, k)
            assert np.array_equal(a, a[xs][:, ys]), (k, n)
    for n in [int(s) for s in d["steps"]]:
        for k in ("rho", "u", "v"):
            a = d["%s_%d" % (k, n)]
            assert np.array_equal(a, a[xs][:, ys]), (k, n)
    if name == "pm_open_3x3":
        assert len(np.unique(d["rho_200"])) == 1                 # every boundary cell copies the one interior cell


def test_uniform_fluid_reaches_darcy_and_forchheimer_states():
    """The float64 model at the parameters of the GPU test of the same name (16 x 8, rho = 1, eps 0.6, nu 0.2, K 2, nu_e 0.1, g 1e-3): u = g K / nu for Fe = 0, the positive root of
    (Fe / sqrt(K)) u^2 + (nu / K) u - g = 0 otherwise, in both families."""
    g, K, nu = 1e-3, 2., 0.2
    for bc in ("periodic", "zero_gradient"):
        for Fe in (0., 0.5):
            m = PorousModel(16, 8, 1. / (0.5 + 3. * 0.1), 0.6, nu, K, Fe, bc, np.float64)
            m.set_f(np.broadcast_to(m.w, (16, 8, 9)))
            m.set_body_force(g, 0.)
            m.run(300)
            a, b = Fe / np.sqrt(K), nu / K
            want = g / b if Fe == 0 else (-b + np.sqrt(b * b + 4. * a * g)) / (2. * a)
            assert np.abs(m.ub / want - 1.).max() < 1e-7, (bc, Fe)
            assert np.abs(m.vb).max() < 1e-15 and np.ptp(m.rho) < 1e-12


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lb_set_porous", "lb_set_body_force", "lb_set_force_field", "lb_get_force", "lb_set_force", "lb_set_bary_velocity",
               "lb_get_bary_velocity", "lb_update_forces", "lb_update_bary_velocity")


def test_new_symbols_exported_and_bound(lbhip):
    from LB_D2Q9 import _native
    assert lbhip.lb_abi_version() == 11 == _native.ABI_VERSION and ct.sizeof(_native.LbParams) == 64
    assert _native.BC_NAMES["zero_gradient"] == _native.LB_BC_ZERO_GRADIENT == 7
    text = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    assert re.search(r"\bLB_SEM_POROUS = %d\b" % _native.LB_SEM_POROUS, text) and re.search(r"\bLB_BC_ZERO_GRADIENT = 7\b", text)
    for name in NEW_SYMBOLS:
        fn = getattr(lbhip, name)
        assert name in _native.EXPORTS and fn.argtypes is not None, name
        args = [None] + [None if a is ct.c_void_p else 0 for a in fn.argtypes[1:]]
        assert fn(*args) == -1 and b"null" in lbhip.lb_last_error(), name      # a null handle: an argument error, not a crash


def _params(**kw):
    from LB_D2Q9 import _native
    p = _native.LbParams()
    p.nx, p.ny, p.y0, p.local_ny, p.omega = 16, 12, 0, 12, 1.25
    p.semantics, p.bc_mode, p.device = _native.LB_SEM_POROUS, _native.LB_BC_ZERO_GRADIENT, 0
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
    (dict(semantics=0), b"LB_BC_ZERO_GRADIENT exists"),            # this family with every other semantics
    (dict(semantics=1), b"LB_BC_ZERO_GRADIENT exists"),
    (dict(semantics=2), b"LB_BC_ZERO_GRADIENT exists"),
    (dict(semantics=3), b"LB_BC_ZERO_GRADIENT exists"),
    (dict(semantics=4), b"LB_BC_ZERO_GRADIENT exists"),
    (dict(semantics=5), b"LB_BC_ZERO_GRADIENT exists"),
    (dict(nx=2), b"at least 3x3"),                                 # no interior cell
    (dict(ny=2, local_ny=2), b"at least 3x3"),
    (dict(local_ny=6), b"slab"),
    (dict(y0=2, local_ny=10), b"slab"),
    (dict(flags=1), b"halo"),
    (dict(device=-1), b"CPU"),
    (dict(bc_mode=1, device=-1), b"CPU"),
    (dict(bc_mode=8), b"unknown bc_mode"),
    (dict(semantics=8, bc_mode=1), b"unknown semantics"),
    (dict(omega=2.5), b"omega"),
])
def test_create_refusals_are_status_codes_with_messages(lbhip, kw, word):
    """Refused before any device is touched: these hold on a box without a GPU."""
    h = ct.c_void_p()
    p = _params(**kw)
    assert lbhip.lb_create(ct.byref(p), ct.byref(h)) == -1 and not h.value          # LB_ERR_ARG
    msg = lbhip.lb_last_error()
    assert word.lower() in msg.lower(), msg


def test_dropin_surface_and_unbuilt_calls():
    """The reference's names; what is not built says so before any handle exists."""
    from LB_D2Q9.porous_media import single_component as sc
    assert sc.num_type is np.float32
    for m in ("add_fluid", "complete_setup", "set_bary_velocity", "update_bary_velocity", "add_constant_body_force",
              "add_radial_body_force", "run", "add_eating_rate", "add_interaction_force", "add_interaction_force_second_belt"):
        assert callable(getattr(sc.Simulation_Runner, m)), m
    for m in ("initialize", "init_pop", "update_forces", "update_feq", "move_bcs", "move", "update_hydro", "collide_particles"):
        assert callable(getattr(sc.Pourous_Media, m)), m
    with pytest.raises(NotImplementedError, match="several fluids"):
        sc.Simulation_Runner(nx=8, ny=8, num_populations=2)
    sim = sc.Simulation_Runner(nx=8, ny=8)
    assert sim.two_d_global_size == (32, 32) and sim.num_jumpers == 9
    for call in (lambda: sim.add_interaction_force(0, 0, 1.), lambda: sim.add_interaction_force_second_belt(0, 0, 1.),
                 lambda: sim.add_eating_rate(0, 0, 1.)):
        with pytest.raises(NotImplementedError, match="Shan-Chen"):
            call()
