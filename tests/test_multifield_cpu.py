"""Coupled scalar lattices without a GPU: the numpy model against the fixtures recorded from the reference's C and against a
literal push + move_bcs restatement, Fisher_Expansion's parameter arithmetic, the new ABI symbols, lb_create's refusals."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from multifield_model import CORNER_LINKS, CX, CY, MultifieldModel, contract_tol

RUN_FIXTURES = ("mf_box_37x23", "mf_fisher_37x23", "mf_box_5x4")


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def model_of(d, bc="box"):
    m = MultifieldModel(int(d["nx"]), int(d["ny"]), d["omega"], d["G"], bc)
    m.set_fields(np.zeros(d["f0"].shape[:3], np.float32), d["u"], d["v"])
    m.set_f(d["f0"])
    if int(d["corner_zero"]):
        m.set_corner_state(np.zeros((m.nf, 8), np.float32))
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
        meas = dict(f=maxdiff(m.f, d["f_%d" % n]), rho=maxdiff(m.rho, d["rho_%d" % n]))
        print("%s after %d steps, measured / bound: f %.2e / %.1e, rho %.2e / %.1e" % (name, n, meas["f"], tol["f"], meas["rho"], tol["rho"]))
        assert meas["f"] <= tol["f"] and meas["rho"] <= tol["rho"]


def test_fixtures_are_the_cases_they_claim():
    d = golden("mf_box_37x23")
    assert d["f0"].shape == (37, 23, 3, 9) and len(set(d["omega"].tolist())) == 3 and np.all((d["omega"] > 0.8) & (d["omega"] < 1.4))
    assert np.allclose(d["G"], (0.01, 0.02, 0.)) and float(d["f0"].sum(axis=(2, 3)).max()) < 1.
    lim = np.float32(0.07)                                  # (the arrays are float32)
    assert 0. < np.abs(d["u"]).max() <= lim and 0. < np.abs(d["v"]).max() <= lim and np.ptp(d["u"]) > 0.
    d = golden("mf_fisher_37x23")
    assert d["f0"].shape == (37, 23, 2, 9) and not d["u"].any() and not d["v"].any() and np.allclose(d["G"], (0.01, 0.012))
    assert int(d["corner_zero"]) == 1 and list(d["steps"]) == [1, 200, 1000]
    assert golden("mf_box_5x4")["f0"].shape == (5, 4, 2, 9) and list(golden("mf_box_5x4")["steps"]) == [1, 7]


def test_model_phases_follow_reference_fixture():
    d = golden("mf_phases_21x13")
    m = model_of(d)
    tol = contract_tol(1)
    m.move()
    assert np.array_equal(m.f, d["f_move"])                   # streaming and bounce-back move values, they compute nothing
    m.move_bcs()
    assert np.array_equal(m.f, d["f_bcs"])
    m.update_hydro()
    assert maxdiff(m.rho, d["rho_hydro"]) <= tol["rho"]
    m.update_feq()
    assert maxdiff(m.feq, d["feq_feq"]) <= tol["f"]
    m.collide_particles()
    assert maxdiff(m.f, d["f_collide"]) <= tol["f"]


def test_box_never_writes_eight_corner_links():
    """The fact the corner state rests on: after move + move_bcs those links hold what f_streamed held (the fixture shows it)."""
    d = golden("mf_phases_21x13")
    for k, x, y in CORNER_LINKS:
        assert np.array_equal(d["f_bcs"][x, y, :, k], d["f0"][x, y, :, k])
    m = model_of(d)
    c = m.get_corner_state()
    assert c.shape == (2, 8) and np.array_equal(c[:, 0], d["f0"][0, 0, :, 6]) and np.array_equal(c[:, 7], d["f0"][-1, -1, :, 8])
    m.set_corner_state(c + 1.)
    assert np.array_equal(m.get_corner_state(), c + 1.)


# ---- the model against the reference's own formulation, restated literally: push streaming into a second buffer, copy back,
#      move_bcs in place cell by cell ------------------------------------------------------------------------------------------
def literal_move(f, fs):
    nx, ny = f.shape[:2]
    for k in range(9):
        for x in range(nx):
            for y in range(ny):
                sx, sy = x + CX[k], y + CY[k]
                if 0 <= sx < nx and 0 <= sy < ny:
                    fs[sx, sy, :, k] = f[x, y, :, k]
    f[...] = fs


def literal_move_bcs(f):
    nx, ny = f.shape[:2]
    for x in range(nx):
        for y in range(ny):
            left, right = x == 0 and 1 <= y < ny - 1, x == nx - 1 and 1 <= y < ny - 1
            top, bottom = y == ny - 1 and 1 <= x < nx - 1, y == 0 and 1 <= x < nx - 1
            f1, f2, f3, f4, f5, f6, f7, f8 = (f[x, y, :, k].copy() for k in range(1, 9))
            put = lambda **kw: [f.__setitem__((x, y, slice(None), int(k[1])), val) for k, val in kw.items()]
            if top: put(f7=f5, f4=f2, f8=f6)
            if bottom: put(f2=f4, f5=f7, f6=f8)
            if right: put(f3=f1, f6=f8, f7=f5)
            if left: put(f1=f3, f5=f7, f8=f6)
            if x == 0 and y == ny - 1: put(f1=f3, f4=f2, f8=f6)
            if x == nx - 1 and y == ny - 1: put(f3=f1, f4=f2, f7=f5)
            if x == nx - 1 and y == 0: put(f2=f4, f3=f1, f6=f8)
            if x == 0 and y == 0: put(f1=f3, f2=f4, f5=f7)


@pytest.mark.parametrize("shape", [(7, 5), (3, 3), (2, 4)])
def test_pull_form_equals_literal_push_and_move_bcs(shape):
    nx, ny = shape
    rng = np.random.default_rng(5)
    f0 = (0.02 + 0.05 * rng.uniform(size=(nx, ny, 2, 9))).astype(np.float32)
    u, v = (0.05 * rng.uniform(-1, 1, (nx, ny))).astype(np.float32), (0.05 * rng.uniform(-1, 1, (nx, ny))).astype(np.float32)
    m = MultifieldModel(nx, ny, (0.9, 1.3), (0.02, 0.01))
    lit = MultifieldModel(nx, ny, (0.9, 1.3), (0.02, 0.01))
    for b in (m, lit):
        b.set_fields(np.zeros((nx, ny, 2), np.float32), u, v)
        b.set_f(f0)
    fs = f0.copy()                                           # the literal's f_streamed
    for step in range(20):
        m.step()
        literal_move(lit.f, fs)
        literal_move_bcs(lit.f)
        lit.update_hydro(); lit.update_feq(); lit.collide_particles()
        assert np.array_equal(m.f, lit.f) and np.array_equal(m.rho, lit.rho), step


def test_one_field_is_the_scalar_model():
    """With one field rho_tot = rho: the periodic family is scalar_model.py's, bit for bit."""
    from scalar_model import ScalarModel
    rng = np.random.default_rng(6)
    f0 = (0.05 + 0.05 * rng.uniform(size=(9, 6, 1, 9))).astype(np.float32)
    u = (0.05 * rng.uniform(-1, 1, (9, 6))).astype(np.float32)
    a, b = MultifieldModel(9, 6, [1.1], [0.02], "periodic"), ScalarModel(9, 6, 1.1, 0.02, "periodic")
    a.set_fields(np.zeros((9, 6, 1), np.float32), u, -u); a.set_f(f0)
    b.set_fields(np.zeros((9, 6), np.float32), u, -u); b.set_f(f0[:, :, 0, :])
    a.run(10); b.run(10)
    assert np.array_equal(a.f[:, :, 0, :], b.f)


# ---- Fisher_Expansion's parameter arithmetic (worked out from the formulas of deterministic_fisher_waves.py) ----------------
def test_fisher_expansion_parameters():
    from LB_D2Q9.advecting_range_expansion import deterministic_fisher_waves as fw
    p = fw.fisher_expansion_parameters(Lx=8., Ly=4., vx=1., vy=2., vc=4., mu_standard=4., mu_list=[4., 2.], D_standard=1.,
                                       D_list=[1., 0.5], time_prefactor=0.5, N=10)
    # L = 2 sqrt(1 / 4) = 1, T = 0.25, vf = 4; delta_x = 0.1, delta_t = 0.005, ulb = 0.05
    assert p["L"] == pytest.approx(1.) and p["T"] == pytest.approx(0.25) and p["vf"] == pytest.approx(4.)
    assert p["delta_t"] == pytest.approx(0.005) and p["ulb"] == pytest.approx(0.05)
    assert p["lb_G"].dtype == np.float32 and p["lb_G"] == pytest.approx([0.005, 0.0025])
    # lb_D = D / 4 * 0.5 = (0.125, 0.0625); omega = 1 / (0.5 + 3 lb_D)
    assert p["lb_D_population"] == pytest.approx([0.125, 0.0625]) and p["omega"] == pytest.approx([1. / 0.875, 1. / 0.6875])
    assert (p["lx"], p["ly"], p["nx"], p["ny"]) == (80, 40, 82, 42)
    # vc / vf = 1: lattice velocity = ulb (vx, vy) / vc
    assert p["lb_vx"] == pytest.approx(0.05 * 0.25) and p["lb_vy"] == pytest.approx(0.05 * 0.5)
    q = fw.fisher_expansion_parameters(mu_list=[1.], D_list=[1.], N=5)        # no flow: vc = 0 gives zero velocity, not NaN
    assert q["lb_vx"] == 0. and q["lb_vy"] == 0. and (q["nx"], q["ny"]) == (2, 2)


def test_inoculation_stripes():
    from LB_D2Q9.advecting_range_expansion import deterministic_fisher_waves as fw
    rho = fw.inoculation_stripes(10, 6, 3, [0.33, 0.33, 0.34], [2, 0, 1], 2)
    assert rho.shape == (10, 6, 3) and rho.dtype == np.float32 and np.isfortran(rho)
    assert rho[0:3, 0:2, 2].all() and rho[3:6, 0:2, 0].all() and rho[6:10, 0:2, 1].all()      # the last stripe takes the rest
    assert rho.sum() == 10 * 2 and not rho[:, 2:, :].any() and rho.sum(axis=2).max() == 1.


def test_class_has_the_reference_surface():
    from LB_D2Q9.advecting_range_expansion.deterministic_fisher_waves import Fisher_Expansion
    from LB_D2Q9.coupled import Coupled_Scalars
    for m in ("init_hydro", "update_feq", "init_f", "move", "move_bcs", "update_hydro", "collide_particles", "run", "get_fields",
              "get_nondim_fields", "get_physical_fields"):
        assert callable(getattr(Fisher_Expansion, m)), m
    for m in ("set_f", "set_fields", "set_velocity_from", "init_pop", "move", "move_bcs", "update_hydro", "update_feq",
              "collide_particles", "run", "step", "get_fields", "check", "get_corner_state", "set_corner_state", "close"):
        assert callable(getattr(Coupled_Scalars, m)), m


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lb_run_coupled", "lb_collide_coupled")


def test_new_symbols_exported_and_bound(lbhip):
    from LB_D2Q9 import _native
    assert lbhip.lb_abi_version() == 11 == _native.ABI_VERSION and ct.sizeof(_native.LbParams) == 64
    assert _native.LB_SEM_MULTIFIELD == 4 and _native.LB_BC_BOX == 5 and _native.BC_NAMES["box"] == 5
    for name in NEW_SYMBOLS:
        fn = getattr(lbhip, name)
        assert name in _native.EXPORTS and fn.argtypes is not None, name
        args = [None] + [1] * (len(fn.argtypes) - 1)
        assert fn(*args) == -1                              # no set at all: an argument error, not a crash
        one = (ct.c_void_p * 1)(None)                       # a null handle in the set
        assert fn(one, *([1] * (len(fn.argtypes) - 1))) == -1 and b"null" in lbhip.lb_last_error()


def _params(**kw):
    from LB_D2Q9 import _native
    p = _native.LbParams()
    p.nx, p.ny, p.y0, p.local_ny, p.omega = 16, 12, 0, 12, 1.0
    p.semantics, p.bc_mode, p.device = _native.LB_SEM_MULTIFIELD, _native.LB_BC_BOX, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, word", [
    (dict(bc_mode=0), b"LB_BC_PERIODIC and LB_BC_BOX"),            # PIPE, CAVITY, VELOCITY_INLET with this semantics
    (dict(bc_mode=2), b"LB_BC_PERIODIC and LB_BC_BOX"),
    (dict(bc_mode=3), b"LB_BC_PERIODIC and LB_BC_BOX"),
    (dict(bc_mode=4), b"LB_BC_OPEN"),                              # OPEN is LB_SEM_DIFFUSION's
    (dict(semantics=0), b"bc_mode LB_BC_BOX"),                     # LB_BC_BOX with every other semantics
    (dict(semantics=1), b"bc_mode LB_BC_BOX"),
    (dict(semantics=2), b"bc_mode LB_BC_BOX"),
    (dict(semantics=3), b"bc_mode LB_BC_BOX"),
    (dict(local_ny=6), b"slab"),                                   # a slab
    (dict(y0=2, local_ny=10), b"slab"),
    (dict(flags=1), b"halo"),                                      # LB_FLAG_HALO
    (dict(device=-1), b"CPU"),                                     # LB_DEVICE_CPU
    (dict(bc_mode=1, device=-1), b"CPU"),
    (dict(bc_mode=6), b"unknown bc_mode"),
    (dict(semantics=5, bc_mode=1), b"unknown semantics"),
])
def test_create_refusals_are_status_codes_with_messages(lbhip, kw, word):
    """Refused before any device is touched: these hold on a box without a GPU."""
    h = ct.c_void_p()
    p = _params(**kw)
    assert lbhip.lb_create(ct.byref(p), ct.byref(h)) == -1 and not h.value          # LB_ERR_ARG
    msg = lbhip.lb_last_error()
    assert word.lower() in msg.lower(), msg
