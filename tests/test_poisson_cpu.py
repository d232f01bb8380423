"""The LB Poisson solver without a GPU: the numpy model against the fixtures recorded from the reference's C and against a
literal push + copy + cell-by-cell move_bcs restatement, what the fixtures claim to be, the stopping rule in the recorded
ratio series, the drop-in's parameter arithmetic, the new ABI symbols, lb_create's refusals."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden
from multifield_model import CORNER_LINKS
from poisson_model import CX, CY, F, W, PoissonModel, contract_tol

RUN_FIXTURES = ("ps_box_37x23", "ps_noise_37x23", "ps_box_5x4")
TOLERANCE = 1e-4            # of the stopping tests, here and on the GPU


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def model_of(d, dtype=F):
    m = PoissonModel(int(d["nx"]), int(d["ny"]), d["omega"], d["rho_on_boundary"], d["react_factor"], dtype)
    m.set_f(d["f0"])
    m.set_source(d["scaled_source"])
    return m


def first_below(d, tolerance=TOLERANCE):
    """n*: the first recorded iteration whose ratio is < tolerance, and its index in the series"""
    i = int(np.argmax(d["ratios"] < tolerance))
    assert d["ratios"][i] < tolerance
    return int(d["ratio_iters"][i]), i


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
        tol = contract_tol(n)
        tol["feq"] = tol["f"]
        want = dict(f=d["f_%d" % n], rho=d["rho_%d" % n], feq=d["feq_%d" % n])
        meas = {k: maxdiff(getattr(m, k), want[k]) for k in want}
        own = {k: maxdiff(getattr(m64, k), want[k]) for k in want}      # the reference's float32 against a float64 evaluation
        print("%s after %d iterations, model / reference's own rounding / bound: %s"
              % (name, n, ", ".join("%s %.2e / %.2e / %.1e" % (k, meas[k], own[k], tol[k]) for k in want)))
        for k in want:
            assert meas[k] <= tol[k], (k, meas[k], tol[k])
            assert own[k] <= 0.5 * tol[k], (k, own[k], tol[k])          # (else the fixture's run would have to be shortened)


def test_model_ratio_series_follows_reference():
    """The model's convergence ratio against the recorded one while it is far above float32's noise floor."""
    d = golden("ps_box_37x23")
    m = model_of(d)
    for n, want in zip(d["ratio_iters"][:300], d["ratios"][:300]):
        while m.iterations < n:
            m.step()
        if n == 2:
            assert np.isinf(want) and np.isinf(m.ratio)      # x / 0: rho_before is the zero lattice's
        else:
            assert abs(m.ratio - want) <= 1e-3 * want, (n, m.ratio, want)


def test_model_phases_follow_reference_fixture():
    d = golden("ps_phases_21x13")
    m = model_of(d)
    tol = contract_tol(1)
    m.move()
    assert np.array_equal(m.f, d["f_move"])                 # streaming moves values, it computes nothing
    m.move_bcs()
    # the rule's arithmetic is restated operation for operation (five links in ascending order, + (w0 - 1) rho_b, a division by the
    # three weights' float32 sum, w_k R), so the walls agree bit for bit as well; the bound is what the contract would allow
    assert maxdiff(m.f, d["f_bcs"]) <= tol["f"] and np.array_equal(m.f, d["f_bcs"])
    m.update_hydro()
    assert maxdiff(m.rho, d["rho_hydro"]) <= tol["rho"]
    m.update_feq()
    assert maxdiff(m.feq, d["feq_feq"]) <= tol["f"]
    m.collide_particles()
    assert maxdiff(m.f, d["f_collide"]) <= tol["f"]


# ---- the fixtures are what they claim --------------------------------------------------------------------------------------
def test_fixtures_are_the_cases_they_claim():
    d = golden("ps_box_37x23")
    assert d["f0"].shape == (37, 23, 9) and not d["f0"].any() and list(d["steps"]) == [1, 10, 200]
    assert (float(d["delta_x"]), float(d["delta_t"]), float(d["omega"]), float(d["rho_on_boundary"])) == (1., 0.5, 0.5, 0.)
    assert d["source"].shape == (37, 23) and d["source"].min() > 0 and np.ptp(d["source"]) > 0
    assert 0.1 <= np.abs(d["rho_200"]).max() <= 1.
    assert list(d["ratio_iters"]) == list(range(2, 601)) and d["ratios"].dtype == np.float64 and d["ratios"].shape == (599,)
    assert not np.isfinite(d["ratios"][0]) and np.all(np.isfinite(d["ratios"][1:]))       # iteration 2: x / 0 on the zero lattice
    d = golden("ps_noise_37x23")
    assert d["f0"].shape == (37, 23, 9) and float(d["delta_t"]) == 1. and abs(float(d["omega"]) - 1. / 3.5) < 1e-7
    assert float(d["rho_on_boundary"]) == np.float32(0.3) and list(d["steps"]) == [1, 10, 200] and d["source"].min() > 0
    assert 0.1 <= np.abs(d["rho_200"]).max() <= 1.
    assert np.all(model_of(d).get_corner_state() != 0)                                    # a noisy start: the corner state is not zero
    d = golden("ps_box_5x4")
    assert d["f0"].shape == (5, 4, 9) and list(d["steps"]) == [1, 7] and 0.1 <= np.abs(d["rho_7"]).max() <= 1.
    assert np.all(model_of(d).get_corner_state() != 0)
    d = golden("ps_phases_21x13")
    assert d["f0"].shape == (21, 13, 9) and float(d["rho_on_boundary"]) != 0.
    for k in ("f_move", "f_bcs", "feq_feq", "f_collide"):
        assert d[k].shape == (21, 13, 9)
    d = golden("ps_grad_21x13")
    assert d["rho"].shape == d["u"].shape == d["v"].shape == (21, 13) and np.abs(d["u"]).max() > 0 and np.abs(d["v"]).max() > 0
    for name in RUN_FIXTURES + ("ps_phases_21x13",):
        d = golden(name)
        assert np.array_equal(d["scaled_source"], d["source"] * np.float32(d["lb_D"] * d["delta_t"]))
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", name + ".npz")) < 400 * 1024


def test_box_never_writes_eight_corner_links():
    """The fact the corner state rests on: after move + move_bcs those links hold what f_streamed held (the fixture shows it) --
    LB_BC_BOX's eight links in LB_BC_BOX's order."""
    d = golden("ps_phases_21x13")
    for k, x, y in CORNER_LINKS:
        assert d["f_bcs"][x, y, k] == d["f0"][x, y, k] != 0.
    m = model_of(d)
    c = m.get_corner_state()
    assert c.shape == (8,) and c[0] == d["f0"][0, 0, 6] and c[7] == d["f0"][-1, -1, 8]
    m.set_corner_state(c + 1.)
    assert np.array_equal(m.get_corner_state(), c + 1.)


# ---- the model against the reference's own formulation, restated literally: push streaming into a second buffer, copy back,
#      move_bcs in place cell by cell, branch by branch (D2Q9_poisson.cl:115-254) -------------------------------------------------
def literal_move(f, fs):
    nx, ny = f.shape[:2]
    for k in range(9):
        for x in range(nx):
            for y in range(ny):
                sx, sy = x + CX[k], y + CY[k]
                if 0 <= sx < nx and 0 <= sy < ny:
                    fs[sx, sy, k] = f[x, y, k]
    f[...] = fs


def literal_move_bcs(f, rho_b):
    nx, ny = f.shape[:2]
    w = W
    wall = (F(-1) + w[0]) * F(rho_b)
    for x in range(nx):
        for y in range(ny):
            left, right = x == 0 and 1 <= y < ny - 1, x == nx - 1 and 1 <= y < ny - 1
            top, bottom = y == ny - 1 and 1 <= x < nx - 1, y == 0 and 1 <= x < nx - 1
            q = [None] + [f[x, y, k] for k in range(1, 9)]

            def rule(read, write):
                total = q[read[0]]
                for k in read[1:]:
                    total = total + q[k]
                R = -(total + wall) / ((w[write[0]] + w[write[1]]) + w[write[2]])
                for k in write:
                    f[x, y, k] = w[k] * R
            if top: rule((1, 2, 3, 5, 6), (4, 7, 8))
            if right: rule((1, 2, 4, 5, 8), (3, 6, 7))
            if bottom: rule((1, 3, 4, 7, 8), (2, 5, 6))
            if left: rule((2, 3, 4, 6, 7), (1, 5, 8))
            if x == 0 and y == 0: rule((3, 4, 6, 7, 8), (1, 2, 5))
            if x == nx - 1 and y == 0: rule((1, 4, 5, 7, 8), (2, 3, 6))
            if x == 0 and y == ny - 1: rule((2, 3, 5, 6, 7), (1, 4, 8))
            if x == nx - 1 and y == ny - 1: rule((1, 2, 5, 6, 8), (3, 4, 7))


@pytest.mark.parametrize("shape", [(7, 5), (21, 13)])
def test_pull_form_equals_literal_push_copy_and_move_bcs(shape):
    nx, ny = shape
    rng = np.random.default_rng(7)
    f0 = (W * 0.3 * (1. + 0.2 * rng.uniform(-1, 1, (nx, ny, 9)))).astype(F)
    src = (0.001 * rng.uniform(size=(nx, ny))).astype(F)
    m, lit = PoissonModel(nx, ny, 0.7, 0.3, 0.5), PoissonModel(nx, ny, 0.7, 0.3, 0.5)
    for b in (m, lit):
        b.set_f(f0)
        b.set_source(src)
    fs = f0.copy()                                           # the literal's f_streamed
    for step in range(12 if nx > 10 else 30):
        m.step()
        literal_move(lit.f, fs)
        for _ in range(2):                                   # (the reference runs the rule nine times over: it is idempotent)
            literal_move_bcs(lit.f, 0.3)
        lit.update_hydro(); lit.update_feq(); lit.collide_particles()
        assert np.array_equal(m.f, lit.f) and np.array_equal(m.rho, lit.rho), step


# ---- the stopping rule ---------------------------------------------------------------------------------------------------
def test_recorded_ratio_series_fixes_the_stop():
    """n* of the GPU's stopping tests: the reference's first iteration with ratio < 1e-4.  The ratios on either side of the
    threshold are more than 1 % away from it, a thousand times what any float32 summation order of 851 cells can move them by:
    a solver stops AT n* or it is wrong -- there is no window to allow."""
    d = golden("ps_box_37x23")
    n_star, i = first_below(d)
    before, at = float(d["ratios"][i - 1]), float(d["ratios"][i])
    print("n* = %d, ratio at n* - 1: %.6e, at n*: %.6e" % (n_star, before, at))
    assert 100 <= n_star <= 400 and int(d["ratio_iters"][i - 1]) == n_star - 1
    assert before > 1.01 * TOLERANCE and at < 0.99 * TOLERANCE
    assert np.all(d["ratios"][1:i] >= TOLERANCE)            # nothing earlier is below (inf at iteration 2 included)
    m = model_of(d)                                          # and the model's own loop stops there
    done, converged, ratio = m.solve(600, TOLERANCE)
    assert (done, converged) == (n_star, True) and abs(ratio - at) <= 1e-3 * at
    # inf and NaN count as "not converged": the zero lattice with a zero source never stops
    z = PoissonModel(9, 7, 0.5)
    assert z.solve(5, TOLERANCE)[:2] == (5, False) and np.isnan(z.ratio)


# ---- the drop-in's parameter arithmetic ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES + ("ps_phases_21x13",))
def test_dropin_parameter_arithmetic(name):
    from LB_D2Q9.poisson.solver import Poisson_Solver, poisson_parameters
    d = golden(name)
    p = poisson_parameters(float(d["delta_t"]), float(d["delta_x"]))
    for k in ("lb_D", "omega", "react_factor"):
        assert p[k].dtype == np.float32 and p[k] == d[k], k
    # the factor is applied twice: once by update_source on the host, once more in the collision
    assert p["source_scale"] == np.float32(d["lb_D"] * d["delta_t"]) == p["react_factor"]
    assert np.array_equal(d["source"] * p["source_scale"], d["scaled_source"])
    for m in ("run", "update_source", "update_negative_gradient", "move", "move_bcs", "update_hydro", "update_feq",
              "collide_particles", "init_pop", "get_fields", "set_D_and_omega"):
        assert callable(getattr(Poisson_Solver, m)), m


def test_dropin_omega_values():
    from LB_D2Q9.poisson import poisson_parameters
    assert poisson_parameters(0.5, 1.)["omega"] == np.float32(0.5) and poisson_parameters(0.5, 1.)["lb_D"] == np.float32(0.5)
    assert poisson_parameters(1., 1.)["omega"] == np.float32(1. / 3.5)
    assert poisson_parameters(0.25, 0.5)["lb_D"] == np.float32(1.) and poisson_parameters(0.25, 0.5)["ulb"] == np.float32(0.5)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lb_set_poisson", "lb_set_source", "lb_get_source", "lb_solve", "lb_solve_reset", "lb_get_solve_state",
               "lb_set_solve_state", "lb_gradient")


def test_new_symbols_exported_and_bound(lbhip):
    from LB_D2Q9 import _native
    assert lbhip.lb_abi_version() == 11 == _native.ABI_VERSION and ct.sizeof(_native.LbParams) == 64
    assert _native.LB_SEM_POISSON == 5 and _native.LB_BC_DIRICHLET == 6 and _native.BC_NAMES["dirichlet"] == 6
    text = open(os.path.join(ROOT, "include", "lb_hip.h")).read()
    assert re.search(r"\bLB_SEM_POISSON = 5\b", text) and re.search(r"\bLB_BC_DIRICHLET = 6\b", text)
    for name in NEW_SYMBOLS:
        fn = getattr(lbhip, name)
        assert name in _native.EXPORTS and fn.argtypes is not None, name
        args = [None] + [None if hasattr(a, "contents") or a is ct.c_void_p else 0 for a in fn.argtypes[1:]]
        assert fn(*args) == -1 and b"null" in lbhip.lb_last_error(), name      # a null handle: an argument error, not a crash


def _params(**kw):
    from LB_D2Q9 import _native
    p = _native.LbParams()
    p.nx, p.ny, p.y0, p.local_ny, p.omega = 16, 12, 0, 12, 0.5
    p.semantics, p.bc_mode, p.device = _native.LB_SEM_POISSON, _native.LB_BC_DIRICHLET, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw, word", [
    (dict(bc_mode=0), b"LB_BC_DIRICHLET only"),                    # every other family with this semantics
    (dict(bc_mode=1), b"LB_BC_DIRICHLET only"),
    (dict(bc_mode=2), b"LB_BC_DIRICHLET only"),
    (dict(bc_mode=3), b"LB_BC_DIRICHLET only"),
    (dict(bc_mode=4), b"LB_BC_DIRICHLET only"),                    # (OPEN is LB_SEM_DIFFUSION's, BOX is LB_SEM_MULTIFIELD's)
    (dict(bc_mode=5), b"LB_BC_DIRICHLET only"),
    (dict(semantics=0), b"LB_BC_DIRICHLET exists"),                # this family with every other semantics
    (dict(semantics=1), b"LB_BC_DIRICHLET exists"),
    (dict(semantics=2), b"LB_BC_DIRICHLET exists"),
    (dict(semantics=3), b"LB_BC_DIRICHLET exists"),
    (dict(semantics=4), b"LB_BC_DIRICHLET exists"),
    (dict(local_ny=6), b"slab"),                                   # a slab
    (dict(y0=2, local_ny=10), b"slab"),
    (dict(flags=1), b"halo"),                                      # LB_FLAG_HALO
    (dict(device=-1), b"CPU"),                                     # LB_DEVICE_CPU
    (dict(bc_mode=7), b"unknown bc_mode"),
    (dict(semantics=6), b"LB_BC_DIRICHLET exists"),
    (dict(semantics=6, bc_mode=1), b"unknown semantics"),
    (dict(omega=2.5), b"omega"),
])
def test_create_refusals_are_status_codes_with_messages(lbhip, kw, word):
    """Refused before any device is touched: these hold on a box without a GPU."""
    h = ct.c_void_p()
    p = _params(**kw)
    assert lbhip.lb_create(ct.byref(p), ct.byref(h)) == -1 and not h.value          # LB_ERR_ARG
    msg = lbhip.lb_last_error()
    assert word.lower() in msg.lower(), msg
