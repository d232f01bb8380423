"""The LB Poisson solver on the GPU: k_ps_step and the un-fused phases against the fixtures recorded from the reference's C and
against the numpy model (tests/poisson_model.py); the fused step against the phases, bitwise; the device-side stopping rule against
the reference's recorded ratio series; the reduction, the gradient, sources, checkpoints, the corner state, refusals.
Bounds: the project's parity contract (contract_tol); everything the product computes twice must agree bit for bit."""
import ctypes as ct
import os

import numpy as np
import pytest

from conftest import golden
from multifield_model import CORNER_LINKS
from poisson_model import F, W, PoissonModel, contract_tol
from test_poisson_cpu import RUN_FIXTURES, TOLERANCE, first_below, maxdiff, model_of

pytestmark = pytest.mark.gpu


def assert_close(got, want, n, keys=("f", "rho"), what=""):
    """max |got - want| within the contract for n iterations (feq is held to f's bound); prints the measured margins."""
    tol = contract_tol(n)
    tol["feq"] = tol["f"]
    meas = {k: maxdiff(got[k], want[k]) for k in keys}
    print("%s after %d iterations, measured / bound: %s" % (what, n, ", ".join("%s %.2e / %.1e" % (k, meas[k], tol[k]) for k in keys)))
    for k in keys:
        assert meas[k] <= tol[k], "%s %s: %.3e > %.1e" % (what, k, meas[k], tol[k])


def sim_of(d, tolerance=1e-6, batch=None):
    """a Poisson handle in the state of fixture / case d; batch: lb_solve's batch length forced through the handle's diagnostic word"""
    from LB_D2Q9.simulation import Simulation
    old = os.environ.get("LB_DIAG")
    if batch is not None:
        os.environ["LB_DIAG"] = str(batch)
    try:
        s = Simulation(int(d["nx"]), int(d["ny"]), d["omega"], bc="dirichlet", semantics="poisson")
    finally:
        if batch is not None:
            os.environ.pop("LB_DIAG")
            if old is not None:
                os.environ["LB_DIAG"] = old
    s.set_poisson(d["rho_on_boundary"], d["react_factor"], tolerance)
    s.set_source(d["scaled_source"])
    s.set_f(d["f0"])
    return s


def random_case(nx, ny, seed, omega=0.7, rho_b=0.3):
    rng = np.random.default_rng(seed)
    f0 = (W * 0.3 * (1. + 0.2 * rng.uniform(-1, 1, (nx, ny, 9)))).astype(F)
    src = (0.002 * rng.uniform(size=(nx, ny))).astype(F)
    return dict(nx=nx, ny=ny, omega=F(omega), rho_on_boundary=F(rho_b), react_factor=F(0.5), scaled_source=src, f0=f0)


def same_bits(a, b, keys=("f", "rho")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_fused_run_follows_reference_fixture_and_model(lbhip, name):
    d = golden(name)
    s, m = sim_of(d), model_of(d)
    done = 0
    for n in [int(k) for k in d["steps"]]:
        s.run(n - done)
        m.run(n - done)
        done = n
        got = s.get_fields(("f", "rho", "feq"))
        assert got["rho"].any() == d["rho_%d" % n].any()                    # the run stored it (all zero after one iteration of the zero lattice)
        assert_close(got, dict(f=d["f_%d" % n], rho=d["rho_%d" % n], feq=d["feq_%d" % n]), n, ("f", "rho", "feq"), name + " fused")
        assert_close(got, m.get_fields(), n, ("f", "rho", "feq"), name + " fused vs model")
        # feq on demand comes from the STORED rho: feq_0 = (w0 - 1) rho, feq_k = w_k rho, one float32 product each
        want = np.stack([(W[0] - F(1)) * got["rho"]] + [W[k] * got["rho"] for k in range(1, 9)], axis=2)
        assert np.array_equal(got["feq"], want)
        assert s.solve_state()[0] == n                                      # lb_run's iterations count (solver.py's num_iterations)
    s.close()


def test_single_phases_follow_reference_fixture(lbhip):
    d = golden("ps_phases_21x13")
    s = sim_of(d)
    tol = contract_tol(1)
    s.move()
    assert np.array_equal(s.get_fields(("f",))["f"], d["f_move"])
    s.move_bcs()
    f = s.get_fields(("f",))["f"]
    inner = np.zeros((21, 13), bool)
    inner[1:-1, 1:-1] = True
    assert np.array_equal(f[inner], d["f_bcs"][inner]) and maxdiff(f, d["f_bcs"]) <= tol["f"]
    for k, x, y in CORNER_LINKS:                                            # the eight links nothing writes
        assert f[x, y, k] == d["f0"][x, y, k]
    s.move_bcs()                                                            # the reference runs the rule nine times: idempotent
    assert np.array_equal(s.get_fields(("f",))["f"], f)
    s.update_hydro()
    assert maxdiff(s.get_fields(("rho",))["rho"], d["rho_hydro"]) <= tol["rho"]
    s.update_feq()
    assert maxdiff(s.get_fields(("feq",))["feq"], d["feq_feq"]) <= tol["f"]
    s.collide_particles()
    assert maxdiff(s.get_fields(("f",))["f"], d["f_collide"]) <= tol["f"]
    t = sim_of(d)                                                           # and the fused step from the same start
    t.run(1)
    assert_close(t.get_fields(("f", "rho", "feq")), dict(f=d["f_collide"], rho=d["rho_hydro"], feq=d["feq_feq"]), 1, ("f", "rho", "feq"),
                 "ps_phases fused")
    # phases behind a fused run: the corner links are patched back in from the corner state
    c = t.get_corner_state()
    assert np.array_equal(c, [d["f0"][x, y, k] for k, x, y in CORNER_LINKS])
    t.run(2)
    t.move()
    t.move_bcs()
    f = t.get_fields(("f",))["f"]
    assert np.array_equal([f[x, y, k] for k, x, y in CORNER_LINKS], c) and np.array_equal(t.get_corner_state(), c)
    s.close(); t.close()


# ---- the fused step is the five phases, bit for bit ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 4), (37, 23), (261, 9), (256, 4)])
def test_fused_step_equals_phases_bitwise(lbhip, shape):
    """261 x 9: two workgroups in x, three in y, nx no multiple of 4, the last lane straddling the east wall; 256 x 4: exactly one
    workgroup, the east wall in the last lane's last cell.  Both forms of the fused kernel (lb_run's and lb_solve's)."""
    d = random_case(shape[0], shape[1], 31)
    fused, solve, phases = sim_of(d), sim_of(d, tolerance=0.), sim_of(d)
    for it in range(10):
        fused.run(1)
        assert solve.solve(1)[:2] == (1, False)
        for phase in (phases.move, phases.move_bcs, phases.update_hydro, phases.update_feq, phases.collide_particles):
            phase()
        a, b, c = (x.get_fields(("f", "rho")) for x in (fused, solve, phases))
        assert same_bits(a, c), (shape, it)
        assert same_bits(a, b), (shape, it)
    assert_close(a, _model_run(d, 10), 10, what="%dx%d vs model" % shape)
    for x in (fused, solve, phases):
        x.close()


def _model_run(d, n):
    m = model_of(d)
    m.run(n)
    return m.get_fields()


# ---- the stopping rule ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stopped(lbhip):
    """ps_box_37x23 solved to 1e-4 in one call, once: (n*, the fixture's ratio at n*, iterations, converged, ratio, fields)"""
    d = golden("ps_box_37x23")
    n_star, i = first_below(d)
    s = sim_of(d, TOLERANCE)
    done, converged, ratio = s.solve(600)
    out = dict(n_star=n_star, want=float(d["ratios"][i]), done=done, converged=converged, ratio=ratio,
               fields=s.get_fields(("f", "rho")), state=s.solve_state())
    s.close()
    return out


def test_solve_stops_at_the_reference_iteration(lbhip, stopped):
    d = golden("ps_box_37x23")
    print("n* = %d, device ratio %.6e, recorded %.6e" % (stopped["n_star"], stopped["ratio"], stopped["want"]))
    assert (stopped["done"], stopped["converged"]) == (stopped["n_star"], True)
    assert stopped["state"] == (stopped["n_star"], stopped["n_star"])        # the counter, and the stop word the device wrote
    # (1 %: the margin the fixture keeps around the threshold -- a ratio further off could have moved the stop)
    assert abs(stopped["ratio"] - stopped["want"]) <= 0.01 * stopped["want"] and stopped["ratio"] < TOLERANCE
    t = sim_of(d)
    t.run(stopped["n_star"])                                                 # exactly the state after n* iterations
    assert same_bits(stopped["fields"], t.get_fields(("f", "rho")))
    t.close()


def test_solve_does_not_depend_on_the_batch_length(lbhip, stopped):
    d = golden("ps_box_37x23")
    for batch in (1, 7):
        s = sim_of(d, TOLERANCE, batch=batch)
        assert s.solve(600)[:2] == (stopped["n_star"], True)
        assert same_bits(stopped["fields"], s.get_fields(("f", "rho"))), batch
        s.close()


def test_solve_in_two_calls_and_after_a_stop(lbhip, stopped):
    d = golden("ps_box_37x23")
    n_star = stopped["n_star"]
    s = sim_of(d, TOLERANCE)
    assert s.solve(n_star - 5)[:2] == (n_star - 5, False)
    assert s.solve(600)[:2] == (5, True) and s.solve_state() == (n_star, n_star)
    assert same_bits(stopped["fields"], s.get_fields(("f", "rho")))
    # a call after a stop goes on, as the reference's run does: one more iteration, which meets the rule again
    assert s.solve(600)[:2] == (1, True) and s.solve_state() == (n_star + 1, n_star + 1)
    t = sim_of(d)
    t.run(n_star + 1)
    assert same_bits(s.get_fields(("f", "rho")), t.get_fields(("f", "rho")))
    s.close(); t.close()


def test_solve_without_convergence(lbhip):
    d = golden("ps_box_37x23")
    s = sim_of(d, tolerance=0.)                                              # nothing is < 0: all iterations, not converged
    done, converged, ratio = s.solve(40)
    assert (done, converged) == (40, False) and 0. < ratio < 1. and s.solve_state() == (40, 0)
    assert abs(ratio - float(d["ratios"][40 - 2])) <= 0.01 * float(d["ratios"][40 - 2])
    s.close()
    from LB_D2Q9.simulation import Simulation
    z = Simulation(37, 23, 0.5, bc="dirichlet", semantics="poisson")       # the zero lattice, a zero source: 0 / 0 every time
    z.set_poisson(0., 0.25, TOLERANCE)
    done, converged, ratio = z.solve(20)
    assert (done, converged) == (20, False) and np.isnan(ratio) and not z.get_fields(("rho",))["rho"].any()
    z.close()


# ---- the reduction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [False, True])
def test_device_ratio_is_the_float64_ratio_of_the_box(lbhip, poison):
    """261 x 9 (row pitch 320: 59 padding columns, three rows of padding lanes in the last workgroups).  No upload reaches the
    padding -- every one is nx wide --, so it is poisoned the way it is written at all: f1 of the east column leaves the box and
    is read by nothing but the first padding column's pull, so a NaN there turns the padding of the populations AND of rho into
    NaN within two fused iterations and leaves every cell of the box as it was.  The sums must select, not weigh."""
    d = random_case(261, 9, 41)
    clean = sim_of(d, tolerance=0.)
    if poison:
        d = dict(d, f0=d["f0"].copy())
        d["f0"][-1, :, 1] = np.nan
    s = sim_of(d, tolerance=0.)
    for x in (s, clean):
        x.run(2)
    old = s.get_fields(("rho",))["rho"]
    done, converged, ratio = s.solve(1)
    clean.solve(1)
    new = s.get_fields(("f", "rho"))
    assert np.all(np.isfinite(new["rho"])) and same_bits(new, clean.get_fields(("f", "rho")))
    want = np.abs(new["rho"].astype(np.float64) - old).sum() / old.astype(np.float64).sum()
    print("device ratio %.9e, float64 %.9e" % (ratio, want))
    assert (done, converged) == (1, False) and abs(ratio - want) <= 1e-5 * want
    s.close(); clean.close()


# ---- the gradient --------------------------------------------------------------------------------------------------------
def test_gradient_follows_reference_fixture_and_naming(lbhip):
    from LB_D2Q9.poisson import Poisson_Solver
    d = golden("ps_grad_21x13")
    ps = Poisson_Solver(nx=21, ny=13, sources=np.zeros((21, 13), np.float32), delta_t=0.5, delta_x=float(d["delta_x"]))
    assert not np.asarray(ps.u).any() and not np.asarray(ps.v).any()
    zero = np.zeros((21, 13), np.float32)
    ps.sim.set_fields(d["rho"], zero, zero)
    ddx, ddy = ps.sim.gradient(float(d["delta_x"]))                         # the native surface: (d/dx, d/dy)
    m = PoissonModel(21, 13, 0.5)
    m.rho = d["rho"].copy()
    mx, my = m.gradient(float(d["delta_x"]))
    assert maxdiff(ddx, mx) <= 1e-6 and maxdiff(ddy, my) <= 1e-6 and np.abs(ddx).max() > 0
    g = ps.sim.get_fields(("u", "v"))                                       # ... which the handle's u, v hold from then on
    assert np.array_equal(g["u"], ddx) and np.array_equal(g["v"], ddy)
    ps.update_negative_gradient()                                           # the reference's names: u = -d/dy, v = -d/dx
    u, v = np.asarray(ps.u), np.asarray(ps.v)
    assert u.shape == (21, 13) and maxdiff(u, d["u"]) <= 1e-6 and maxdiff(v, d["v"]) <= 1e-6
    assert np.array_equal(u, -ddy) and np.array_equal(v, -ddx)
    ps.sim.close()


# ---- sources, the drop-in class, checkpoints ----------------------------------------------------------------------------------
def test_dropin_solves_and_update_source_restarts_the_count(lbhip, stopped):
    from LB_D2Q9.poisson import Poisson_Solver
    d = golden("ps_box_37x23")
    ps = Poisson_Solver(nx=37, ny=23, sources=d["source"], delta_t=float(d["delta_t"]), delta_x=float(d["delta_x"]),
                        rho_on_boundary=float(d["rho_on_boundary"]), tolerance=TOLERANCE)
    assert ps.omega == d["omega"] and ps.lb_D == d["lb_D"] and np.array_equal(ps.scaled_sources, d["scaled_source"])
    assert ps.num_iterations == 0 and not ps.converged and not ps.get_fields()["f"].any()
    ps.run(30)
    assert ps.num_iterations == 30 and not ps.converged
    ps.run(600)
    assert ps.num_iterations == stopped["n_star"] and ps.converged
    g = ps.get_fields()
    assert sorted(g) == ["f", "feq", "rho"] and np.isfortran(g["f"]) and same_bits(g, stopped["fields"])
    assert np.array_equal(np.asarray(ps.rho), g["rho"]) and np.abs(np.asarray(ps.u)).max() > 0      # the stop updated u, v
    ps.update_source(2. * d["source"])                                      # counter to 0, the fields stay
    assert ps.num_iterations == 0 and not ps.converged and same_bits(ps.get_fields(), g)
    assert np.array_equal(ps.sim.get_source(), 2. * d["scaled_source"])
    ps.run(3)
    assert ps.num_iterations == 3
    ps.sim.close()


DEVICE_SOURCE_CHILD = r"""
import sys
import torch                                    # first: the process then has ONE HIP runtime, torch's, and the library binds to it
import numpy as np
sys.path[:0] = [sys.argv[1], sys.argv[2]]
from conftest import golden
from LB_D2Q9.poisson import Poisson_Solver
d = golden("ps_noise_37x23")
kw = dict(nx=37, ny=23, delta_t=float(d["delta_t"]), delta_x=float(d["delta_x"]), rho_on_boundary=float(d["rho_on_boundary"]))
a = Poisson_Solver(sources=d["source"], **kw)
t = torch.from_numpy(np.ascontiguousarray(d["source"])).cuda()
b = Poisson_Solver(sources=t, **kw)
assert b.sources is t and b.scaled_sources.is_cuda
assert np.array_equal(a.sim.get_source(), d["scaled_source"]) and np.array_equal(b.sim.get_source(), d["scaled_source"])
for x in (a, b):
    x.sim.set_f(d["f0"])
    x.run(10)
fa, fb = a.get_fields(), b.get_fields()
assert all(np.array_equal(fa[k], fb[k]) for k in ("f", "rho", "feq")) and a.num_iterations == b.num_iterations == 10
b.update_source(2. * t)                         # and again, device to device
assert np.array_equal(b.sim.get_source(), 2. * d["scaled_source"]) and b.num_iterations == 0
print("DEVICE_SOURCE_OK")
"""


def test_device_tensor_source_equals_numpy_source(lbhip, tmp_path):
    """A float32 torch tensor on the device as the source (the reference is handed a device array by its Fisher-wave script): copied
    device to device, bit for bit the numpy source.  In a process of its own, because that is what the test is about: torch and the
    library share a device pointer only where they share one HIP runtime, i.e. where torch was imported first."""
    import subprocess
    import sys
    from conftest import ROOT
    script = tmp_path / "device_source.py"
    script.write_text(DEVICE_SOURCE_CHILD)
    p = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-lb_amd")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "DEVICE_SOURCE_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_checkpoint_in_mid_solve(lbhip, stopped, tmp_path):
    from LB_D2Q9.simulation import Simulation
    d = golden("ps_box_37x23")
    n_star = stopped["n_star"]
    s = sim_of(d, TOLERANCE)
    s.set_corner_state(np.arange(1, 9, dtype=np.float32) * 1e-3)            # (a state of its own, so that the checkpoint must carry it)
    ref = sim_of(d, TOLERANCE)
    ref.set_corner_state(s.get_corner_state())
    assert s.solve(n_star - 5)[1] is False
    s.save_checkpoint(tmp_path / "mid")
    t = Simulation.from_checkpoint(tmp_path / "mid")
    assert t.semantics == "poisson" and t.solve_state() == (n_star - 5, 0) and np.array_equal(t.get_source(), d["scaled_source"])
    assert (t.rho_on_boundary, t.react_factor, t.tolerance) == (s.rho_on_boundary, s.react_factor, s.tolerance)
    assert np.array_equal(t.get_corner_state(), s.get_corner_state())
    a, b, c = s.solve(600), t.solve(600), ref.solve(600)
    assert a == b and a[1] and a[0] + n_star - 5 == c[0] and b[2] == c[2]
    assert same_bits(t.get_fields(("f", "rho")), ref.get_fields(("f", "rho"))) and t.solve_state() == ref.solve_state()
    for x in (s, t, ref):
        x.close()


# ---- the corner state ----------------------------------------------------------------------------------------------------
def test_kernel_reads_the_corner_state(lbhip):
    """f6 of (0, 0) changed in the corner state: behind move + move_bcs exactly that link and the three the corner's rule writes from
    it (f1, f2, f5) differ; behind one fused step nothing but the cell (0, 0) differs, and there those four links.  Its rho does NOT
    follow: the rule exists to pin (9/5)(f1 + ... + f8) of a wall cell to rho_on_boundary, whatever the other links hold -- up to the
    rounding of the rule, which is all that rho, and through feq the other links, may differ by."""
    d = golden("ps_noise_37x23")
    c = model_of(d).get_corner_state()
    changed = c.copy()
    changed[0] += np.float32(0.01)
    out = []
    for state in (c, changed):
        s, p = sim_of(d), sim_of(d)
        for x in (s, p):
            assert np.array_equal(x.get_corner_state(), c)                 # set_f captured f0's own corner links
            x.set_corner_state(state)
        s.run(1)
        p.move(); p.move_bcs()
        out.append((s.get_fields(("f", "rho")), p.get_fields(("f",))["f"]))
        s.close(); p.close()
    (a, pa), (b, pb) = out
    assert sorted(zip(*np.nonzero(pa != pb))) == [(0, 0, 1), (0, 0, 2), (0, 0, 5), (0, 0, 6)]
    elsewhere = np.ones((37, 23), bool)
    elsewhere[0, 0] = False
    assert np.array_equal(a["rho"][elsewhere], b["rho"][elsewhere]) and np.array_equal(a["f"][elsewhere], b["f"][elsewhere])
    assert np.all(a["f"][0, 0, [1, 2, 5, 6]] != b["f"][0, 0, [1, 2, 5, 6]])
    assert abs(float(a["f"][0, 0, 6]) - float(b["f"][0, 0, 6])) > 1e-3      # (the state link itself: 0.01 (1 - omega))
    for g in (a, b):
        assert abs(float(g["rho"][0, 0]) - float(d["rho_on_boundary"])) <= contract_tol(1)["rho"]
    assert maxdiff(a["f"][0, 0, [0, 3, 4, 7, 8]], b["f"][0, 0, [0, 3, 4, 7, 8]]) <= contract_tol(1)["f"]
    m = model_of(d)                                                         # and the model agrees about the changed run
    m.set_corner_state(changed)
    m.run(1)
    assert_close(b, m.get_fields(), 1, what="changed corner state")


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_are_status_codes_and_planner_names_the_kernel(lbhip):
    from LB_D2Q9.simulation import Simulation
    s = Simulation(40, 12, 0.5, bc="dirichlet", semantics="poisson")
    L, h = s._lib, s._h
    assert "k_ps_step" in s.hot_kernel() and s.steps_per_launch() == 1 and s.plan_launches(5) == [1] * 5
    STATE = -3
    assert L.lb_set_reaction(h, 0.1) == STATE and b"Poisson" in L.lb_last_error()
    assert L.lb_set_velocity_from(h, h) == STATE
    assert L.lb_set_variant(h, 1 << 9) == STATE and L.lb_set_variant(h, 0) == 0 and L.lb_set_variant(h, -1) == 0
    assert L.lb_autotune(h) == STATE and L.lb_autotune_quick(h, 100) == STATE
    assert L.lb_check(h, 0, None, None, None) == STATE
    mask = np.zeros((12, 40), np.int32)
    assert L.lb_set_mask(h, mask.ctypes.data) == STATE and L.lb_halo_floats(h) == STATE
    assert L.lb_run_batch((ct.c_void_p * 1)(h), 1, 1) == STATE and L.lb_step_boundary(h, 0) == STATE
    assert L.lb_solve(h, -1, None, None, None) == -1 and L.lb_set_poisson(h, 0., 1., -1.) == -1
    assert L.lb_gradient(h, float("inf"), None, None) == -1 and L.lb_set_source(h, None, 0) == -1
    assert L.lb_gradient(h, 0.5, None, None) == 0                           # no copy: the gradient stays in the handle's u, v
    assert L.lb_set_solve_state(h, 3, 5) == -1
    assert L.lb_solve(h, 0, None, None, None) == 0 and L.lb_edge_floats(h) == 0
    s.close()
    t = Simulation(40, 12, 1.0, bc="open", semantics="diffusion")          # the solver's entry points on another handle
    for rc in (L.lb_solve(t._h, 1, None, None, None), L.lb_set_poisson(t._h, 0., 1., 1e-6), L.lb_solve_reset(t._h),
               L.lb_get_solve_state(t._h, None, None), L.lb_set_solve_state(t._h, 0, 0)):
        assert rc == STATE and b"LB_SEM_POISSON" in L.lb_last_error()
    t.close()
