"""Forced flow in a porous medium on the GPU: k_pm_step and the un-fused phases against the fixtures recorded from the reference's
C and against the numpy model (tests/porous_model.py); the fused step against the eight phases, bitwise; the analytic Darcy and
Forchheimer states; conservation; the empty cell; the drop-in classes; checkpoints; refusals.
Bounds: the project's parity contract (contract_tol) as tests/test_porous_cpu.py states it for each array; everything the
product computes twice must agree bit for bit."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from porous_model import W64
from test_porous_cpu import NAMES, RUN_FIXTURES, compare, model_of, state

pytestmark = pytest.mark.gpu

F = np.float32
ALL = ("f", "feq", "rho", "u", "v", "u_bary", "v_bary", "Gx", "Gy")
FIELDS = ("rho", "u", "v", "u_bary", "v_bary", "Gx", "Gy")
# 261 x 9: two workgroups in x, nx no multiple of 4, the east edge a lane's first cell; 3 x 3 and 256 x 4: the east edge inside a lane
SHAPES = ((5, 4), (3, 3), (37, 23), (261, 9), (256, 4))
PHASES = ("move", "move_bcs", "update_hydro", "update_forces", "update_bary_velocity", "update_feq", "collide_particles")


def got_of(s, which=ALL):
    """the handle's fields under the fixtures' names"""
    g = s.get_fields(which)
    ren = dict(u_bary="ub", v_bary="vb")
    return {ren.get(k, k): v for k, v in g.items()}


def sim_of(d):
    """a porous handle in the state of fixture / case d"""
    from LB_D2Q9.simulation import Simulation
    s = Simulation(int(d["nx"]), int(d["ny"]), F(d["omega"]), bc=str(d["bc"]), semantics="porous")
    s.set_porous(d["epsilon"], d["nu_fluid"], d["K"], d["Fe"])
    s.set_body_force(*d["g"])
    if "field_x" in d:
        s.set_force_field(d["field_x"], d["field_y"])
    if "f0" in d:
        s.set_f(d["f0"])
    return s


def random_case(nx, ny, bc, seed, field=False, Fe=0.3, omega=1.25):
    rng = np.random.default_rng(seed)
    d = dict(nx=nx, ny=ny, bc=bc, omega=F(omega), epsilon=F(0.7), nu_fluid=F(0.15), K=F(20.), Fe=F(Fe), g=np.array([2e-3, -1e-3], F),
             f0=(W64 * (1. + 0.1 * rng.uniform(-1, 1, (nx, ny, 9)))).astype(F))
    if field:
        d["field_x"], d["field_y"] = (1e-3 * rng.uniform(-1, 1, (2, nx, ny))).astype(F)
    return d


def step_by_phases(s):
    for name in PHASES:
        getattr(s, name)()


def same_bits(a, b, keys=ALL):
    return [k for k in keys if not np.array_equal(a[k], b[k], equal_nan=True)]


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
        got = got_of(s)
        compare("%s after %d steps, fused / reference" % (name, n), d, n, got, {k: d["%s_%d" % (k, n)] for k in NAMES})
        compare("%s after %d steps, fused / model" % (name, n), d, n, got, state(m))


def test_phases_follow_phases_fixture(lbhip):
    """move and move_bcs are data movement: exact; the rest within the contract of one step.  The body force of stage 4 is the
    handle's input (constant + field): stages 4 and 5 are one kernel."""
    d = golden("pm_phases_21x13")
    s = sim_of(d)
    stages = dict(move="move", move_bcs="move_bcs", update_hydro="update_hydro", update_forces="update_forces",
                  update_bary_velocity="update_bary", update_feq="update_feq", collide_particles="collide")
    for i, k in enumerate(("x", "y")):                      # (one float32 addition against the reference's float64 one)
        have = (F(d["g"][i]) + d["field_" + k].astype(F)).astype(np.float64)
        assert np.abs(have - d["G%s_after_body_force" % k]).max() <= 2. ** -23 * np.abs(d["G%s_after_body_force" % k]).max()
    full = dict(u=d["u_after_update_hydro"], v=d["v_after_update_hydro"])
    for call, stage in stages.items():
        getattr(s, call)()
        want = {k: d["%s_after_%s" % (k, stage)] for k in NAMES if "%s_after_%s" % (k, stage) in d}
        got = got_of(s, [dict(ub="u_bary", vb="v_bary").get(k, k) for k in want])
        if stage in ("move", "move_bcs"):
            assert np.array_equal(got["f"], want["f"].astype(F)), stage
        else:
            compare("after %s" % stage, d, 1, got, dict(full, **want), list(want))


# ---- what the product computes twice -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ("periodic", "zero_gradient"))
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_step_equals_eight_phases_bitwise(lbhip, shape, bc):
    for field in (False, True):
        for Fe in (0., 0.3):
            d = random_case(shape[0], shape[1], bc, 41, field, Fe)
            a, b = sim_of(d), sim_of(d)
            for n in range(1, 11):
                a.run(1)
                step_by_phases(b)
                bad = same_bits(a.get_fields(ALL), b.get_fields(ALL))
                assert not bad, (shape, bc, field, Fe, n, bad)


@pytest.mark.parametrize("bc", ("periodic", "zero_gradient"))
def test_run_7_equals_seven_run_1_and_model(lbhip, bc):
    d = random_case(37, 23, bc, 42, True)
    a, b, m = sim_of(d), sim_of(d), model_of(d)
    a.run(7)
    for _ in range(7):
        b.run(1)
    m.run(7)
    assert not same_bits(a.get_fields(ALL), b.get_fields(ALL))
    compare("random case, 7 steps, fused / model", d, 7, got_of(a), state(m))


@pytest.mark.parametrize("bc", ("periodic", "zero_gradient"))
def test_stored_fields_equal_phases_recomputed_from_same_f(lbhip, bc):
    """rho, u, v, G, u_b after run(n) are those of the last step before its collision: the phases give them again from the
    populations run(n - 1) left."""
    d = random_case(261, 9, bc, 43, True)
    a, b = sim_of(d), sim_of(d)
    a.run(6)
    b.run(5)
    for name in PHASES[:5]:
        getattr(b, name)()
    assert not same_bits(a.get_fields(FIELDS), b.get_fields(FIELDS), FIELDS)


# ---- physics -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Fe", (0., 0.5))
@pytest.mark.parametrize("bc", ("periodic", "zero_gradient"))
def test_uniform_fluid_reaches_analytic_steady_state(lbhip, bc, Fe):
    """u = g K / nu (Darcy) for Fe = 0, the positive root of (Fe / sqrt(K)) u^2 + (nu / K) u - g = 0 (Forchheimer) otherwise.
    Bound 5e-4 relative: ten times what the reference's own float32 C misses by (3.3e-5 and 4.8e-5)."""
    g, K, nu = 1e-3, 2., 0.2
    d = dict(nx=16, ny=8, bc=bc, omega=F(1. / (0.5 + 3. * 0.1)), epsilon=0.6, nu_fluid=nu, K=K, Fe=Fe, g=(g, 0.),
             f0=np.broadcast_to(W64.astype(F), (16, 8, 9)))
    s = sim_of(d)
    s.run(300)
    got = s.get_fields(FIELDS)
    a, b = Fe / np.sqrt(K), nu / K
    want = g / b if Fe == 0 else (-b + np.sqrt(b * b + 4. * a * g)) / (2. * a)
    err = float(np.abs(got["u_bary"].astype(np.float64) / want - 1.).max())
    print("%s, Fe = %g: u_b = %.8g, analytic %.8g, relative error %.2e / 5e-4; max |v| %.1e, rho spread %.1e"
          % (bc, Fe, got["u_bary"].mean(), want, err, np.abs(got["v_bary"]).max(), np.ptp(got["rho"])))
    assert err <= 5e-4
    assert np.abs(got["v_bary"]).max() <= 1e-7 and np.abs(got["v"]).max() <= 1e-7
    assert np.ptp(got["rho"]) <= 1e-5


def test_mass_and_momentum_conserved_without_force_and_drag(lbhip):
    """Fe = nu_fluid = 0, epsilon = 1, g = 0, periodic: the scheme is plain BGK.  Streaming moves values; the collision of one
    cell keeps sum f and sum f c up to the roundings of its nine results and of the terms they are made of -- a few times
    2^-24 relative to rho ~ 1 per cell and step -- so over n steps the float64 sums of the float32 populations move by at most
    4 n nx ny 2^-24 (the systematic part, sum_k fl(w_k) = 1 + 7.5e-9, is an eighth of 2^-24)."""
    nx, ny, n = 37, 23, 50
    d = random_case(nx, ny, "periodic", 44, False, 0.)
    d.update(epsilon=F(1.), nu_fluid=F(0.), g=np.zeros(2, F))
    s = sim_of(d)
    sums = lambda f: np.array([f.astype(np.float64).sum(), (f.astype(np.float64) * CXY[0]).sum(), (f.astype(np.float64) * CXY[1]).sum()])
    before = sums(d["f0"])
    s.run(n)
    after = sums(s.get_fields(("f",))["f"])
    bound = 4. * n * nx * ny * 2. ** -24
    print("mass, x-momentum, y-momentum moved by %s / %.2e" % (np.abs(after - before), bound))
    assert np.all(np.abs(after - before) <= bound)


CXY = (np.array([0, 1, 0, -1, 0, 1, -1, -1, 1.]), np.array([0, 0, 1, 0, -1, 1, 1, -1, -1.]))


def test_empty_cell_gives_zero_velocity_zero_force_and_nan_bary_velocity_there_only(lbhip):
    """rho = 0 after streaming: u = v = G = 0 by the rule rho > 1e-6, u_b = 0 / 0, as in the reference: not guarded."""
    nx, ny, x0, y0 = 9, 6, 4, 2
    d = random_case(nx, ny, "periodic", 45, True)
    for k in range(9):
        d["f0"][x0 - int(CXY[0][k]), y0 - int(CXY[1][k]), k] = 0.       # what cell (x0, y0) pulls
    s = sim_of(d)
    s.run(1)
    got = s.get_fields(FIELDS)
    assert got["rho"][x0, y0] == 0 and (np.delete(got["rho"].ravel(order="F"), y0 * nx + x0) > 0.5).all()
    for k in ("u", "v", "Gx", "Gy"):
        assert got[k][x0, y0] == 0 and np.isfinite(got[k]).all(), k
    for k in ("u_bary", "v_bary"):
        nan = np.isnan(got[k])
        assert nan[x0, y0] and nan.sum() == 1, k


# ---- the drop-in classes -----------------------------------------------------------------------------------------------------
def runner_of(d):
    from LB_D2Q9.porous_media.single_component import Pourous_Media, Simulation_Runner
    sim = Simulation_Runner(nx=int(d["nx"]), ny=int(d["ny"]))
    fluid = Pourous_Media(sim, 0, nu_e=float(d["nu_e"]), epsilon=float(d["epsilon"]), nu_fluid=float(d["nu_fluid"]), K=float(d["K"]),
                          Fe=float(d["Fe"]), bc=str(d["bc"]))
    sim.add_fluid(fluid)
    sim.complete_setup()
    assert fluid.omega == F(d["omega"]) and sim.tau_arr.shape == (1,)
    return sim, fluid


def runner_state(sim):
    g = sim.get_fields()
    assert g["f"].shape == (sim.nx, sim.ny, 1, 9) and g["rho"].shape == (sim.nx, sim.ny, 1) and g["f"].flags.f_contiguous
    ren = dict(u_bary="ub", v_bary="vb")
    return {ren.get(k, k): (v[:, :, 0] if v.ndim == 3 else v[:, :, 0, :]) for k, v in g.items()}


def test_dropin_initialize_reproduces_init_fixture(lbhip):
    d = golden("pm_init_21x13")
    sim, fluid = runner_of(d)
    sim.add_constant_body_force(0, 3e-4, 0.)                # (not in the buffers during initialize, as in the reference)
    sim.set_bary_velocity(d["ub_in"], d["vb_in"])
    fluid.initialize(d["rho_in"], f_amp=0.)
    assert sim.engine.body_force == (float(F(3e-4)), 0.)
    compare("initialize", d, 1, runner_state(sim), {k: d[k] for k in NAMES})
    assert np.array_equal(np.asarray(sim.rho), runner_state(sim)["rho"][:, :, None])


def test_dropin_run_reproduces_darcy_fixture(lbhip):
    d = golden("pm_darcy_37x23")
    sim, fluid = runner_of(d)
    sim.add_constant_body_force(0, *[float(x) for x in d["g"]])
    sim.engine.set_f(d["f0"])
    sim.run(10)
    compare("drop-in, 10 steps", d, 10, runner_state(sim), {k: d["%s_10" % k] for k in NAMES})


def test_dropin_radial_force_reproduces_radial_fixture(lbhip):
    d = golden("pm_radial_21x13")
    sim, fluid = runner_of(d)
    cx, cy, pref, scal = d["radial"]
    sim.add_radial_body_force(0, int(cx), int(cy), pref, scal)
    fx, fy = sim.engine._force_field
    assert np.array_equal(fx, d["field_x"].astype(F)) and np.array_equal(fy, d["field_y"].astype(F))
    sim.engine.set_f(d["f0"])
    sim.run(10)
    compare("drop-in with a radial force, 10 steps", d, 10, runner_state(sim), {k: d["%s_10" % k] for k in NAMES})


def test_unbuilt_calls_raise_not_implemented(lbhip):
    d = golden("pm_init_21x13")
    sim, fluid = runner_of(d)
    for call in (lambda: sim.add_interaction_force(0, 0, 1.), lambda: sim.add_interaction_force_second_belt(0, 0, 1.),
                 lambda: sim.add_eating_rate(0, 0, 0.1)):
        with pytest.raises(NotImplementedError, match="several fluids and Shan-Chen"):
            call()
    from LB_D2Q9.porous_media.single_component import Simulation_Runner
    with pytest.raises(NotImplementedError, match="several fluids and Shan-Chen"):
        Simulation_Runner(nx=8, ny=8, num_populations=2)
    with pytest.raises(NotImplementedError):
        sim.add_fluid(fluid)                                # a second fluid


# ---- state I/O, refusals, introspection --------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", (False, True))
def test_checkpoint_written_mid_run_resumes_bitwise(lbhip, tmp_path, field):
    from LB_D2Q9.simulation import Simulation
    d = random_case(21, 13, "zero_gradient", 46, field)
    a = sim_of(d)
    a.run(5)
    a.save_checkpoint(tmp_path / "pm")
    b = Simulation.from_checkpoint(tmp_path / "pm")
    assert (b.epsilon, b.nu_fluid, b.K, b.Fe, b.body_force) == (a.epsilon, a.nu_fluid, a.K, a.Fe, a.body_force)
    assert not same_bits(a.get_fields(("f",) + FIELDS), b.get_fields(("f",) + FIELDS), ("f",) + FIELDS)
    a.run(7)
    b.run(7)
    assert not same_bits(a.get_fields(ALL), b.get_fields(ALL))


def test_refusals_are_status_codes_in_both_directions(lbhip):
    from LB_D2Q9.simulation import Simulation
    s = sim_of(random_case(16, 12, "periodic", 47))
    h, L = s._h, lbhip
    one = (ct.c_void_p * 1)(h)
    buf = np.zeros(4096, F)
    p = buf.ctypes.data
    i0 = ct.c_int()
    refused = dict(
        lb_set_mask=lambda: L.lb_set_mask(h, p), lb_set_mask_halo=lambda: L.lb_set_mask_halo(h, None, None),
        lb_step_boundary=lambda: L.lb_step_boundary(h, 0), lb_step_interior=lambda: L.lb_step_interior(h, 0),
        lb_step_finish=lambda: L.lb_step_finish(h), lb_halo_export=lambda: L.lb_halo_export(h, 0, p),
        lb_halo_import=lambda: L.lb_halo_import(h, 0, p), lb_halo_floats=lambda: L.lb_halo_floats(h),
        lb_run_group=lambda: L.lb_run_group(one, 1, 1), lb_set_slab_cycle=lambda: L.lb_set_slab_cycle(h, 3),
        lb_autotune=lambda: L.lb_autotune(h), lb_autotune_quick=lambda: L.lb_autotune_quick(h, 100),
        lb_set_variant=lambda: L.lb_set_variant(h, 512), lb_run_batch=lambda: L.lb_run_batch(one, 1, 1),
        lb_run_coupled=lambda: L.lb_run_coupled(one, 1, 1), lb_solve=lambda: L.lb_solve(h, 1, None, None, None),
        lb_solve_reset=lambda: L.lb_solve_reset(h), lb_get_solve_state=lambda: L.lb_get_solve_state(h, ct.byref(i0), ct.byref(i0)),
        lb_set_poisson=lambda: L.lb_set_poisson(h, 0., 1., 1e-6), lb_gradient=lambda: L.lb_gradient(h, 0.5, None, None),
        lb_set_reaction=lambda: L.lb_set_reaction(h, 0.1), lb_set_velocity_from=lambda: L.lb_set_velocity_from(h, h),
        lb_check=lambda: L.lb_check(h, 0, None, None, None), lb_get_corner_state=lambda: L.lb_get_corner_state(h, p),
        lb_edge_floats=lambda: L.lb_edge_floats(h), lb_zero_velocity_in_obstacle=lambda: L.lb_zero_velocity_in_obstacle(h))
    for name, call in refused.items():
        assert call() == -3, name                                               # LB_ERR_STATE
        msg = L.lb_last_error()
        assert b"LB_SEM_POROUS" in msg and name.encode() in msg, (name, msg)
    assert L.lb_set_variant(h, 0) == 0 and L.lb_set_variant(h, -1) == 0
    for eps, nu, K, Fe in ((0., 0.1, 1., 0.), (-1., 0.1, 1., 0.), (1., 0.1, 0., 0.), (1., 0.1, -2., 0.), (np.nan, 0.1, 1., 0.),
                           (1., np.inf, 1., 0.), (1., 0.1, np.inf, 0.), (1., 0.1, 1., np.nan)):
        assert L.lb_set_porous(h, eps, nu, K, Fe) == -1                        # LB_ERR_ARG
    assert L.lb_set_force_field(h, p, None, 0) == -1
    s.run(3)                                                                    # none of it disturbed the handle
    assert np.isfinite(s.get_fields(("f",))["f"]).all()
    # the other direction: the new calls on every other kind of handle
    others = [Simulation(16, 12, 1.2, bc="periodic"), Simulation(16, 12, 1.2, bc="periodic", semantics="diffusion"),
              Simulation(16, 12, 0.5, bc="dirichlet", semantics="poisson")]
    for o in others:
        g = o._h
        calls = dict(lb_set_porous=lambda: L.lb_set_porous(g, 1., 0., 1., 0.), lb_set_body_force=lambda: L.lb_set_body_force(g, 0., 0.),
                     lb_set_force_field=lambda: L.lb_set_force_field(g, None, None, 0), lb_get_force=lambda: L.lb_get_force(g, p, p),
                     lb_set_force=lambda: L.lb_set_force(g, p, p), lb_set_bary_velocity=lambda: L.lb_set_bary_velocity(g, p, p),
                     lb_get_bary_velocity=lambda: L.lb_get_bary_velocity(g, p, p), lb_update_forces=lambda: L.lb_update_forces(g),
                     lb_update_bary_velocity=lambda: L.lb_update_bary_velocity(g))
        for name, call in calls.items():
            assert call() == -3 and b"LB_SEM_POROUS" in L.lb_last_error() and name.encode() in L.lb_last_error(), (o.semantics, name)
    with pytest.raises(Exception, match="LB_SEM_POROUS"):
        others[0].get_fields(("u_bary",))


@pytest.mark.parametrize("bc", ("periodic", "zero_gradient"))
def test_hot_kernel_plan_and_layout(lbhip, bc):
    s = sim_of(random_case(37, 23, bc, 48))
    assert s.hot_kernel().startswith("k_pm_step") and bc.upper() in s.hot_kernel() and "FIELD" not in s.hot_kernel()
    assert s.plan_launches(5) == [1] * 5 and s.steps_per_launch() == 1
    lay = s.layout()
    assert lay["pitch"] == 64 and lay["bytes"] > 0
    s.set_force_field(np.zeros((37, 23), F), np.zeros((37, 23), F))
    assert "FIELD" in s.hot_kernel() and s.layout()["bytes"] == lay["bytes"] + 2 * 4 * 64 * 23
    s.set_force_field(None, None)
    assert "FIELD" not in s.hot_kernel() and s.layout()["bytes"] == lay["bytes"]
