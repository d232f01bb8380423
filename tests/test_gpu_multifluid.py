"""Multicomponent Shan-Chen fluids on the GPU: the two-launch step (k_mc_moments + k_mc_collide) and the un-fused phases against
the fixtures recorded from the reference's C and against the numpy model (tests/multifluid_model.py); the step against the
phases, bitwise; conservation; uniform acceleration; the empty cell; the drop-in classes; checkpoints; refusals.
Bounds: the project's parity contract (contract_tol) as tests/test_multifluid_cpu.py states it for each array; everything the
product computes twice must agree bit for bit."""
import ctypes as ct
import os

import numpy as np
import pytest

from conftest import golden
from multifluid_model import POTENTIALS, W64, MultifluidModel, from_fixture
from scalar_model import contract_tol
from test_multifluid_cpu import NAMES, RUN_FIXTURES, WRITES, compare, recorded, state

pytestmark = pytest.mark.gpu

F = np.float32
ALL = ("f", "feq", "rho", "u", "v", "Gx", "Gy", "u_bary", "v_bary")
# 261 x 9: two workgroups in x, nx no multiple of 4, the east edge a lane's first cell; 3 x 3 and 256 x 4: the east edge inside a
# lane; 517 x 5: three workgroups in x, so that one has neighbours on both sides of its column halo, and ny = 2 * 2 + 1 for the two
# rows a workgroup of k_mc_step owns with three fluids; 6 x 13: ny = 2 * 6 + 1 for its six rows with one and two fluids; 6 x 9:
# 2 * 4 + 1 for the four rows of a workgroup of the two-launch step -- a row halo crosses a workgroup boundary and the last
# workgroup is ragged
SHAPES = ((3, 3), (5, 4), (37, 23), (261, 9), (256, 4), (517, 5), (6, 9), (6, 13))


def got_of(s, which=ALL):
    g = s.get_fields(which)
    ren = dict(u_bary="ub", v_bary="vb")
    return {ren.get(k, k): v for k, v in g.items()}


def set_of(d):
    """a set of fluids in the state of fixture / case d"""
    from LB_D2Q9.coupled import Shan_Chen_Fluids
    s = Shan_Chen_Fluids(int(d["nx"]), int(d["ny"]), [F(o) for o in d["omega"]], bc=str(d["bc"]))
    for i, (gx, gy) in enumerate(d["g"]):
        s.set_body_force(i, gx, gy)
    for i, fld in enumerate(d["field"] if "field" in d else ()):
        if fld is not None:
            s.set_force_field(i, fld[0], fld[1])
    s.set_interactions([(int(r[0]), int(r[1]), r[2], POTENTIALS[int(r[3])], r[4]) for r in d["interactions"]])
    s.set_reactions([("eat", int(r[1]), int(r[2]), r[3], r[4]) if int(r[0]) == 0 else ("grow", int(r[1]), r[3], r[4], r[5]) for r in d["reactions"]])
    if "f0" in d:
        s.set_f(d["f0"])
    return s


def random_case(nx, ny, bc, nf, seed, field=False, tables=True):
    """nf fluids with noisy populations; all three potentials, a self term and both reactions where the set is large enough"""
    rng = np.random.default_rng(seed)
    rhos = np.array([1., 0.9, 0.8][:nf])
    inter = [[0, 0, -0.4, 1, 1.]]
    react = [[1, 0, 0, 0.95, 1.05, 1e-3]]
    if nf > 1:
        inter += [[0, 1, 0.9, 0, 0.], [1, 0, 0.3, 2, 1.5]]
        react += [[0, 1, 0, 1e-3, 0.5, 0.]]
    if nf > 2:
        inter += [[1, 2, 0.6, 1, 0.8], [0, 2, 0.5, 0, 0.], [2, 2, 0.2, 2, 2.]]
        react += [[0, 2, 1, 2e-3, 0.2, 0.], [1, 2, 0, 0.5, 1.5, -1e-3]]
    d = dict(nx=nx, ny=ny, bc=bc, omega=np.array([1.25, 0.9, 1.05][:nf], F), g=np.array([[2e-3, -1e-3], [0., 1e-3], [-1e-3, 0.]][:nf], F),
             interactions=np.array(inter if tables else [], np.float64).reshape(-1, 5),
             reactions=np.array(react if tables else [], np.float64).reshape(-1, 6),
             f0=(W64 * rhos[None, None, :, None] * (1. + 0.1 * rng.uniform(-1, 1, (nx, ny, nf, 9)))).astype(F))
    if field:
        d["field"] = [tuple((1e-3 * rng.uniform(-1, 1, (2, nx, ny))).astype(F)) if i != 1 else None for i in range(nf)]
    return d


def model_of_case(d, dtype=np.float64):
    m = from_fixture(d, dtype)
    for i, fld in enumerate(d.get("field", ())):
        if fld is not None:
            m.set_force_field(i, *fld)
    return m


def same_bits(a, b, keys=ALL):
    return [k for k in keys if not np.array_equal(a[k], b[k], equal_nan=True)]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_run_follows_reference_fixture_and_model(lbhip, name, variant):
    d = golden(name)
    s, m = set_of(d), from_fixture(d, F)
    s.set_variant(variant)
    done = 0
    for n in [int(k) for k in d["steps"]]:
        s.run(n - done)
        m.run(n - done)
        done = n
        got = got_of(s)
        compare("%s after %d steps, run / reference" % (name, n), m, n, got, recorded(d, n))
        compare("%s after %d steps, run / model" % (name, n), m, n, got, state(m))


def test_phases_follow_phases_fixture(lbhip):
    """move and move_bcs are data movement: exact; the rest within the contract of one step."""
    d = golden("mc_phases_21x13")
    s, m = set_of(d), from_fixture(d, F)
    stages = dict(move="move", move_bcs="move_bcs", update_hydro="update_hydro", update_forces="forces", update_bary_velocity="update_bary",
                  update_feq="update_feq", collide_particles="collide", react="react")
    for call, stage in stages.items():
        getattr(s, call)()
        want = {k: d["%s_after_%s" % (k, stage)] for k in WRITES[stage]}
        got = got_of(s, [dict(ub="u_bary", vb="v_bary").get(k, k) for k in want])
        if stage in ("move", "move_bcs"):
            assert np.array_equal(got["f"], want["f"].astype(F)), stage
        else:
            compare("after %s" % stage, m, 1, got, dict(want, rho=d["rho_after_update_hydro"]), list(want))


# ---- what the product computes twice -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ("periodic", "zero_gradient"))
@pytest.mark.parametrize("nf", (1, 2, 3))
@pytest.mark.parametrize("shape", SHAPES)
def test_run_equals_phases_bitwise(lbhip, shape, nf, bc):
    """The one-launch step = the two-launch step = the phases: ten steps, every array, with and without a force field, with all
    three potentials and a reaction table."""
    for field in (False, True):
        d = random_case(shape[0], shape[1], bc, nf, 41 + nf, field)
        a, b, c = set_of(d), set_of(d), set_of(d)
        a.set_variant(0)
        c.set_variant(1)
        for n in range(1, 11):
            a.run(1)
            b.step_phases()
            c.run(1)
            want = b.get_fields(ALL)
            bad = same_bits(a.get_fields(ALL), want), same_bits(c.get_fields(ALL), want)
            assert not bad[0] and not bad[1], (shape, nf, bc, field, n, bad)
        for s in (a, b, c):
            s.close()


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("bc", ("periodic", "zero_gradient"))
def test_run_7_is_seven_runs_of_1_and_last_launch_fields_are_the_phases(lbhip, bc, variant):
    d = random_case(37, 23, bc, 3, 7, field=True)
    a, b, c = set_of(d), set_of(d), set_of(d)
    for s in (a, b, c):
        s.set_variant(variant)
    a.run(7)
    for _ in range(7):
        b.run(1)
    assert not same_bits(a.get_fields(ALL), b.get_fields(ALL))
    # the fields a run's last launch stores = the phases recomputed from the populations of run(n - 1)
    c.run(6)
    c.step_phases()
    assert not same_bits(a.get_fields(ALL), c.get_fields(ALL))


def test_without_tables_a_single_fluid_is_plain_bgk_with_guo_forcing(lbhip):
    """No tables, no force: u_b = u, G = 0; mass and momentum are conserved to the contract."""
    d = random_case(37, 23, "periodic", 1, 9, tables=False)
    d["g"][:] = 0
    s, m = set_of(d), model_of_case(d)
    s.run(10)
    m.run(10)
    g = s.get_fields(ALL)
    assert not np.any(g["Gx"]) and not np.any(g["Gy"])
    cells = 37 * 23
    assert abs(float(g["f"].astype(np.float64).sum()) - m.f.sum()) <= cells * contract_tol(10)["rho"]


# ---- physics ---------------------------------------------------------------------------------------------------------------------
def test_conservation_on_the_device(lbhip):
    """Pair forces: every fluid's mass stays and sum G = 0; eating: the pair's mass stays; growth: rate x cells in the window.
    Device totals within cells x the per-cell contract of the float64 model's."""
    nx, ny, n = 37, 23, 5
    cells = nx * ny
    tol = contract_tol(n)
    d = random_case(nx, ny, "periodic", 3, 11)
    d["g"][:] = 0
    d["reactions"] = np.zeros((0, 6))
    s, m = set_of(d), model_of_case(d)
    s.run(n)
    m.run(n)
    g = s.get_fields(ALL)
    mass = g["f"].astype(np.float64).sum(axis=(0, 1, 3))
    assert np.all(np.abs(mass - d["f0"].astype(np.float64).sum(axis=(0, 1, 3))) <= cells * tol["rho"])
    assert np.all(np.abs(mass - m.f.sum(axis=(0, 1, 3))) <= cells * tol["rho"])
    from multifluid_model import force_bound
    gb = force_bound(m.interactions, m.g, 3, float(m.rho.max()), tol["rho"]).sum()
    assert abs(g["Gx"].astype(np.float64).sum()) <= cells * gb and abs(g["Gy"].astype(np.float64).sum()) <= cells * gb
    # eating alone, then growth alone
    e = random_case(nx, ny, "periodic", 2, 12, tables=False)
    e["reactions"] = np.array([[0, 0, 1, 1e-3, 0.5, 0.]])
    s, m = set_of(e), model_of_case(e)
    s.run(n)
    m.run(n)
    mass = s.get_fields(("f",))["f"].astype(np.float64).sum(axis=(0, 1, 3))
    assert abs(mass.sum() - e["f0"].astype(np.float64).sum()) <= cells * tol["rho"] and mass[0] > e["f0"][:, :, 0].astype(np.float64).sum() + 1e-3
    assert np.all(np.abs(mass - m.f.sum(axis=(0, 1, 3))) <= cells * tol["rho"])
    w = random_case(nx, ny, "periodic", 2, 13, tables=False)
    w["reactions"] = np.array([[1, 1, 0, 0.5, 1.5, 1e-3]])              # every cell of fluid 1 (rho ~ 0.9) is inside the window
    s = set_of(w)
    s.run(n)
    mass = s.get_fields(("f",))["f"].astype(np.float64).sum(axis=(0, 1, 3))
    assert abs(mass[1] - (w["f0"][:, :, 1].astype(np.float64).sum() + n * 1e-3 * cells)) <= cells * tol["rho"]
    assert abs(mass[0] - w["f0"][:, :, 0].astype(np.float64).sum()) <= cells * tol["rho"]


@pytest.mark.parametrize("bc", ("periodic", "zero_gradient"))
def test_uniform_fluid_accelerates_uniformly(lbhip, bc):
    """One uniform fluid under constant g: sum f c = n rho g and u_b = (n - 1/2) g after n steps."""
    from LB_D2Q9.coupled import Shan_Chen_Fluids
    nx, ny, n, rho, gx, gy = 16, 8, 6, 0.8, 1e-3, -2e-3
    s = Shan_Chen_Fluids(nx, ny, [1.25], bc=bc)
    s.set_body_force(0, gx, gy)
    s.set_f(np.broadcast_to((rho * W64).astype(F), (nx, ny, 1, 9)))
    s.run(n)
    g = s.get_fields(ALL)
    f = g["f"].astype(np.float64)[:, :, 0]
    from multifluid_model import CX, CY
    tol = contract_tol(n)
    assert np.abs((f * CX).sum(axis=2) - n * rho * gx).max() <= tol["u"] and np.abs((f * CY).sum(axis=2) - n * rho * gy).max() <= tol["u"]
    assert np.abs(g["u_bary"] - (n - 0.5) * gx).max() <= tol["u"] and np.abs(g["v_bary"] - (n - 0.5) * gy).max() <= tol["u"]


def test_self_term_acts_twice(lbhip):
    """(0, 0, G) on one fluid = what fluid 0 feels from (0, 1, 2 G) with a copy of itself."""
    rng = np.random.default_rng(5)
    f0 = (W64 * 0.7 * (1. + 0.05 * rng.uniform(-1, 1, (21, 13, 1, 9)))).astype(F)
    one = dict(nx=21, ny=13, bc="periodic", omega=[1.25], g=np.zeros((1, 2)), interactions=np.array([[0, 0, -1.5, 1, 1.]]), reactions=np.zeros((0, 6)), f0=f0)
    two = dict(one, omega=[1.25, 1.25], g=np.zeros((2, 2)), interactions=np.array([[0, 1, -3., 1, 1.]]), f0=np.concatenate([f0, f0], axis=2))
    a, b = set_of(one), set_of(two)
    for s in (a, b):
        s.update_hydro()
        s.update_forces()
    ga, gb = a.get_fields(("Gx", "Gy")), b.get_fields(("Gx", "Gy"))
    assert np.abs(ga["Gx"]).max() > 1e-4
    for k in ("Gx", "Gy"):
        assert np.abs(ga[k][:, :, 0].astype(np.float64) - gb[k][:, :, 0]).max() <= 2. ** -22 * np.abs(ga[k]).max()


def test_empty_cell_gives_nan_bary_velocity_there_only(lbhip):
    """Every link that streams into (7, 5) is empty: after the step's streaming the cell holds no fluid.  The run and the phases."""
    from multifluid_model import CX, CY
    d = random_case(21, 13, "periodic", 2, 15)
    for k in range(9):
        d["f0"][7 - CX[k], 5 - CY[k], :, k] = 0
    a, b, c = set_of(d), set_of(d), set_of(d)
    a.run(1)
    for stage in ("move", "move_bcs", "update_hydro", "update_forces", "update_bary_velocity"):
        getattr(b, stage)()
    c.set_variant(1)
    c.run(1)
    for s in (a, b, c):
        g = s.get_fields(("rho", "u", "v", "u_bary", "v_bary"))
        nan = np.isnan(g["u_bary"])
        assert nan[7, 5] and nan.sum() == 1 and np.isnan(g["v_bary"][7, 5]) and np.isnan(g["v_bary"]).sum() == 1
        assert not np.any(g["rho"][7, 5]) and not np.any(g["u"][7, 5]) and not np.any(g["v"][7, 5])
        assert np.isfinite(g["u"]).all() and np.isfinite(g["v"]).all()


# ---- the drop-in classes -------------------------------------------------------------------------------------------------------
def _runner(d, rho=None):
    from LB_D2Q9.multicomponent_multiphase import multi
    nf = len(d["omega"])
    sim = multi.Simulation_Runner(nx=int(d["nx"]), ny=int(d["ny"]), num_populations=nf)
    if rho is not None:
        sim.set_bary_velocity(d["ub_in"], d["vb_in"])
    for i in range(nf):
        fl = multi.Fluid(sim, i, d["nu"][i], bc=str(d["bc"]))
        assert fl.omega == F(d["omega"][i])
        sim.add_fluid(fl)
        if rho is not None:
            fl.initialize(rho[:, :, i], f_amp=0.)
    sim.complete_setup()
    return sim


def test_dropin_initialize_reproduces_init_fixture(lbhip):
    d = golden("mc_init_21x13")
    sim = _runner(d, d["rho_in"])
    g = sim.get_fields()
    assert g["f"].shape == (21, 13, 2, 9) and g["f"].flags["F_CONTIGUOUS"] and g["rho"].shape == (21, 13, 2) and g["u_bary"].shape == (21, 13)
    tol = contract_tol(1)["f"]
    assert np.abs(g["f"] - d["f"]).max() <= tol and np.abs(g["feq"] - d["feq"]).max() <= tol
    assert np.array_equal(np.asarray(sim.rho), d["rho_in"].astype(F))


def test_dropin_run_reproduces_a_run_fixture(lbhip):
    d = golden("mc_react_21x13")
    sim = _runner(d)
    for r in d["interactions"]:
        sim.add_interaction_force(int(r[0]), int(r[1]), r[2], bc=str(d["bc"]), potential=POTENTIALS[int(r[3])], potential_parameters=[r[4]])
    sim.add_eating_rate(0, 1, d["reactions"][0][3], d["reactions"][0][4])
    sim.add_growth(1, *d["reactions"][1][3:6])
    sim.engine.set_f(d["f0"])
    sim.run(5)
    g = sim.get_fields()
    m = from_fixture(d, F)
    compare("drop-in after 5 steps", m, 5, {dict(u_bary="ub", v_bary="vb").get(k, k): v for k, v in g.items()}, recorded(d, 5))
    with pytest.raises(NotImplementedError, match="vdw"):
        sim.add_interaction_force(0, 1, 1., potential="vdw", potential_parameters=[1., 1., 1., 1.])


# ---- checkpoints, selection, refusals ----------------------------------------------------------------------------------------------
def test_checkpoint_resumes_bitwise_tables_included(lbhip, tmp_path):
    from LB_D2Q9.coupled import Shan_Chen_Fluids
    d = random_case(37, 23, "zero_gradient", 3, 17, field=True)
    a = set_of(d)
    a.run(4)
    a.save_checkpoint(os.path.join(str(tmp_path), "set"))
    b = Shan_Chen_Fluids.from_checkpoint(os.path.join(str(tmp_path), "set"))
    assert b.members[0].interactions == a.members[0].interactions and b.members[0].reactions == a.members[0].reactions
    assert len(b.members[0].interactions) == 6 and len(b.members[0].reactions) == 4
    assert not same_bits(a.get_fields(ALL), b.get_fields(ALL))
    a.run(3)
    b.run(3)
    assert not same_bits(a.get_fields(ALL), b.get_fields(ALL))
    # one handle on its own: Simulation's checkpoint carries its tables
    from LB_D2Q9.simulation import Simulation
    one = random_case(21, 13, "periodic", 1, 18)
    s = set_of(one)
    s.run(2)
    s.members[0].save_checkpoint(os.path.join(str(tmp_path), "one"))
    t = Simulation.from_checkpoint(os.path.join(str(tmp_path), "one"))
    assert t.semantics == "multifluid" and t.interactions == s.members[0].interactions and t.reactions == s.members[0].reactions
    s.run(3)
    t.run(3)
    assert not same_bits(s.members[0].get_fields(ALL), t.get_fields(ALL))


def test_hot_kernel_and_variant_selection(lbhip):
    from LB_D2Q9._native import LbError
    s = set_of(random_case(21, 13, "zero_gradient", 2, 19, field=True))
    for v in (-1, 0, 1):
        s.set_variant(v)
        name = s.hot_kernel()
        if v == 0:
            assert name.startswith("k_mc_moments + k_mc_collide ")
        else:                                   # (the planner's choice is the one-launch step: profiles/multifluid_bench.txt)
            assert name.startswith("k_mc_step ") and "k_mc_moments" not in name
        assert "ZERO_GRADIENT" in name and "FIELD" in name and s.members[0].steps_per_launch() == 1
        s.run(2)
    for v in (2, -2, 512):
        with pytest.raises(LbError, match="LB_SEM_MULTIFLUID"):
            s.set_variant(v)


def test_refusals_are_status_codes_in_both_directions(lbhip):
    """What makes no sense on a fluid of a set names LB_SEM_MULTIFLUID; the set calls refuse every other kind of handle."""
    from LB_D2Q9._native import FluidReaction, Interaction, LbError
    from LB_D2Q9.simulation import Simulation
    L = lbhip
    s = set_of(random_case(16, 12, "periodic", 2, 20))
    h, hs = s.members[0]._h, s._handles
    buf = np.zeros(4096, F)
    p = buf.ctypes.data
    i0 = ct.c_int()
    refused = dict(
        lb_set_mask=lambda: L.lb_set_mask(h, p), lb_set_mask_halo=lambda: L.lb_set_mask_halo(h, None, None),
        lb_step_boundary=lambda: L.lb_step_boundary(h, 0), lb_step_interior=lambda: L.lb_step_interior(h, 0),
        lb_step_finish=lambda: L.lb_step_finish(h), lb_halo_export=lambda: L.lb_halo_export(h, 0, p),
        lb_halo_import=lambda: L.lb_halo_import(h, 0, p), lb_halo_floats=lambda: L.lb_halo_floats(h),
        lb_run_group=lambda: L.lb_run_group(hs, 2, 1), lb_set_slab_cycle=lambda: L.lb_set_slab_cycle(h, 3),
        lb_autotune=lambda: L.lb_autotune(h), lb_autotune_quick=lambda: L.lb_autotune_quick(h, 100),
        lb_set_variant=lambda: L.lb_set_variant(h, 512), lb_run_batch=lambda: L.lb_run_batch(hs, 2, 1),
        lb_run_coupled=lambda: L.lb_run_coupled(hs, 2, 1), lb_solve=lambda: L.lb_solve(h, 1, None, None, None),
        lb_solve_reset=lambda: L.lb_solve_reset(h), lb_get_solve_state=lambda: L.lb_get_solve_state(h, ct.byref(i0), ct.byref(i0)),
        lb_set_poisson=lambda: L.lb_set_poisson(h, 0., 1., 1e-6), lb_gradient=lambda: L.lb_gradient(h, 0.5, None, None),
        lb_set_reaction=lambda: L.lb_set_reaction(h, 0.1), lb_set_velocity_from=lambda: L.lb_set_velocity_from(h, h),
        lb_check=lambda: L.lb_check(h, 0, None, None, None), lb_get_corner_state=lambda: L.lb_get_corner_state(h, p),
        lb_set_corner_state=lambda: L.lb_set_corner_state(h, p), lb_edge_floats=lambda: L.lb_edge_floats(h),
        lb_zero_velocity_in_obstacle=lambda: L.lb_zero_velocity_in_obstacle(h), lb_set_porous=lambda: L.lb_set_porous(h, 1., 0., 1., 0.))
    for name, call in refused.items():
        assert call() == -3, name                                   # LB_ERR_STATE
        msg = L.lb_last_error()
        assert b"LB_SEM_MULTIFLUID" in msg and name.encode() in msg, (name, msg)
    s.run(3)                                                        # none of it disturbed the set
    assert np.isfinite(s.get_fields(("f",))["f"]).all()
    # argument errors of the tables
    bad = (Interaction * 1)(Interaction(0, 1, 0, 1, 1., 0.))         # the other family's stencil rule
    assert L.lb_set_interactions(hs, 2, bad, 1) == -1 and b"family" in L.lb_last_error()
    bad = (Interaction * 1)(Interaction(0, 2, 0, 0, 1., 0.))         # a fluid outside the set
    assert L.lb_set_interactions(hs, 2, bad, 1) == -1
    bad = (Interaction * 1)(Interaction(0, 1, 3, 0, 1., 0.))         # vdw
    assert L.lb_set_interactions(hs, 2, bad, 1) == -1 and b"vdw" in L.lb_last_error()
    assert L.lb_set_interactions(hs, 2, bad, 7) == -1
    eat_self = (FluidReaction * 1)(FluidReaction(0, 1, 1, 1e-3, 0.5, 0.))
    assert L.lb_set_reactions(hs, 2, eat_self, 1) == -1 and L.lb_set_reactions(hs, 2, eat_self, 5) == -1
    assert L.lb_run_fluids(hs, 4, 1) == -1 and b"more than 3" in L.lb_last_error()
    twice = (ct.c_void_p * 2)(h, h)
    assert L.lb_run_fluids(twice, 2, 1) == -1
    # a set whose first handle's table names more fluids than the call brings
    assert L.lb_run_fluids(hs, 1, 1) == -3 and b"table" in L.lb_last_error()
    # different families in one set
    z = Simulation(16, 12, 1.25, bc="zero_gradient", semantics="multifluid")
    mixed = (ct.c_void_p * 2)(h, z._h)
    assert L.lb_run_fluids(mixed, 2, 1) == -1 and b"different families" in L.lb_last_error()
    # ... and the other direction
    others = [Simulation(16, 12, 1.25, bc="periodic"), Simulation(16, 12, 1.25, bc="periodic", semantics="porous"),
              Simulation(16, 12, 1.25, bc="periodic", semantics="diffusion")]
    for o in others:
        one = (ct.c_void_p * 1)(o._h)
        for name in ("lb_run_fluids",):
            assert getattr(L, name)(one, 1, 1) == -3 and b"LB_SEM_MULTIFLUID" in L.lb_last_error(), (o.semantics, name)
        for name in ("lb_update_forces_fluids", "lb_update_bary_fluids", "lb_react_fluids"):
            assert getattr(L, name)(one, 1) == -3 and b"LB_SEM_MULTIFLUID" in L.lb_last_error(), (o.semantics, name)
        assert L.lb_set_interactions(one, 1, None, 0) == -3 and L.lb_set_reactions(one, 1, None, 0) == -3
        assert L.lb_get_interactions(o._h, None, None) == -3 and L.lb_get_reactions(o._h, None, None) == -3
    with pytest.raises(LbError, match="LB_SEM_POROUS"):              # the porous calls' wording survives on other handles
        others[0].set_body_force(1e-3, 0.)
    with pytest.raises(NotImplementedError, match="more than 3"):
        from LB_D2Q9.coupled import Shan_Chen_Fluids
        Shan_Chen_Fluids(16, 12, [1., 1., 1., 1.])
