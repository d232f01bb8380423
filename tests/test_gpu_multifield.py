"""Coupled scalar lattices on the GPU: k_mf_step and the un-fused phases against the fixtures recorded from the reference's C and
against the numpy model (tests/multifield_model.py), through Coupled_Scalars and through Fisher_Expansion; the corner state,
checkpoints, the coupling to a flow handle, lb_run_coupled's refusals.  Bounds: the project's parity contract (contract_tol)."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from multifield_model import CORNER_LINKS, MultifieldModel, W, contract_tol

pytestmark = pytest.mark.gpu

RUN_FIXTURES = ("mf_box_37x23", "mf_fisher_37x23", "mf_box_5x4")
OMEGAS, GS = (0.9, 1.3, 1.1, 1.25), (0.02, 0.01, 0.015, 0.005)


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def assert_close(got, want, n, keys=("f", "rho"), what=""):
    """max |got - want| within the contract for n steps (feq is held to f's bound); prints the measured margins."""
    tol = contract_tol(n)
    tol["feq"] = tol["f"]
    meas = {k: maxdiff(got[k], want[k]) for k in keys}
    print("%s after %d steps, measured / bound: %s" % (what, n, ", ".join("%s %.2e / %.1e" % (k, meas[k], tol[k]) for k in keys)))
    for k in keys:
        assert meas[k] <= tol[k], "%s %s: %.3e > %.1e" % (what, k, meas[k], tol[k])


def load(c, d):
    """the state of a fixture / case d into a Coupled_Scalars or a MultifieldModel"""
    c.set_fields(np.zeros(d["f0"].shape[:3], np.float32), d["u"], d["v"])
    c.set_f(d["f0"])
    if int(d["corner_zero"]):
        c.set_corner_state(np.zeros((d["f0"].shape[2], 8), np.float32))
    return c


def set_of(d, bc="box", **kw):
    from LB_D2Q9.coupled import Coupled_Scalars
    return load(Coupled_Scalars(int(d["nx"]), int(d["ny"]), d["omega"], d["G"], bc=bc, **kw), d)


def model_of(d, bc="box"):
    return load(MultifieldModel(int(d["nx"]), int(d["ny"]), d["omega"], d["G"], bc), d)


def random_case(nx, ny, nf, seed, Gs=GS, flow=True):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    f0 = np.zeros((nx, ny, nf, 9), np.float32)
    for i in range(nf):
        rho = 0.03 + (0.7 / nf) * np.exp(-(((x - (0.3 + 0.1 * i) * nx) / (0.3 * nx)) ** 2 + ((y - 0.5 * ny) / (0.35 * ny)) ** 2))
        f0[:, :, i, :] = W[None, None, :] * rho[:, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))
    u = (0.07 * np.sin(2. * np.pi * y / ny) * np.cos(2. * np.pi * x / nx) if flow else 0. * x).astype(np.float32)
    v = (-0.07 * np.cos(2. * np.pi * y / ny) * np.sin(2. * np.pi * x / nx) if flow else 0. * x).astype(np.float32)
    return dict(nx=nx, ny=ny, f0=f0, u=u, v=v, omega=np.array(OMEGAS[:nf], np.float32), G=np.array(Gs[:nf], np.float32), corner_zero=0)


# ---- the fixtures (the reference's box) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_fused_run_follows_reference_fixture_and_model(lbhip, name):
    d = golden(name)
    s, m = set_of(d), model_of(d)
    done = 0
    for n in [int(k) for k in d["steps"]]:
        s.run(n - done)
        m.run(n - done)
        done = n
        got = s.get_fields()
        assert_close(got, dict(f=d["f_%d" % n], rho=d["rho_%d" % n]), n, what=name + " fused")
        assert_close(got, m.get_fields(), n, what=name + " fused vs model")
        assert np.array_equal(got["u"], d["u"]) and np.array_equal(got["v"], d["v"])        # lb_run_coupled never writes u, v
    s.close()


def test_fisher_expansion_follows_reference_fixture(lbhip):
    from LB_D2Q9.advecting_range_expansion.deterministic_fisher_waves import Fisher_Expansion, inoculation_stripes
    d = golden("mf_fisher_37x23")
    fe = Fisher_Expansion(Lx=10., Ly=6., mu_list=[0.49, 0.588], D_list=[2. / 3., 4. / 9.], N=7,
                          initial_frac_widths=[0.5, 0.5], initial_frac_indices=[0, 1])
    assert (fe.nx, fe.ny, int(fe.num_populations)) == (37, 23, 2)
    assert np.array_equal(fe.omega, d["omega"]) and np.array_equal(fe.lb_G, d["G"])
    # the class's own start: stripes at equilibrium, the never-written corner links zero (its f_temporary starts as zeros)
    g = fe.get_fields()
    assert np.array_equal(g["rho"], inoculation_stripes(37, 23, 2, [0.5, 0.5], [0, 1], 14)) and g["f"].shape == (37, 23, 2, 9)
    assert maxdiff(g["f"], W * g["rho"][..., None]) <= 1e-7 and not fe.sim.get_corner_state().any()
    # the fixture's state through the class's engine (load() zeroes the corner links again, as init_f does behind set_f)
    load(fe.sim, d)
    done = 0
    for n in [int(k) for k in d["steps"]]:
        fe.run(n - done)
        done = n
        assert_close(fe.get_fields(), dict(f=d["f_%d" % n], rho=d["rho_%d" % n]), n, what="Fisher_Expansion")
    assert np.asarray(fe.rho).shape == (37, 23, 2) and fe.get_physical_fields()["u"].shape == (37, 23)
    fe.sim.close()


def test_single_phases_follow_reference_fixture(lbhip):
    d = golden("mf_phases_21x13")
    s = set_of(d)
    tol = contract_tol(1)
    s.move()
    assert np.array_equal(s.get_fields(("f",))["f"], d["f_move"])
    s.move_bcs()
    assert np.array_equal(s.get_fields(("f",))["f"], d["f_bcs"])
    s.update_hydro()
    g = s.get_fields(("rho", "u", "v"))
    assert maxdiff(g["rho"], d["rho_hydro"]) <= tol["rho"] and np.array_equal(g["u"], d["u"]) and np.array_equal(g["v"], d["v"])
    s.update_feq()
    assert maxdiff(s.get_fields(("feq",))["feq"], d["feq_feq"]) <= tol["f"]
    s.collide_particles()
    assert maxdiff(s.get_fields(("f",))["f"], d["f_collide"]) <= tol["f"]
    t = set_of(d)                                   # and the fused step from the same start
    t.run(1)
    assert_close(t.get_fields(), dict(f=d["f_collide"], rho=d["rho_hydro"], feq=d["feq_feq"]), 1, ("f", "rho", "feq"), "mf_phases fused")
    s.close(); t.close()


def test_phases_after_a_fused_run_keep_the_corner_links(lbhip):
    """lb_move after lb_run_coupled: the second lattice no longer is the reference's f_streamed; the corner state stands in."""
    d = golden("mf_box_37x23")
    s = set_of(d)
    s.run(7)
    for _ in range(3):
        s.move(); s.move_bcs(); s.update_hydro(); s.update_feq(); s.collide_particles()
    assert_close(s.get_fields(), dict(f=d["f_10"], rho=d["rho_10"]), 10, what="7 fused + 3 phase steps")
    for j, (k, x, y) in enumerate(CORNER_LINKS):        # un-fused, those links sit in the lattice: still the values of set_f
        assert np.array_equal(s.get_corner_state()[:, j], d["f0"][x, y, :, k])
    s.close()


# ---- k_mf_step against the model: lanes holding both walls (5, 3), a wall inside a lane's last quad (37, 63, 255), a wall on a
#      wave boundary (64: pitch 64; 256 would be the next) and two cells past it (258), rows not a multiple of four ---------------
SHAPES = [(37, 23), (63, 17), (64, 16), (255, 33), (258, 9), (5, 4), (3, 3), (1000, 12)]


@pytest.mark.parametrize("bc", ["box", "periodic"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_fused_step_follows_model(lbhip, shape, bc):
    nx, ny = shape
    n = 8 + nx % 6
    for nf in (1, 2, 3, 4):
        for Gs in ((0., 0., 0., 0.), GS):
            c = random_case(nx, ny, nf, 100 + nf, Gs)
            s, m = set_of(c, bc), model_of(c, bc)
            s.run(n)
            m.run(n)
            assert_close(s.get_fields(), m.get_fields(), n, what="%dx%d %s nf=%d G=%g" % (nx, ny, bc, nf, Gs[0]))
            s.close()


# ---- bitwise ---------------------------------------------------------------------------------------------------------------
def test_one_periodic_field_equals_the_scalar_lattice_bitwise(lbhip):
    from LB_D2Q9.simulation import Simulation
    from LB_D2Q9.variants import K_STEP
    c = random_case(70, 19, 1, 7)
    s = set_of(c, "periodic")
    t = Simulation(70, 19, float(c["omega"][0]), bc="periodic", semantics="diffusion")
    t.set_variant(K_STEP)
    t.set_reaction(float(c["G"][0]))
    t.set_fields(np.zeros((70, 19), np.float32), c["u"], c["v"])
    t.set_f(c["f0"][:, :, 0, :])
    s.run(11); t.run(11)
    a, b = s.get_fields(("f", "rho")), t.get_fields(("f", "rho"))
    assert np.array_equal(a["f"][:, :, 0, :], b["f"]) and np.array_equal(a["rho"][:, :, 0], b["rho"])
    s.close(); t.close()


@pytest.mark.parametrize("bc", ["box", "periodic"])
def test_without_growth_a_set_equals_its_members_alone_bitwise(lbhip, bc):
    from LB_D2Q9.coupled import Coupled_Scalars
    c = random_case(45, 14, 3, 8, Gs=(0., 0., 0.))
    s = set_of(c, bc)
    s.run(9)
    a = s.get_fields(("f", "rho"))
    for i in range(3):
        one = Coupled_Scalars(45, 14, [c["omega"][i]], [0.], bc=bc)
        one.set_fields(np.zeros((45, 14, 1), np.float32), c["u"], c["v"])
        one.set_f(c["f0"][:, :, i:i + 1, :])
        one.run(9)
        b = one.get_fields(("f", "rho"))
        assert np.array_equal(a["f"][:, :, i], b["f"][:, :, 0]) and np.array_equal(a["rho"][:, :, i], b["rho"][:, :, 0])
        one.close()
    s.close()


@pytest.mark.parametrize("bc", ["box", "periodic"])
def test_split_runs_and_planar_layout_give_the_same_bits(lbhip, bc):
    c = random_case(66, 13, 3, 9)
    a, b, p = set_of(c, bc), set_of(c, bc), set_of(c, bc, planar=True)
    a.run(13)
    b.run(5); b.run(8)
    p.run(13)
    fa = a.get_fields(("f", "rho"))
    for other in (b, p):
        fo = other.get_fields(("f", "rho"))
        assert np.array_equal(fa["f"], fo["f"]) and np.array_equal(fa["rho"], fo["rho"])
    assert p.members[0].layout()["plane_stride"] != a.members[0].layout()["plane_stride"]
    for s in (a, b, p):
        s.close()


def test_checkpoint_restore_run_bitwise(lbhip):
    from LB_D2Q9.coupled import Coupled_Scalars
    c = random_case(37, 11, 2, 10)
    s = set_of(c)
    s.set_corner_state(s.get_corner_state() + np.float32(0.01))
    s.run(3)
    ck = [m.checkpoint_arrays() for m in s.members]
    assert all(k["corner_state"].shape == (8,) and str(k["semantics"]) == "multifield" for k in ck)
    s.run(6)
    t = Coupled_Scalars(37, 11, c["omega"], [0., 0.])            # (G comes back with the checkpoint)
    for m, k in zip(t.members, ck):
        m.restore_arrays(k)
    assert np.array_equal(t.get_corner_state(), s.get_corner_state())
    t.run(6)
    a, b = s.get_fields(("f", "rho")), t.get_fields(("f", "rho"))
    assert np.array_equal(a["f"], b["f"]) and np.array_equal(a["rho"], b["rho"])
    s.close(); t.close()


# ---- the corner state ------------------------------------------------------------------------------------------------------
def test_corner_state_is_the_models_and_the_kernel_reads_it(lbhip):
    c = random_case(21, 9, 2, 11)
    s, m = set_of(c), model_of(c)
    assert np.array_equal(s.get_corner_state(), m.get_corner_state()) and s.get_corner_state().shape == (2, 8)
    base = set_of(c)
    base.run(1)
    r0 = base.get_fields(("rho",))["rho"]
    for j, (k, x, y) in enumerate(CORNER_LINKS):
        for i in range(2):
            t = set_of(c)
            st = t.get_corner_state()
            st[i, j] += np.float32(0.25)
            t.set_corner_state(st)
            t.run(1)
            changed = np.argwhere(t.get_fields(("rho",))["rho"] != r0)
            assert changed.tolist() == [[x % 21, y % 9, i]], (j, i, changed)
            t.close()
    m.set_corner_state(m.get_corner_state() + np.float32(0.125))
    s.set_corner_state(m.get_corner_state())
    s.run(5); m.run(5)
    assert_close(s.get_fields(), m.get_fields(), 5, what="perturbed corner state")
    s.close(); base.close()


def test_set_velocity_from_equals_download_and_set_fields(lbhip):
    from LB_D2Q9.simulation import Simulation
    c = random_case(48, 20, 2, 12)
    flow = Simulation(48, 20, 1.2, bc="periodic")
    x, y = np.meshgrid(np.arange(48), np.arange(20), indexing="ij")
    flow.init_equilibrium(np.ones((48, 20), np.float32), (0.05 * np.sin(2 * np.pi * y / 20)).astype(np.float32),
                          (0.03 * np.cos(2 * np.pi * x / 48)).astype(np.float32))
    flow.run(6)
    a, b = set_of(c), set_of(c)
    a.set_velocity_from(flow)
    g = flow.get_fields(("u", "v"))
    b.set_fields(np.zeros((48, 20, 2), np.float32), g["u"], g["v"])
    for m in a.members:                             # every member got it
        assert np.array_equal(m.get_fields(("u",))["u"], g["u"])
    a.run(7); b.run(7)
    fa, fb = a.get_fields(("f", "rho")), b.get_fields(("f", "rho"))
    assert np.array_equal(fa["f"], fb["f"]) and np.array_equal(fa["rho"], fb["rho"]) and g["u"].any()
    a.close(); b.close(); flow.close()


# ---- the ABI's answers and refusals -------------------------------------------------------------------------------------------
def test_refusals_are_status_codes_and_the_planner_answers(lbhip):
    from LB_D2Q9.coupled import Coupled_Scalars
    from LB_D2Q9.simulation import Simulation
    a, b = Coupled_Scalars(16, 12, [1., 1.1], [0., 0.]), Coupled_Scalars(20, 12, [1.], [0.])
    p, d = Coupled_Scalars(16, 12, [1.], [0.], bc="periodic"), Simulation(16, 12, 1., bc="periodic", semantics="diffusion")
    H = lambda *sims: (ct.c_void_p * len(sims))(*[s._h for s in sims])
    m0, m1 = a.members
    for handles, n, word in ((H(m0, b.members[0]), 2, b"share grid"), (H(m0, p.members[0]), 2, b"boundary family"),
                             (H(m0, d), 2, b"LB_SEM_MULTIFIELD"), (H(m0, m0), 2, b"twice"), (H(m0), 0, b"1..4"),
                             (H(m0, m1, m0, m1, m0), 5, b"1..4")):
        assert lbhip.lb_run_coupled(handles, n, 1) == -1 and word in lbhip.lb_last_error(), lbhip.lb_last_error()
    assert lbhip.lb_run_coupled(H(m0, m1), 2, -1) == -1 and lbhip.lb_run_coupled(H(m0, m1), 2, 0) == 0
    assert lbhip.lb_run_batch(H(m0, m1), 2, 1) == -3 and lbhip.lb_set_mask(m0._h, None) == -3          # still scalar lattices
    assert lbhip.lb_set_variant(m0._h, 1 << 9) == -1 and lbhip.lb_set_variant(m0._h, 0) == 0 and lbhip.lb_set_variant(m0._h, -1) == 0
    assert m0.steps_per_launch() == 1 and m0.plan_launches(3) == [1, 1, 1] and m0.edge_floats() == 0
    assert m0.hot_kernel().startswith("k_mf_step") and m0.hot_kernel().endswith("<BOX>") and p.members[0].hot_kernel().endswith("<PERIODIC>")
    c = random_case(16, 12, 2, 13)
    load(a, c)
    a.run(4)
    for i, chk in enumerate(a.check()):
        assert chk["n_nonfinite"] == 0 and np.isfinite(chk["sum_rho"])
        assert chk["sum_rho"] == pytest.approx(float(a.get_fields(("f",))["f"][:, :, i].astype(np.float64).sum()), rel=1e-6)
    assert m0.layout()["pitch"] == 64
    for s in (a, b, p, d):
        s.close()
