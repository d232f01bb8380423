"""Scalar lattices on the GPU: k_ad_step and the un-fused phases against the fixtures recorded from the reference's C and against
the numpy model (tests/scalar_model.py), through the C ABI (Simulation) and through the drop-in classes; the edge state, the
coupling to a flow handle, checkpoints, mass and the diffusion law.  Bounds: the project's parity contract (contract_tol)."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from LB_D2Q9.variants import AUTO, K_STEP, TILES
from scalar_model import ScalarModel, W, contract_tol

pytestmark = pytest.mark.gpu

RUN_FIXTURES = ("ad_diffusion_37x23", "ad_advection_37x23", "ad_fisher_37x23")


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def assert_close(got, want, n, keys=("f", "rho", "feq"), what=""):
    """max |got - want| within the contract for n steps (feq is held to f's bound); prints the measured margins."""
    tol = contract_tol(n)
    tol["feq"] = tol["f"]
    meas = {k: maxdiff(got[k], want[k]) for k in keys}
    print("%s after %d steps, measured / bound: %s" % (what, n, ", ".join("%s %.2e / %.1e (%.0f %%)" % (k, meas[k], tol[k], 100. * meas[k] / tol[k]) for k in keys)))
    for k in keys:
        assert meas[k] <= tol[k], "%s %s: %.3e > %.1e" % (what, k, meas[k], tol[k])


def sim_of(d, bc="open", **kw):
    from LB_D2Q9.simulation import Simulation
    s = Simulation(int(d["nx"]), int(d["ny"]), float(d["omega"]), bc=bc, semantics="diffusion", **kw)
    s.set_reaction(float(d["G"]))
    s.set_fields(np.zeros_like(d["u"]), d["u"], d["v"])
    s.set_f(d["f0"])
    return s


def random_case(nx, ny, seed, flow=True):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    rho = 0.2 + 0.7 * np.exp(-(((x - 0.45 * nx) / (0.2 * nx)) ** 2 + ((y - 0.5 * ny) / (0.25 * ny)) ** 2))
    f0 = (W[None, None, :] * rho[:, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(np.float32)
    u = (0.07 * np.sin(2. * np.pi * y / ny) * np.cos(2. * np.pi * x / nx) if flow else 0. * x).astype(np.float32)
    v = (-0.07 * np.cos(2. * np.pi * y / ny) * np.sin(2. * np.pi * x / nx) if flow else 0. * x).astype(np.float32)
    return dict(nx=nx, ny=ny, f0=f0, u=u, v=v)


def pair(nx, ny, omega, G, bc, seed, flow=True):
    """a GPU handle and the model in the same state"""
    c = random_case(nx, ny, seed, flow)
    c.update(omega=np.float32(omega), G=np.float32(G))
    s = sim_of(c, bc)
    m = ScalarModel(nx, ny, omega, G, bc)
    m.set_fields(np.zeros_like(c["u"]), c["u"], c["v"])
    m.set_f(c["f0"])
    return s, m, c


# ---- the fixtures (the reference's box: OPEN) ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_fused_run_follows_reference_fixture(lbhip, name):
    d = golden(name)
    s = sim_of(d)
    done = 0
    for n in [int(k) for k in d["steps"]]:
        s.run(n - done)
        done = n
        got = s.get_fields()
        assert_close(got, dict(f=d["f_%d" % n], rho=d["rho_%d" % n], feq=d["feq_%d" % n]), n, what=name + " fused")
        assert np.array_equal(got["u"], d["u"]) and np.array_equal(got["v"], d["v"])        # lb_run never writes u, v


@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_phase_by_phase_follows_reference_fixture(lbhip, name):
    d = golden(name)
    s = sim_of(d)
    n = int(d["steps"][1])                          # a recorded count: 10, 10, 200
    for _ in range(n):
        s.move(); s.move_bcs(); s.update_hydro(); s.update_feq(); s.collide_particles()
    assert_close(s.get_fields(), dict(f=d["f_%d" % n], rho=d["rho_%d" % n], feq=d["feq_%d" % n]), n, what=name + " phases")
    m = ScalarModel(int(d["nx"]), int(d["ny"]), d["omega"], d["G"], "open")
    m.set_fields(np.zeros_like(d["u"]), d["u"], d["v"]); m.set_f(d["f0"]); m.run(n)
    assert_close(s.get_fields(), m.get_fields(), n, what=name + " phases vs model")


def test_single_phases_follow_reference_fixture(lbhip):
    d = golden("ad_phases_21x13")
    s = sim_of(d)
    tol = contract_tol(1)
    s.move(); s.move_bcs()
    assert np.array_equal(s.get_fields(("f",))["f"], d["f_move"])
    s.update_hydro()
    g = s.get_fields(("rho", "u", "v"))
    assert maxdiff(g["rho"], d["rho_hydro"]) <= tol["rho"] and np.array_equal(g["u"], d["u"]) and np.array_equal(g["v"], d["v"])
    s.update_feq()
    assert maxdiff(s.get_fields(("feq",))["feq"], d["feq_feq"]) <= tol["f"]
    s.collide_particles()
    assert maxdiff(s.get_fields(("f",))["f"], d["f_collide"]) <= tol["f"]
    # and the fused step from the same start
    t = sim_of(d)
    t.run(1)
    assert_close(t.get_fields(), dict(f=d["f_collide"], rho=d["rho_hydro"], feq=d["feq_feq"]), 1, what="ad_phases fused")


def test_phases_after_a_fused_run_keep_the_edge_links(lbhip):
    """lb_move after lb_run: the second lattice no longer is the reference's f_streamed; the edge state stands in for it."""
    d = golden("ad_advection_37x23")
    s = sim_of(d)
    s.run(7)
    for _ in range(3):
        s.move(); s.move_bcs(); s.update_hydro(); s.update_feq(); s.collide_particles()
    assert_close(s.get_fields(), dict(f=d["f_10"], rho=d["rho_10"], feq=d["feq_10"]), 10, what="7 fused + 3 phase steps")


# ---- GPU against the model: both families, G = 0 and != 0, awkward widths, full-size boxes ------------------------------------
@pytest.mark.parametrize("bc", ["periodic", "open"])
@pytest.mark.parametrize("G", [0., 0.01])
@pytest.mark.parametrize("nx,ny,steps", [(37, 23, 13), (64, 16, 9), (130, 50, 12), (63, 17, 11), (255, 33, 8), (258, 70, 8),
                                         (4, 2, 5), (5, 3, 6)])
def test_step_kernel_follows_model_on_awkward_boxes(lbhip, bc, G, nx, ny, steps):
    s, m, _ = pair(nx, ny, 1.25, G, bc, seed=nx * 1000 + ny)
    s.run(steps)
    m.run(steps)
    assert_close(s.get_fields(), m.get_fields(), steps, what="%s %dx%d G=%g" % (bc, nx, ny, G))


@pytest.mark.parametrize("bc", ["periodic", "open"])
@pytest.mark.parametrize("n", [256, 1000])
def test_step_kernel_follows_model_full_size(lbhip, bc, n):
    steps = 40 if n == 256 else 12
    s, m, _ = pair(n, n, 1.6, 0.01, bc, seed=n)
    s.run(steps)
    m.run(steps)
    assert_close(s.get_fields(), m.get_fields(), steps, what="%s %d^2" % (bc, n))


# ---- k_ad_tile4 bitwise against k_ad_step ----------------------------------------------------------------------------------------
# widths that are and are not multiples of 4, 32 and 64; heights that are not multiples of 16; boxes smaller than one tile
TILE_BOXES = [(64, 48), (128, 50), (96, 33), (160, 17), (37, 23), (130, 50), (63, 17), (255, 33), (258, 70), (20, 10), (9, 5), (5, 3),
              (4, 2)]


def assert_same_bits(a, b, what):
    ga, gb = a.get_fields(("f", "rho")), b.get_fields(("f", "rho"))
    for k in ("f", "rho"):
        assert np.array_equal(ga[k], gb[k]), "%s: %s differs, max %.3e" % (what, k, maxdiff(ga[k], gb[k]))


@pytest.mark.parametrize("bc", ["periodic", "open"])
@pytest.mark.parametrize("G", [0., 0.01])
@pytest.mark.parametrize("shape", [0, 1, 2, 3])       # 0: by size; 1, 2, 3: 32 x 16 two cells per thread, 32 x 16 one, 16 x 16
def test_tile_kernel_equals_step_kernel_bitwise(lbhip, bc, G, shape):
    """K_STEP forces k_ad_step, TILES k_ad_tile4 for every group of four steps (the ROWS field: the shape).  Runs of
    1 ... 13 steps one after the other (1, 1 + 1, ..., 4 + 4 + 4 + 1), each compared bit for bit, on every box."""
    for nx, ny in TILE_BOXES:
        c = random_case(nx, ny, seed=nx * 100 + ny)
        c.update(omega=np.float32(1.35), G=np.float32(G))
        a, b = sim_of(c, bc), sim_of(c, bc)
        a.set_variant(K_STEP)
        b.set_variant(TILES | (shape << 2))         # (shape 1, 2: TILES | ROWS_1, TILES | ROWS_2)
        assert a.plan_launches(13) == [1] * 13 and b.plan_launches(13) == [4, 4, 4, 1] and b.plan_launches(3) == [1, 1, 1]
        assert a.hot_kernel().startswith("k_ad_step") and b.hot_kernel().startswith("k_ad_tile4")
        assert a.steps_per_launch() == 1 and b.steps_per_launch() == 4
        for n in range(1, 14):
            a.run(n); b.run(n)
            assert_same_bits(a, b, "%s %dx%d G=%g shape %d, run(%d)" % (bc, nx, ny, G, shape, n))


@pytest.mark.parametrize("bc", ["periodic", "open"])
@pytest.mark.parametrize("G", [0., 0.01])
def test_tile_kernel_equals_step_kernel_bitwise_long_run(lbhip, bc, G):
    for (nx, ny), shape in zip([(258, 70), (130, 50), (1000, 130)], [1, 3, 2]):
        c = random_case(nx, ny, seed=nx + ny)
        c.update(omega=np.float32(1.7), G=np.float32(G))
        a, b = sim_of(c, bc), sim_of(c, bc)
        a.set_variant(K_STEP)
        b.set_variant(TILES | (shape << 2))         # (shape 1, 2: TILES | ROWS_1, TILES | ROWS_2)
        a.run(403); b.run(403)
        assert_same_bits(a, b, "%s %dx%d G=%g shape %d, 403 steps" % (bc, nx, ny, G, shape))


def test_tile_kernel_follows_model_and_fixture(lbhip):
    d = golden("ad_fisher_37x23")
    s = sim_of(d)
    s.set_variant(TILES)
    s.run(200)
    assert_close(s.get_fields(), dict(f=d["f_200"], rho=d["rho_200"], feq=d["feq_200"]), 200, what="ad_fisher tiles")
    for bc in ("periodic", "open"):
        t, m, _ = pair(256, 256, 1.6, 0.01, bc, seed=77)
        t.set_variant(TILES)
        t.run(40); m.run(40)
        assert_close(t.get_fields(), m.get_fields(), 40, what="%s 256^2 tiles" % bc)


def test_automatic_choice_follows_the_size_rule(lbhip):
    """AUTO: the planner's size rule (plan.cpp, from profiles/scalar_bench.txt): k_ad_tile4 on boxes of 256^2 ... 8192^2 cells,
    k_ad_step below -- and whichever it picks, the bits are k_ad_step's."""
    for n, want in ((96, [1] * 9), (700, [4, 4, 1])):
        c = random_case(n, n, seed=n)
        c.update(omega=np.float32(1.2), G=np.float32(0.))
        a, b = sim_of(c, "open"), sim_of(c, "open")
        a.set_variant(K_STEP)
        plan = b.plan_launches(9)
        assert plan == want and (b.steps_per_launch() == 4) == (plan[0] == 4)
        assert b.hot_kernel().startswith("k_ad_tile4" if plan[0] == 4 else "k_ad_step")
        a.run(9); b.run(9)
        assert_same_bits(a, b, "automatic %d^2" % n)


def test_planar_layout_gives_the_same_bits(lbhip):
    c = random_case(130, 50, 5)
    c.update(omega=np.float32(1.1), G=np.float32(0.01))
    a, b = sim_of(c, "open"), sim_of(c, "open", planar=True)
    a.run(9); b.run(9)
    ga, gb = a.get_fields(), b.get_fields()
    for k in ("f", "rho", "feq"):
        assert np.array_equal(ga[k], gb[k]), k


def test_run_in_pieces_equals_run_at_once(lbhip):
    c = random_case(130, 50, 6)
    c.update(omega=np.float32(0.8), G=np.float32(0.02))
    for bc in ("periodic", "open"):
        a, b = sim_of(c, bc), sim_of(c, bc)
        a.run(13)
        for k in (1, 4, 5, 3):
            b.run(k)
        ga, gb = a.get_fields(), b.get_fields()
        for k in ("f", "rho"):
            assert np.array_equal(ga[k], gb[k]), (bc, k)


# ---- edge state ------------------------------------------------------------------------------------------------------------
def test_edge_state_is_the_models_and_is_read_by_the_kernel(lbhip):
    s, m, c = pair(37, 23, 1.2, 0., "open", seed=3)
    e = s.get_edge_state()
    assert e.shape == (6 * (37 + 23),) and np.array_equal(e, m.get_edge_state())
    rng = np.random.default_rng(9)
    e2 = (e * (1. + 0.2 * rng.uniform(-1., 1., e.shape))).astype(np.float32)
    s.set_edge_state(e2)
    m.set_edge_state(e2)
    assert np.array_equal(s.get_edge_state(), m.get_edge_state())      # (the column's entry in both places of a shared corner link)
    s.run(10); m.run(10)
    assert_close(s.get_fields(), m.get_fields(), 10, what="perturbed edge state")
    s.set_f(c["f0"])                                                    # lb_set_f resets it
    assert np.array_equal(s.get_edge_state(), e)
    p = pair(16, 12, 1.2, 0., "periodic", seed=4)[0]
    assert p.edge_floats() == 0 and p.get_edge_state().shape == (0,)


def test_checkpoint_restore_run_is_bitwise_open_with_perturbed_edge_state(lbhip, tmp_path):
    from LB_D2Q9.simulation import Simulation
    s, _, _ = pair(130, 50, 1.3, 0.01, "open", seed=8)
    e = s.get_edge_state()
    s.set_edge_state((e * np.float32(1.1)).astype(np.float32))
    s.run(7)
    s.save_checkpoint(tmp_path / "ck")
    s.run(9)
    t = Simulation.from_checkpoint(tmp_path / "ck")
    assert t.semantics == "diffusion" and t.G == s.G and np.array_equal(t.get_edge_state(), s.get_edge_state())
    t.run(9)
    gs, gt = s.get_fields(), t.get_fields()
    for k in ("f", "rho", "u", "v", "feq"):
        assert np.array_equal(gs[k], gt[k]), k


# ---- the coupling ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eager", [False, True])
def test_set_velocity_from_equals_download_and_set_fields(lbhip, eager):
    from LB_D2Q9.simulation import Simulation
    nx, ny = 200, 96
    rng = np.random.default_rng(2)
    flow = Simulation(nx, ny, 1.5, bc="periodic", eager_macro=eager)
    flow.set_f((W[None, None, :] * (1. + 0.02 * rng.standard_normal((nx, ny, 9)))).astype(np.float32))
    flow.run(25, wait=False)                                   # (not waited for: the copy is ordered behind it on the device)
    a, _, c = pair(nx, ny, 1.2, 0.005, "periodic", seed=1)
    b = sim_of(dict(c, omega=np.float32(1.2), G=np.float32(0.005)), "periodic")
    a.set_velocity_from(flow)
    g = flow.get_fields(("u", "v"))
    rho_b = b.get_fields(("rho",))["rho"]
    b.set_fields(rho_b, g["u"], g["v"])
    ga = a.get_fields(("u", "v"))
    assert np.array_equal(ga["u"], g["u"]) and np.array_equal(ga["v"], g["v"]) and float(np.abs(g["u"]).max()) > 0.
    a.run(11); b.run(11)
    ga, gb = a.get_fields(), b.get_fields()
    for k in ("f", "rho", "u", "v"):
        assert np.array_equal(ga[k], gb[k]), k
    # refusals: another grid, a scalar handle as the source, a flow handle as the target
    other = Simulation(nx + 4, ny, 1.5, bc="periodic")
    assert lbhip.lb_set_velocity_from(a._h, other._h) == -1 and b"grid" in lbhip.lb_last_error()
    assert lbhip.lb_set_velocity_from(a._h, b._h) == -1
    assert lbhip.lb_set_velocity_from(flow._h, flow._h) == -3


# ---- what a scalar handle answers ----------------------------------------------------------------------------------------------
def test_introspection_and_refusals_on_a_scalar_handle(lbhip):
    s, m, c = pair(96, 40, 1.2, 0.01, "open", seed=7)
    s.set_variant(K_STEP)
    assert s.plan_launches(6) == [1] * 6 and s.steps_per_launch() == 1
    assert s.hot_kernel().startswith("k_ad_step") and s.hot_kernel().endswith("<OPEN>")
    s.set_variant(AUTO)
    chk = s.check()
    assert chk["n_nonfinite"] == 0
    assert chk["sum_rho"] == pytest.approx(float(c["f0"].astype(np.float64).sum()), rel=1e-6)
    assert chk["max_mach"] == pytest.approx(float(np.sqrt(3. * (c["u"].astype(np.float64) ** 2 + c["v"].astype(np.float64) ** 2).max())), rel=1e-5)
    bad = c["f0"].copy()
    bad[5, 6, 2] = np.nan
    s.set_f(bad)
    assert s.check()["n_nonfinite"] == 1
    s.set_f(c["f0"])
    lay = s.layout()
    assert lay["pitch"] == 128
    s.set_variant(K_STEP); s.run(3); s.set_variant(TILES); s.run(6); s.set_variant(AUTO); s.run(2)
    m.run(11)
    assert_close(s.get_fields(), m.get_fields(), 11, what="variants")
    gbs, nbytes = s.copy_calibration(iters=2)
    assert nbytes > 0 and gbs > 0
    h = s._h
    buf = (ct.c_float * 4096)()
    mask = np.zeros((96, 40), np.int32, order="F")
    arr = (ct.c_void_p * 1)(h.value)
    for rc in (lbhip.lb_set_mask(h, mask.ctypes.data), lbhip.lb_set_mask_halo(h, None, None), lbhip.lb_step_boundary(h, 0),
               lbhip.lb_step_interior(h, 0), lbhip.lb_step_finish(h), lbhip.lb_halo_floats(h), lbhip.lb_halo_export(h, 0, buf),
               lbhip.lb_halo_import(h, 0, buf), lbhip.lb_comm_init(h, buf, 0, 1), lbhip.lb_peer_export(h, buf),
               lbhip.lb_peer_connect(h, 0, 1, None, None, 40), lbhip.lb_run_group(arr, 1, 1), lbhip.lb_run_batch(arr, 1, 1),
               lbhip.lb_autotune(h), lbhip.lb_autotune_quick(h, 10000), lbhip.lb_get_corner_state(h, buf),
               lbhip.lb_set_corner_state(h, buf)):
        assert rc == -3 and b"scalar lattice" in lbhip.lb_last_error()            # LB_ERR_STATE
    from LB_D2Q9.simulation import Simulation
    flow = Simulation(32, 32, 1.0, bc="periodic")
    for rc in (lbhip.lb_set_reaction(flow._h, 0.1), lbhip.lb_edge_floats(flow._h), lbhip.lb_get_edge_state(flow._h, buf),
               lbhip.lb_set_edge_state(flow._h, buf)):
        assert rc == -3


# ---- conservation and the diffusion law ----------------------------------------------------------------------------------------
def test_periodic_mass_drift_tracks_model(lbhip):
    """Periodic box, G = 0: sum(rho) is conserved up to the rounding bias of the float32 weights.  The GPU's relative drift per
    step stays within 5e-9 of the model's (the allowance test_periodic_mass_drift_tracks_reference gives the flow kernels
    against the oracle), checked after every block of steps."""
    n, block, blocks = 256, 50, 4
    s, m, c = pair(n, n, 1.7, 0., "periodic", seed=21)
    m0 = c["f0"].astype(np.float64).sum()
    for b in range(1, blocks + 1):
        s.run(block); m.run(block)
        steps = b * block
        drift = (s.get_fields(("f",))["f"].astype(np.float64).sum() - m0) / m0 / steps
        mdrift = (m.f.astype(np.float64).sum() - m0) / m0 / steps
        print("after %d steps: drift per step GPU %.3e, model %.3e" % (steps, drift, mdrift))
        assert abs(drift - mdrift) < 5e-9, (steps, drift, mdrift)


def test_gaussian_variance_grows_by_2Dt(lbhip):
    """The Gaussian of Diffusion (rho = exp(-(X^2 + Y^2)), N = 16 cells per unit length) on a 256^2 periodic box, omega = 1,
    300 steps: the variance of rho along either axis grows by 2 D t = 100 with D = (1 / omega - 1/2) / 3.  The numpy model
    (tests/scalar_model.py), run on the CPU on this very case, gives 228.00002366 - 128.00000065 along x and 227.99999847 -
    128.00000065 along y: deviations of +2.30e-5 and -2.2e-6 from 2 D t -- the scheme's own error (float32 rounding: the
    second moment of this scheme grows by exactly 2 D per step).  The GPU is allowed twice the larger: 4.6e-5."""
    from LB_D2Q9.reaction_diffusion.diffusion import gaussian_blob
    from LB_D2Q9.simulation import Simulation
    n, N, omega, steps = 256, 16, 1.0, 300
    _, _, _, _, rho = gaussian_blob(n, n, N)
    z = np.zeros((n, n), np.float32)
    s = Simulation(n, n, omega, bc="periodic", semantics="diffusion")
    s.init_equilibrium(rho, z, z)
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")

    def variances(f):
        r = f.astype(np.float64).sum(axis=2)
        t = r.sum()
        xc, yc = (r * x).sum() / t, (r * y).sum() / t
        return (r * (x - xc) ** 2).sum() / t, (r * (y - yc) ** 2).sum() / t
    v0 = variances(s.get_fields(("f",))["f"])
    s.run(steps)
    v1 = variances(s.get_fields(("f",))["f"])
    D = (1. / omega - 0.5) / 3.
    dev = [v1[i] - v0[i] - 2. * D * steps for i in (0, 1)]
    print("variance growth - 2 D t: x %+.3e, y %+.3e (model: +2.30e-5, -2.2e-6; bound 4.6e-5)" % (dev[0], dev[1]))
    assert max(abs(dev[0]), abs(dev[1])) <= 4.6e-5, dev


# ---- the drop-in classes ---------------------------------------------------------------------------------------------------------
def model_of_class(sim):
    g = sim.get_fields()
    m = ScalarModel(sim.nx, sim.ny, sim.omega, getattr(sim, "G", None) or 0., "open")
    m.set_fields(g["rho"], g["u"], g["v"])
    m.set_f(g["f"])
    return m


@pytest.mark.parametrize("which", ["Diffusion", "Advection_Diffusion", "Reaction_Diffusion", "Reaction_Advection_Diffusion"])
def test_classes_run_fused_and_phase_by_phase(lbhip, which):
    from LB_D2Q9.reaction_diffusion import diffusion as rd
    kw = dict(Lx=0.35, Ly=0.25, D=0.5, z=0.1, N=12, time_prefactor=0.6)
    if "Advection" in which:
        kw.update(vx=1.5, vy=-0.5, vc=2.)
    if "Reaction" in which:
        kw.update(g=40.)
    a, b = getattr(rd, which)(**kw), getattr(rd, which)(**kw)
    assert (a.nx, a.ny) == (38, 26) and a.X_dim.shape == (38, 26)
    rng = np.random.default_rng(5)
    perturb = 1. + 0.001 * rng.standard_normal((a.nx, a.ny, 9))
    a.init_pop(perturb); b.init_pop(perturb)
    m = model_of_class(a)
    if "Reaction" in which:
        assert a.sim.G == float(np.float32(a.G)) and a.G > 0
    steps = 12
    a.run(steps)
    for _ in range(steps):
        b.move(); b.move_bcs(); b.update_hydro(); b.update_feq(); b.collide_particles()
    m.run(steps)
    assert_close(a.get_fields(), m.get_fields(), steps, what=which + " run")
    assert_close(b.get_fields(), m.get_fields(), steps, what=which + " phases")
    ph = a.get_physical_fields()
    assert ph["u"] == pytest.approx(m.u * (a.delta_x / a.delta_t) * (a.L / a.T), rel=1e-6)
    assert a.rho.get().shape == (38, 26)


FIXTURE_CLASSES = {"ad_diffusion_37x23": "Diffusion", "ad_advection_37x23": "Advection_Diffusion",
                   "ad_fisher_37x23": "Reaction_Advection_Diffusion"}


def class_for_fixture(name, d):
    """An instance of the class the fixture's physics belongs to, on the fixture's 37 x 23 box (N = 7 cells per unit length, 5 x 3
    lengths) with the fixture's omega and G: time_prefactor and g are solved from the classes' own formulas, omega =
    1 / (1/2 + 3 lb_D), G = T g delta_t, and checked to round to the fixture's float32 values.  Its fields are then the fixture's."""
    from LB_D2Q9.reaction_diffusion import diffusion as rd
    omega, G = float(d["omega"]), float(d["G"])
    tp = (1. / omega - 0.5) / 3.                    # lb_D = time_prefactor (Diffusion; Advection with Pe = 1)
    kw = dict(Lx=0.55, Ly=0.35, z=0.1, N=7, time_prefactor=tp)
    which = FIXTURE_CLASSES[name]
    if which == "Diffusion":
        kw.update(D=1.)
    else:
        kw.update(D=0.25, vc=2.5, vx=1., vy=0.5)     # Pe = z vc / D = 1
    if which == "Reaction_Advection_Diffusion":
        T, delta_t = 0.1 / 2.5, tp / 49.
        kw.update(g=G / (T * delta_t))
    obj = getattr(rd, which)(**kw)
    assert (obj.nx, obj.ny) == (37, 23) and np.float32(obj.omega) == d["omega"]
    assert np.float32(getattr(obj, "G", None) or 0.) == d["G"]
    obj.sim.set_fields(np.zeros_like(d["u"]), d["u"], d["v"])
    obj.update_feq()
    obj.sim.set_f(d["f0"])
    return obj


@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_fixtures_through_the_classes(lbhip, name):
    d = golden(name)
    a, b = class_for_fixture(name, d), class_for_fixture(name, d)
    n = int(d["steps"][1])
    a.run(n)
    for _ in range(n):
        b.move(); b.move_bcs(); b.update_hydro(); b.update_feq(); b.collide_particles()
    want = dict(f=d["f_%d" % n], rho=d["rho_%d" % n], feq=d["feq_%d" % n])
    assert_close(a.get_fields(), want, n, what=name + " class run")
    assert_close(b.get_fields(), want, n, what=name + " class phases")
