"""The noisy collision of a scalar lattice on the GPU (lb_set_noise ...; csrc/philox.h): the in-kernel
normals against the float64 model (tests/noise_model.py), k_ad_tile4 against k_ad_step bit for bit with noise on, one stream
however a run is split or checkpointed, the fused run against the un-fused phases and against the fixtures recorded from the
reference's C (tests/golden/nf_*.npz), NaN and clamp cells, refusals, the drop-in class."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from LB_D2Q9.variants import K_STEP, STEP4_NO_AHEAD, TILES
from noise_model import normals64
from scalar_model import contract_tol
from test_gpu_scalar import TILE_BOXES, random_case

pytestmark = pytest.mark.gpu

LB_ERR_ARG, LB_ERR_STATE = -1, -3

# max |z_gpu - z_model64| measured on a 1024 x 1024 fill (seed 1, t = 0): float32 rounding of ln, sqrt, sin / cos
# and two products at |z| up to 5.  The same ISA gives the same bits on every machine; the factor 2 covers other seeds and counters.
FILL_ERR_1024 = 5.986566e-07      # at z = -4.36: 2.2e-7 relative, under two units of float32's last place
FILL_BOUND = 2. * FILL_ERR_1024


def maxdiff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sim_of(d, bc="open", noise=True):
    from LB_D2Q9.noisy_simulation import NoisySimulation
    s = NoisySimulation(int(d["nx"]), int(d["ny"]), float(d["omega"]), bc=bc)
    s.set_reaction(float(d["G"]))
    if noise:
        s.set_noise(float(d["Dg"]), int(d["seed"]))
    s.set_fields(np.zeros_like(d["u"]), d["u"], d["v"])
    s.set_f(d["f0"])
    return s


def case(nx, ny, seed, omega=1.35, G=1e-4, Dg=1e-4, noise_seed=5):
    """random_case's blob (test_gpu_scalar.py) scaled to rho <= 0.76, so that a run of a hundred noisy steps stays inside (0, 1)"""
    c = random_case(nx, ny, seed)
    c["f0"] = (c["f0"] * np.float32(0.8)).astype(np.float32)
    c.update(omega=np.float32(omega), G=np.float32(G), Dg=np.float32(Dg), seed=noise_seed)
    return c


def assert_same_bits(a, b, what):
    ga, gb = a.get_fields(("f", "rho")), b.get_fields(("f", "rho"))
    for k in ("f", "rho"):
        assert np.array_equal(bits(ga[k]), bits(gb[k])), "%s: %s differs, max %.3e" % (what, k, maxdiff(ga[k], gb[k]))
    return ga


def assert_close(got, want, n, keys=("f", "rho", "feq"), what=""):
    tol = contract_tol(n)
    tol["feq"] = tol["f"]
    meas = {k: maxdiff(got[k], want[k]) for k in keys}
    print("%s after %d steps, measured / bound: %s" % (what, n, ", ".join("%s %.2e / %.1e" % (k, meas[k], tol[k]) for k in keys)))
    for k in keys:
        assert meas[k] <= tol[k], "%s %s: %.3e > %.1e" % (what, k, meas[k], tol[k])


# ---- 1. lb_noise_fill against the float64 model ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,ny", [(5, 3), (37, 23), (130, 9)])
@pytest.mark.parametrize("t", [0, 12345, (1 << 32) + 7])
def test_noise_fill_follows_the_float64_model(lbhip, nx, ny, t):
    from LB_D2Q9.noisy_simulation import NoisySimulation
    s = NoisySimulation(nx, ny, 1.0, bc="periodic")
    seed = 0x9e3779b97f4a7c15
    s.set_noise(1e-3, seed)
    z = s.noise_fill(t)
    err = maxdiff(z, normals64(nx, ny, seed, t))
    print("%dx%d t=%d: max |z_gpu - z_model64| = %.3e (bound %.3e)" % (nx, ny, t, err, FILL_BOUND))
    assert z.shape == (nx, ny) and err <= FILL_BOUND
    assert s.noise() == (float(np.float32(1e-3)), seed, 0)         # a fill draws nothing: the counter stays
    if t:
        assert not np.array_equal(z, s.noise_fill(t - 1))


def test_noise_fill_1024_error_and_moments(lbhip):
    from LB_D2Q9.noisy_simulation import NoisySimulation
    n = 1024
    s = NoisySimulation(n, n, 1.0, bc="periodic")
    s.set_noise(1e-3, 1)
    z = s.noise_fill(0).astype(np.float64)
    err = maxdiff(z, normals64(n, n, 1, 0))
    print("1024^2 fill: max |z_gpu - z_model64| = %.4e, mean %.3e, variance - 1 = %.3e" % (err, z.mean(), z.var() - 1.))
    assert err <= FILL_BOUND
    # five sigma of the mean and of the variance of n^2 independent standard normals
    assert abs(z.mean()) < 5. / np.sqrt(n * n) and abs(z.var() - 1.) < 5. * np.sqrt(2. / (n * n))


# ---- 2. k_ad_tile4 = four k_ad_step, bitwise, with noise on -----------------------------------------------------------------------
@pytest.mark.parametrize("bc", ["periodic", "open"])
@pytest.mark.parametrize("shape", [0, 1, 2, 3])
@pytest.mark.parametrize("plan", ["plane", "cell"])
def test_noisy_tile_kernel_equals_step_kernel_bitwise(lbhip, bc, shape, plan):
    """Both noise plans of k_ad_tile4: the noise plane in LDS (the default; on the boxes whose width is no multiple of 4 the periodic
    seam takes its per-cell path) and, behind the A/B switch STEP4_NO_AHEAD, a draw per cell."""
    for nx, ny in TILE_BOXES:
        c = case(nx, ny, seed=nx * 100 + ny)
        a, b = sim_of(c, bc), sim_of(c, bc)
        a.set_variant(K_STEP)
        b.set_variant(TILES | (shape << 2) | (STEP4_NO_AHEAD if plan == "cell" else 0))
        assert a.plan_launches(13) == [1] * 13 and b.plan_launches(13) == [4, 4, 4, 1]
        for n in range(1, 14):
            a.run(n); b.run(n)
            g = assert_same_bits(a, b, "%s %dx%d shape %d %s, run(%d)" % (bc, nx, ny, shape, plan, n))
        assert np.isfinite(g["f"]).all() and a.noise()[2] == b.noise()[2] == 91
        plain = sim_of(c, bc, noise=False)
        plain.run(1)
        a2 = sim_of(c, bc)
        a2.run(1)
        assert not np.array_equal(plain.get_fields(("f",))["f"], a2.get_fields(("f",))["f"])       # the noise is on


# ---- 3. one stream ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ["periodic", "open"])
def test_one_stream_across_splits_handles_and_checkpoints(lbhip, bc, tmp_path):
    from LB_D2Q9.noisy_simulation import NoisySimulation
    from LB_D2Q9.simulation import Simulation
    c = case(130, 50, seed=6)
    a, b, other = sim_of(c, bc), sim_of(c, bc), sim_of(dict(c, seed=6), bc)
    a.run(5)
    b.run(2); b.run(3)
    assert_same_bits(a, b, "run(5) vs run(2); run(3)")
    other.run(5)
    assert not np.array_equal(a.get_fields(("f",))["f"], other.get_fields(("f",))["f"])          # another seed, other bits
    assert a.noise() == (float(c["Dg"]), 5, 5)
    a.save_checkpoint(tmp_path / "ck")
    r, plain = NoisySimulation.from_checkpoint(tmp_path / "ck"), Simulation.from_checkpoint(tmp_path / "ck")
    assert r.noise() == a.noise()
    a.run(3); r.run(3); plain.run(3)
    assert_same_bits(a, r, "run(3) after a checkpoint")
    assert_same_bits(a, plain, "run(3) after a checkpoint, restored as a Simulation")
    assert r.noise()[2] == 8


# ---- 4. fused = un-fused ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ["periodic", "open"])
def test_fused_run_equals_phases_fed_with_the_stream(lbhip, bc):
    c = case(63, 17, seed=9, Dg=1e-3)
    a, b = sim_of(c, bc), sim_of(c, bc)
    a.run(6)
    for t in range(6):
        b.set_noise_field(b.noise_fill(t))
        b.move(); b.move_bcs(); b.update_hydro(); b.update_feq(); b.collide_particles()
    assert_close(a.get_fields(), b.get_fields(), 6, keys=("f", "rho"), what="%s fused vs phases" % bc)
    assert a.noise()[2] == b.noise()[2] == 6
    # without a field the un-fused collision draws from the stream itself
    b.set_noise_field(None)
    a.run(1)
    b.move(); b.move_bcs(); b.update_hydro(); b.update_feq(); b.collide_particles()
    assert_close(a.get_fields(), b.get_fields(), 7, keys=("f", "rho"), what="%s fused vs phases on the stream" % bc)


# ---- 5. the reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ["periodic", "open"])
def test_phases_with_the_fixtures_normals_follow_the_reference(lbhip, bc):
    d = golden("nf_run_%s_37x23" % bc)
    s = sim_of(d, bc)
    done = 0
    for n in [int(k) for k in d["steps"]]:
        for t in range(done, n):
            s.set_noise_field(d["z"][t])
            s.move(); s.move_bcs(); s.update_hydro(); s.update_feq(); s.collide_particles()
        done = n
        assert_close(s.get_fields(), dict(f=d["f_%d" % n], rho=d["rho_%d" % n], feq=d["feq_%d" % n]), n, what="nf %s phases" % bc)


@pytest.mark.parametrize("bc", ["periodic", "open"])
@pytest.mark.parametrize("variant", [K_STEP, TILES])
def test_fused_run_follows_the_reference(lbhip, bc, variant):
    """The in-kernel normals differ from the fixture's float32 ones by the error of test 1, which enters f as w_k sqrt(Dg / 4) dz."""
    d = golden("nf_run_%s_37x23" % bc)
    s = sim_of(d, bc)
    s.set_variant(variant)
    done = 0
    for n in [int(k) for k in d["steps"]]:
        s.run(n - done)
        done = n
        assert_close(s.get_fields(), dict(f=d["f_%d" % n], rho=d["rho_%d" % n], feq=d["feq_%d" % n]), n, what="nf %s fused" % bc)


# ---- 6. NaN and clamp ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_nan_and_clamp_cells_of_the_one_step_record(lbhip, fused):
    d = golden("nf_phases_21x13")
    s = sim_of(d)
    if fused:
        s.run(1)
    else:
        s.set_noise_field(d["z"])
        s.move(); s.move_bcs(); s.update_hydro(); s.update_feq(); s.collide_particles()
    g = s.get_fields(("f", "rho"))
    nan_cells, clamped, want = d["nan_cells"], d["clamped"], d["f_collide"]
    assert np.array_equal(np.isnan(g["f"]), np.repeat(nan_cells[:, :, None], 9, axis=2))         # all nine links, nowhere else
    assert np.array_equal((g["f"] == 0.) & ~np.isnan(g["f"]), clamped)                            # exactly 0
    ok = ~np.isnan(want)
    tol = contract_tol(1)
    assert maxdiff(g["f"][ok], want[ok]) <= tol["f"] and maxdiff(g["rho"], d["rho_hydro"]) <= tol["rho"]
    assert s.check()["n_nonfinite"] == int(nan_cells.sum())


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(lbhip):
    from LB_D2Q9.simulation import Simulation
    others = [Simulation(16, 12, 0.5, bc="dirichlet", semantics="poisson"), Simulation(16, 12, 1.0, bc="periodic", semantics="multifield"),
              Simulation(16, 12, 1.0, bc="periodic")]
    buf = np.zeros((16, 12), np.float32, order="F")
    dg, seed, t = ct.c_float(), ct.c_uint64(), ct.c_uint64()
    for s in others:
        L, h = s._lib, s._h
        for rc in (L.lb_set_noise(h, 1e-3, 1), L.lb_get_noise(h, ct.byref(dg), ct.byref(seed), ct.byref(t)), L.lb_set_noise_counter(h, 3),
                   L.lb_noise_fill(h, 0, buf.ctypes.data, 0), L.lb_set_noise_field(h, buf.ctypes.data, 0)):
            assert rc == LB_ERR_STATE, (s.semantics if hasattr(s, "semantics") else s, rc, L.lb_last_error())
    from LB_D2Q9.noisy_simulation import NoisySimulation
    s = NoisySimulation(16, 12, 1.0, bc="periodic")
    L, h = s._lib, s._h
    assert L.lb_set_noise(h, -1e-3, 1) == LB_ERR_ARG and L.lb_set_noise(h, float("nan"), 1) == LB_ERR_ARG
    assert L.lb_set_noise(h, float("inf"), 1) == LB_ERR_ARG and s.noise() == (0., 0, 0)
    assert L.lb_noise_fill(h, 0, None, 0) == LB_ERR_ARG
    s.set_noise(1e-3, 4)
    s.set_noise_field(buf)
    assert L.lb_run(h, 1) == LB_ERR_STATE and b"noise field" in L.lb_last_error()
    s.set_noise_field(None)
    assert L.lb_run(h, 1) == 0 and s.noise() == (float(np.float32(1e-3)), 4, 1)
    s.set_noise(1e-3, 4)
    assert s.noise()[2] == 0                                        # lb_set_noise resets the counter


# ---- 8. Dg = 0 after lb_set_noise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ["periodic", "open"])
def test_noise_switched_off_is_the_plain_handle_bitwise(lbhip, bc):
    c = case(130, 50, seed=3, G=0.01)
    a, b = sim_of(c, bc, noise=False), sim_of(c, bc)
    b.run(3)
    b.set_noise(0., 99)
    b.set_f(c["f0"])
    a.run(9); b.run(9)
    assert_same_bits(a, b, "%s Dg = 0" % bc)
    assert b.noise() == (0., 99, 0)                                 # the plain cell counts nothing
    assert "noise" not in b.checkpoint_arrays()


def test_screened_wave_steps_its_lattice_with_the_noise(lbhip):
    """lb_run_screened steps the scalar lattice through scalar_step: one noisy collision, one count of t, per step."""
    from LB_D2Q9.reaction_diffusion.screened_poisson_waves import Screened_Fisher_Wave
    kw = dict(Lx=3.2, Ly=2.4, vc=0.5, lam=1., R0=0.5, N=10)
    plain, a, b = Screened_Fisher_Wave(**kw), Screened_Fisher_Wave(**kw), Screened_Fisher_Wave(**kw)
    for w in (a, b):
        w.sim._set_noise(1e-6, 11)
    for w in (plain, a, b):
        w.run(3)
    fa, fb, fp = (w.sim.get_fields(("f",))["f"] for w in (a, b, plain))
    assert a.sim._noise() == (float(np.float32(1e-6)), 11, 3) and plain.sim._noise()[2] == 0
    assert np.array_equal(bits(fa), bits(fb)) and not np.array_equal(fa, fp)
    assert maxdiff(fa[np.isfinite(fa)], fp[np.isfinite(fa)]) < 1e-2         # the same wave, roughened


def test_screened_wave_refuses_a_noise_field_before_it_touches_anything(lbhip):
    from LB_D2Q9.reaction_diffusion.screened_poisson_waves import Screened_Fisher_Wave
    w = Screened_Fisher_Wave(Lx=3.2, Ly=2.4, vc=0.5, lam=1., R0=0.5, N=10)
    w.sim._set_noise(1e-6, 11)
    before = w.sim.get_fields(("f", "rho", "u", "v"))
    w.sim._set_noise_field(np.zeros((w.nx, w.ny), np.float32))
    rc = w._lib.lb_run_screened(w.poisson_solver._h, w.sim._h, float(w.velocity_scale), 2)
    assert rc == LB_ERR_STATE and b"noise field" in w._lib.lb_last_error()
    after = w.sim.get_fields(("f", "rho", "u", "v"))
    for k in before:
        assert np.array_equal(bits(before[k]), bits(after[k])), k            # nothing written, the counter where it was
    assert w.sim._noise()[2] == 0
    w.sim._set_noise_field(None)
    w.run(2)                                                                    # and the solver was never left borrowed
    assert w.sim._noise()[2] == 2 and np.isfinite(w.sim.get_fields(("f",))["f"]).all()


def test_nutrient_set_refuses_a_noisy_member(lbhip):
    """The set's own kernels (k_sn_step) draw no noise: a member with the noisy collision on is refused, not silently run plain."""
    from LB_D2Q9.nutrient_set import Nutrient_Set
    s = Nutrient_Set(32, 24, 1.0, 1.2)
    s.members[0]._set_noise(1e-4, 3)
    rc = s._lib.lb_run_nutrient(s.solver._h, s._handles, 2, s._params(), 1)
    assert rc == LB_ERR_STATE and b"noisy collision" in s._lib.lb_last_error()
    s.members[0]._set_noise(0., 3)
    assert s._lib.lb_run_nutrient(s.solver._h, s._handles, 2, s._params(), 1) == 0
    s.sync()
    s.close()


def test_automatic_choice_of_a_noisy_handle_follows_its_own_size_rule(lbhip):
    """plan.cpp's rule (profiles/scalar_bench.txt, the noise column): with noise the tiles stay faster than k_ad_step at every size in a
    periodic box, in the OPEN family only below 1024^2."""
    from LB_D2Q9.noisy_simulation import NoisySimulation
    for bc, n, tiles in (("open", 300, True), ("open", 1100, False), ("periodic", 1100, True), ("periodic", 100, False)):
        s = NoisySimulation(n, n, 1.0, bc=bc)
        plain = s.plan_launches(9)
        assert plain == ([4, 4, 1] if n >= 256 else [1] * 9)
        s.set_noise(1e-4, 1)
        assert s.plan_launches(9) == ([4, 4, 1] if tiles else [1] * 9), (bc, n)
        assert s.hot_kernel().startswith("k_ad_tile4" if tiles else "k_ad_step") and s.steps_per_launch() == (4 if tiles else 1)
        s.set_variant(TILES)
        assert s.plan_launches(9) == [4, 4, 1]
        s.set_variant(-1)
        s.set_noise(0., 1)
        assert s.plan_launches(9) == plain
    # and whichever it picks, the bits are k_ad_step's
    c = case(300, 300, seed=4)
    a, b = sim_of(c, "open"), sim_of(c, "open")
    a.set_variant(K_STEP)
    assert b.plan_launches(9) == [4, 4, 1]
    a.run(9); b.run(9)
    assert_same_bits(a, b, "automatic 300^2 open, noisy")


# ---- 9. the class ----------------------------------------------------------------------------------------------------------------------
def test_class_runs_and_is_reproducible(lbhip):
    from LB_D2Q9.reaction_diffusion.noisy_fisher_wave import Noisy_Advected_Fisher_Wave
    kw = dict(N=10, z=0.1, D=1., g=100., Nc=1000., vx=0.5, vy=0., vc=1., time_prefactor=1.)
    a, b, c = Noisy_Advected_Fisher_Wave(seed=7, **kw), Noisy_Advected_Fisher_Wave(seed=7, **kw), Noisy_Advected_Fisher_Wave(seed=8, **kw)
    assert (a.nx, a.ny) == (102, 102) and a.omega == pytest.approx(1. / 3.5) and a.lb_Gd == pytest.approx(1e-2)
    m0 = float(a.get_fields()["rho"].astype(np.float64).sum())
    for w in (a, b, c):
        w.run(20)
    ga, gb, gc = a.get_fields(), b.get_fields(), c.get_fields()
    assert set(ga) == {"f", "feq", "u", "v", "rho"}
    assert ga["f"].shape == ga["feq"].shape == (102, 102, 9) and ga["rho"].shape == ga["u"].shape == ga["v"].shape == (102, 102)
    assert np.isfinite(ga["f"]).all()
    assert float(ga["f"].astype(np.float64).sum()) > m0             # G > 0: the total mass grows
    for k in ("f", "rho"):
        assert np.array_equal(bits(ga[k]), bits(gb[k])), k
    assert not np.array_equal(ga["f"], gc["f"])
    assert a.sim.noise()[2] == 20
    with pytest.raises(ZeroDivisionError):                          # the reference's default vc = 0
        Noisy_Advected_Fisher_Wave(N=10)
