"""Noisy strains on a shared nutrient on the GPU: lb_run_expansion (k_ex_step, the normals drawn in the kernel) and the un-fused stages
(k_ex_hydro, k_ex_collide, fed the fixtures' stored normals) against the fixtures recorded from the reference's C; what the product
computes twice, bitwise; the fused step against the stages where no fixture reaches; Nutrient_Set as an independent path to the same
physics; the noise counters; an external stream; refusals; the drop-in class.
Shapes: 3x3 and 5x4 (a row narrower than one lane-of-four / one lane and a tail), 8x4 (two whole lanes, one workgroup row), 21x13 and
37x23 (nx % 4 == 1, several workgroups in y, the last ragged), 261x9 (the smallest box with a second workgroup in x: one lane and a
tail of it).
"""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

import expansion_stream_scenarios as ES
from conftest import ROOT, golden
from scalar_model import contract_tol
from test_expansion_cpu import PHASES, RUN_FIXTURES, maxdiff

pytestmark = pytest.mark.gpu

F = np.float32
W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CUT = 0.01


def set_of(nx, ny, omegas, omega_n, Gs, Dgs, seed, f0, u, v, bc="open", cut=CUT, planar=None, edge_zero=False):
    from LB_D2Q9.expansion_set import Expansion_Set
    s = Expansion_Set(nx, ny, [F(o) for o in omegas], F(omega_n), [F(g) for g in Gs], bc=bc, zero_cutoff=cut, planar=planar)
    if Dgs is not None:
        s.set_noise([F(d) for d in Dgs], seed)
    s.set_fields(np.zeros((nx, ny, len(omegas) + 1), F), u, v)
    s.set_f(f0)
    if edge_zero:
        s.set_edge_state(np.zeros_like(s.get_edge_state()))
    return s


def set_of_fixture(d, planar=None):
    seeds = [int(x) for x in d["seeds"]]
    assert seeds == list(range(seeds[0], seeds[0] + len(seeds)))        # (Expansion_Set.set_noise: strain i draws under seed + i)
    return set_of(int(d["nx"]), int(d["ny"]), d["omega"], d["omega_nutrient"], d["G"], d["Dg"], seeds[0], d["f0"], d["u"], d["v"],
                  str(d["bc"]), float(d["zero_cutoff"]), planar, bool(int(d["edge_zero"])))


def smooth_case(nx, ny, n_strains, seed):
    """Strains in [0.15, 0.55], the nutrient in [0.7, 1], a non-uniform velocity <= 0.05: every density stays >= 2 CUT for a few steps."""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    f0 = np.zeros((nx, ny, n_strains + 1, 9), F, order="F")
    for i in range(n_strains + 1):
        bump = 0.5 + 0.5 * np.sin(2 * np.pi * (x / nx + 0.3 * i)) * np.cos(2 * np.pi * (y / ny - 0.2 * i))
        rho = 0.7 + 0.3 * bump if i == n_strains else 0.15 + 0.4 * bump
        f0[:, :, i, :] = (W[None, None, :] * rho[:, :, None] * (1. + 0.02 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(F)
    u = (0.05 * np.sin(2 * np.pi * y / ny) * np.cos(2 * np.pi * x / nx)).astype(F)
    v = (0.05 * np.cos(2 * np.pi * x / nx + 0.4)).astype(F)
    return f0, np.asfortranarray(u), np.asfortranarray(v)


OMEGAS, GS, DGS = (1.1, 0.9, 1.25), (0.01, 0.014, 0.012), (2.0e-3, 1.0e-3, 5.0e-4)


def smooth_set(nx, ny, n_strains, bc, seed=3, Dgs=DGS, noise_seed=40, **kw):
    f0, u, v = smooth_case(nx, ny, n_strains, seed)
    return set_of(nx, ny, OMEGAS[:n_strains], 1.3, GS[:n_strains], None if Dgs is None else Dgs[:n_strains], noise_seed, f0, u, v, bc, **kw)


def state(s):
    g = s.get_fields(("f", "rho"))
    return dict(f=g["f"], rho=g["rho"])


def hold(label, n, have, want):
    tol = contract_tol(n)
    for k in ("f", "rho"):
        d = maxdiff(have[k], want[k])
        print("%s: %s %.2e / %.1e" % (label, k, d, tol[k]))
        assert d <= tol[k], (label, k, d, tol[k])


def same_bits(a, b):
    return [k for k in b if not np.array_equal(a[k], b[k], equal_nan=True)]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_run_follows_reference_fixture(lbhip, name):
    """lb_run_expansion with the normals drawn in the kernel; every cell counts (the fixtures keep clear of the cutoff)."""
    d = golden(name)
    s = set_of_fixture(d)
    done = 0
    for n in [int(x) for x in d["steps"]]:
        s.run(n - done)
        done = n
        got = state(s)
        hold("%s after %d steps, fused / reference" % (name, n), n, got, dict(f=d["f_%d" % n], rho=d["rho_%d" % n]))
        assert np.array_equal(got["rho"] == 0, d["rho_%d" % n] == 0)
    assert [t for _, _, t in s.noise()] == [done] * len(d["omega"])
    s.close()


@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_stages_fed_the_stored_normals_follow_reference_fixture(lbhip, name):
    d = golden(name)
    s = set_of_fixture(d)
    done = 0
    for n in [int(x) for x in d["steps"]]:
        for t in range(done, n):
            for i, m in enumerate(s.strains):
                m.set_noise_field(d["z"][t][:, :, i])
            s.step_phases()
        done = n
        got = state(s)
        hold("%s after %d steps, stages / reference" % (name, n), n, got, dict(f=d["f_%d" % n], rho=d["rho_%d" % n]))
        assert np.array_equal(got["rho"] == 0, d["rho_%d" % n] == 0)
    assert [t for _, _, t in s.noise()] == [done] * len(d["omega"])
    s.close()


def test_stages_follow_phases_fixture_and_the_zeroed_links_are_zero(lbhip):
    d = golden(PHASES)
    tol = contract_tol(1)
    s = set_of_fixture(d)
    for i, m in enumerate(s.strains):
        m.set_noise_field(d["z"][0][:, :, i])
    s.move()
    s.move_bcs()
    assert np.array_equal(s.get_fields(("f",))["f"], d["f_move"], equal_nan=True)
    s.update_hydro()
    rho = s.get_fields(("rho",))["rho"]
    assert maxdiff(rho, d["rho_hydro"]) <= tol["rho"] and np.array_equal(rho == 0, d["rho_hydro"] == 0)
    s.update_feq()
    assert maxdiff(s.get_fields(("feq",))["feq"], d["feq_feq"]) <= tol["f"]
    s.collide_particles()
    f = s.get_fields(("f",))["f"]
    print("phases: f %.2e / %.1e" % (maxdiff(f, d["f_collide"]), tol["f"]))
    assert maxdiff(f, d["f_collide"]) <= tol["f"]
    assert np.array_equal(f == 0, d["zeroed"])
    s.close()
    # the fused step draws for itself: held in every cell whose recorded normals are the stream's own
    fused = set_of_fixture(d)
    fused.run(1)
    got, own = state(fused), d["z_is_stream"]
    assert own.sum() >= own.size - 2 * int(d["ny"])
    assert maxdiff(got["f"][own], d["f_collide"][own]) <= tol["f"] and maxdiff(got["rho"], d["rho_hydro"]) <= tol["rho"]
    assert np.array_equal(got["f"][own] == 0, d["zeroed"][own]) and np.array_equal(got["rho"] == 0, d["rho_hydro"] == 0)
    fused.close()


# ---- what the product computes twice: bitwise ------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc", ("open", "periodic"))
@pytest.mark.parametrize("shape", ((5, 4), (37, 23), (261, 9)), ids=lambda b: "%dx%d" % b)
def test_runs_repeat_split_and_restore_bitwise(lbhip, shape, bc, tmp_path):
    """run(7) against run(3); run(4), against the same seed again, against a checkpoint restored after 3 steps, and the planar
    layout against the default one."""
    from LB_D2Q9.expansion_set import Expansion_Set
    nx, ny = shape
    whole, again, split, planar = [smooth_set(nx, ny, 2, bc, planar=p) for p in (None, None, None, True)]
    whole.run(7)
    again.run(7)
    planar.run(7)
    split.run(3)
    split.save_checkpoint(tmp_path / "ex")
    restored = Expansion_Set.from_checkpoint(tmp_path / "ex")
    assert restored.noise() == split.noise() and restored.noise()[0][2] == 3 and restored.zero_cutoff == split.zero_cutoff
    split.run(4, wait=False)
    restored.run(4)
    want = state(whole)
    for other in (again, split, restored, planar):
        assert not same_bits(state(other), want)
        assert other.noise() == whole.noise()
    other_seed = smooth_set(nx, ny, 2, bc, noise_seed=41)
    other_seed.run(7)
    assert same_bits(state(other_seed), want) == ["f", "rho"]
    for s in (whole, again, split, planar, restored, other_seed):
        s.close()


@pytest.mark.parametrize("bc", ("open", "periodic"))
def test_a_strain_without_noise_draws_nothing(lbhip, bc):
    """Dg = 0 on a strain against never having called set_noise on it, bitwise; its noise counter does not move."""
    from LB_D2Q9.expansion_set import Expansion_Set
    nx, ny = 37, 23
    f0, u, v = smooth_case(nx, ny, 2, 5)
    sets = []
    for call_it in (True, False):
        s = Expansion_Set(nx, ny, OMEGAS[:2], 1.3, GS[:2], bc=bc, zero_cutoff=CUT)
        s.strains[0].set_noise(DGS[0], 40)
        if call_it:
            s.strains[1].set_noise(0., 41)
        s.set_fields(np.zeros((nx, ny, 3), F), u, v)
        s.set_f(f0)
        s.run(5)
        sets.append(s)
    assert not same_bits(state(sets[0]), state(sets[1]))
    assert [t for _, _, t in sets[0].noise()] == [5, 0] == [t for _, _, t in sets[1].noise()]
    quiet = smooth_set(nx, ny, 2, bc, seed=5, Dgs=None)
    quiet.run(5)
    assert same_bits(state(quiet), state(sets[0])) == ["f", "rho"] and [t for _, _, t in quiet.noise()] == [0, 0]
    for s in sets + [quiet]:
        s.close()


def test_noise_counters_and_fill(lbhip):
    """Each strain's t after n steps by run and by the stages; noise_fill(t) is a pure function of (seed, t): a run does not change it."""
    s = smooth_set(21, 13, 3, "open")
    before = [m.noise_fill(4) for m in s.strains]
    assert not np.array_equal(before[0], before[1])
    s.run(4)
    assert [(F(dg), seed, t) for dg, seed, t in s.noise()] == [(F(DGS[i]), 40 + i, 4) for i in range(3)]
    s.step_phases()
    assert [t for _, _, t in s.noise()] == [5, 5, 5]
    for m, z in zip(s.strains, before):
        assert np.array_equal(m.noise_fill(4), z)
    s.close()


# ---- fused against stages where no fixture reaches ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_strains", (1, 2, 3))
@pytest.mark.parametrize("bc", ("open", "periodic"))
@pytest.mark.parametrize("shape", ((8, 4), (261, 9)), ids=lambda b: "%dx%d" % b)
def test_fused_step_follows_the_stages(lbhip, shape, bc, n_strains):
    """Four steps, both drawing from the stream (k_ex_step a lane's four normals, k_ex_collide each cell's own): the same normals bit
    for bit, the relaxation rounded differently -- the contract's tolerance.  Every density stays >= 2 CUT: no threshold is near."""
    nx, ny = shape
    fused, staged = (smooth_set(nx, ny, n_strains, bc) for _ in range(2))
    fused.run(4)
    for _ in range(4):
        staged.step_phases()
    got, want = state(fused), state(staged)
    assert float(want["rho"].min()) >= 2 * CUT and float(got["rho"].min()) >= 2 * CUT
    hold("%dx%d %s NP=%d fused / stages" % (nx, ny, bc, n_strains), 4, got, want)
    assert fused.noise() == staged.noise()
    fused.close(), staged.close()


def test_one_quiet_strain_without_cutoff_is_the_nutrient_set(lbhip):
    """One strain, Dg = 0, zero_cutoff = 0, periodic, u = v = 0 against Nutrient_Set with scale = 0 and the same G: k_sn_step and the
    spectral solve in front of it are an independent path to the same physics."""
    from LB_D2Q9.nutrient_set import Nutrient_Set
    nx, ny, n = 30, 18, 10
    f0, _, _ = smooth_case(nx, ny, 1, 7)
    zero = np.zeros((nx, ny), F, order="F")
    ex = set_of(nx, ny, OMEGAS[:1], 1.3, GS[:1], None, 0, f0, zero, zero, "periodic", cut=0.)
    ns = Nutrient_Set(nx, ny, F(OMEGAS[0]), F(1.3), lam=1., dx=0.1)
    ns.set_params(G=GS[0], scale=0., clumpy=False)
    ns.set_f(f0)
    ex.run(n), ns.run(n)
    hold("30x18 quiet strain / Nutrient_Set", n, state(ex), ns.get_fields(("f", "rho")))
    ex.close(), ns.close()


# ---- an external stream --------------------------------------------------------------------------------------------------------------
def test_external_stream_twin(lbhip, tmp_path):
    """tests/expansion_stream_scenarios.py in a fresh python (torch first: one HIP runtime): the chain behind a delay on a caller's
    stream equals the waiting twin bit for bit, and the delay outlasted four times the enqueue."""
    script = tmp_path / "expansion_child.py"
    script.write_text(ES.PRELUDE + ES.EXPANSION + ES.EPILOGUE)
    p = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-lb_amd")],
                       capture_output=True, text=True, timeout=300)
    print("\n".join(l for l in p.stdout.splitlines() if l.startswith(("RATIO", "SCENARIO"))))
    assert p.returncode == 0 and "EXPANSION_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    assert "SCENARIO expansion_set_with_the_nutrient_on_an_external_stream OK" in p.stdout


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_reason_and_the_state(lbhip):
    from LB_D2Q9 import _native
    from LB_D2Q9.noisy_simulation import NoisySimulation
    from LB_D2Q9.simulation import Simulation
    L = lbhip
    nx, ny = 21, 13
    s = smooth_set(nx, ny, 2, "open")
    s.run(2)
    before = state(s)
    a, b, n = (m._h for m in s.members)
    extra = [NoisySimulation(nx, ny, 1.0, bc="open"), NoisySimulation(nx, ny, 1.0, bc="open")]
    periodic = Simulation(nx, ny, 1.0, bc="periodic", semantics="diffusion")
    planar = Simulation(nx, ny, 1.0, bc="open", semantics="diffusion", planar=True)
    bigger = Simulation(nx + 1, ny, 1.0, bc="open", semantics="diffusion")
    field = Simulation(nx, ny, 1.0, bc="periodic", semantics="multifield")
    arr = lambda *hs: (ct.c_void_p * len(hs))(*hs)
    P = lambda cut=CUT: ct.byref(_native.ExpansionParams(cut))
    ARG, STATE = -1, -3         # LB_ERR_ARG, LB_ERR_STATE

    def refused(rc, code, *words):
        msg = L.lb_last_error().decode()
        assert rc == code, (rc, msg)
        for w in words:
            assert w.lower() in msg.lower(), (w, msg)

    refused(L.lb_run_expansion(arr(a), 1, P(), 1), ARG, "2..4", "count")
    refused(L.lb_run_expansion(arr(a, b, extra[0]._h, extra[1]._h, n), 5, P(), 1), ARG, "2..4")
    refused(L.lb_run_expansion(arr(a, a, n), 3, P(), 1), ARG, "twice")
    refused(L.lb_run_expansion(arr(a, field._h), 2, P(), 1), ARG, "LB_SEM_DIFFUSION")
    refused(L.lb_run_expansion(arr(a, periodic._h), 2, P(), 1), ARG, "family")
    refused(L.lb_run_expansion(arr(a, bigger._h), 2, P(), 1), ARG, "geometry")
    refused(L.lb_run_expansion(arr(a, planar._h), 2, P(), 1), ARG, "layout")
    for bad in (float("nan"), float("inf"), float("-inf")):
        refused(L.lb_run_expansion(arr(a, b, n), 3, P(bad), 1), ARG, "zero_cutoff", "finite")
    refused(L.lb_run_expansion(arr(a, b, n), 3, P(), -1), ARG, "negative")
    extra[0].set_noise(1.0e-3, 99)
    refused(L.lb_run_expansion(arr(a, b, extra[0]._h), 3, P(), 1), STATE, "nutrient", "lb_set_noise")      # a noisy handle in the nutrient's place
    extra[0].set_noise(0., 99)
    s.nutrient.set_reaction(0.01)
    refused(L.lb_run_expansion(arr(a, b, n), 3, P(), 1), ARG, "nutrient", "growth rate")
    s.nutrient.set_reaction(0.)
    _, seed_a, t_a = s.strains[0].noise()
    dg_b, seed_b, t_b = s.strains[1].noise()
    s.strains[1].set_noise(dg_b, seed_a)
    refused(L.lb_run_expansion(arr(a, b, n), 3, P(), 1), ARG, "same seed")
    refused(L.lb_collide_expansion(arr(a, b, n), 3, P()), ARG, "same seed")
    s.strains[1].set_noise(dg_b, seed_b)
    check = _native.check
    check(L.lb_set_noise_counter(b, t_b))
    refused(L.lb_collide_expansion(arr(a, b, n), 3, P()), STATE, "lb_update_feq")
    s.strains[0].set_noise_field(np.zeros((nx, ny), F))
    refused(L.lb_run_expansion(arr(a, b, n), 3, P(), 1), STATE, "noise field")
    s.strains[0].set_noise_field(None)
    refused(L.lb_update_hydro_expansion(arr(a, a), 2, P()), ARG, "twice")
    refused(L.lb_update_hydro_expansion(arr(a, b, n), 3, None), ARG, "null parameters")
    # no kernel has run: the state is what it was, and the set still runs
    assert not same_bits(state(s), before) and [t for _, _, t in s.noise()] == [2, 2]
    s.run(2)
    assert all(c["n_nonfinite"] == 0 for c in s.check())
    for x in [s, periodic, planar, bigger, field] + extra:
        x.close()


# ---- the drop-in class -----------------------------------------------------------------------------------------------------------
def test_dropin_class_conserves_the_mass_budget_while_no_floor_fires(lbhip):
    """Periodic, the whole box inoculated (ny = N + 2 <= 2 N): sum rho_strains + rho_nutrient over the box stays over 20 steps, up to
    float32 rounding -- per link and step some 16 roundings of relative size 2^-24, accumulated linearly at worst -- while neither the
    cutoff nor the floor fires; the test asserts that neither did, after every step."""
    from LB_D2Q9.advecting_range_expansion.stochastic_nutrients import Expansion
    sim = Expansion(Lx=4., Ly=2., vx=0.2, vy=0.1, vc=0.5, mu_list=[1., 1.2], D_list=[1., 0.8], Nb=50., N=8, bc="periodic", seed=11)
    assert (int(sim.nx), int(sim.ny)) == (18, 10) and int(sim.num_populations) == 2
    g = sim.get_fields()
    assert g["rho"].shape == (18, 10, 3) and g["f"].shape == g["feq"].shape == (18, 10, 3, 9) and g["u"].shape == g["v"].shape == (18, 10)
    assert all(g[k].flags.f_contiguous and g[k].dtype == F for k in ("rho", "f", "feq", "u", "v"))
    assert np.all(g["rho"][:, :, :2] == F(0.5)) and np.all(g["rho"][:, :, 2] == 1.) and np.array_equal(g["f"], g["feq"])
    assert np.all(g["u"] == g["u"][0, 0]) and float(g["u"][0, 0]) > 0
    budget = lambda: float(np.asarray(sim.f).astype(np.float64).sum())
    start = budget()
    for step in range(20):
        sim.run(1)
        f, rho = np.asarray(sim.f), np.asarray(sim.rho)
        assert (f > 0).all() and (rho >= float(sim.zero_cutoff)).all(), step
    drift, bound = abs(budget() - start), 20 * 16 * 2. ** -24 * start
    print("mass budget: drift %.3e / %.3e of %.1f" % (drift, bound, start))
    assert drift <= bound
    assert [t for _, _, t in sim.noise()] == [20, 20] and float(np.std(np.asarray(sim.rho)[:, :, 0])) > 0
    sim.sim.close()


def test_dropin_class_starts_as_the_reference_does(lbhip):
    """The open box: the inoculum in rows y < 2 N with real zeros ahead, the nutrient everywhere, the edge state zero; the phase methods
    make the step run(1) makes, within the contract; the front moves into the nutrient."""
    from LB_D2Q9.advecting_range_expansion.stochastic_nutrients import Expansion
    kw = dict(Lx=4., Ly=6., mu_list=[1., 1.], D_list=[1., 1.], Nb=100., N=4, seed=3)
    sim, twin = Expansion(**kw), Expansion(**kw)
    assert (int(sim.nx), int(sim.ny)) == (10, 14)
    rho = np.asarray(sim.rho)
    assert np.all(rho[:, :8, :2] == F(0.5)) and np.all(rho[:, 8:, :2] == 0) and np.all(rho[:, :, 2] == 1.)
    assert not sim.sim.get_edge_state().any()
    sim.run(1)
    twin.move(), twin.move_bcs(), twin.update_hydro(), twin.update_feq(), twin.collide_particles()
    got, want = dict(f=np.asarray(sim.f), rho=np.asarray(sim.rho)), dict(f=np.asarray(twin.f), rho=np.asarray(twin.rho))
    hold("drop-in class, run(1) / the phase methods", 1, got, want)
    assert np.array_equal(got["rho"] == 0, want["rho"] == 0) and (got["rho"][:, 10:, :2] == 0).all()
    sim.run(30)
    assert (np.asarray(sim.rho)[:, :, :2] > 0).sum() > (got["rho"][:, :, :2] > 0).sum()
    sim.sim.close(), twin.sim.close()
