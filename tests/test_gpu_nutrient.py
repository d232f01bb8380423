"""A population and its nutrient under a spectral velocity on the GPU: lb_run_nutrient (k_ad_moments, the three launches of the solve,
k_sn_step) and the un-fused stages against the fixtures recorded from the reference's C and against the numpy model
(tests/nutrient_model.py); what the product computes twice, bitwise; the stencil's locality; an external stream; refusals; the
drop-in classes.
Shapes: 3x3 and 5x4 (a row narrower than one lane-of-four group plus its tail; every stencil neighbour wraps), 30x18 (nx % 4 == 2,
mixed radices, five workgroups of SN_ROWS = 4 rows, the last one ragged), 270x12 (k_sn_step's tile is k_ry_step's 256 cells: the row
crosses it, so the LDS halo columns of the first tile come from the second tile and from the wrap, those of the second from the first
and from the wrap; 12 rows are three workgroups, so every halo row is another workgroup's or the wrap), 20x12 for the phases; 1000x12
and 12x1000 (the solver's batched passes, which begin at 512 points an axis: column blocks of cols = 3 with the last one a column
short, row blocks of rows = 3 with the last one a row short -- tests/test_spectral_cpu.py asks sp_plan for both; four tiles a row).
Bounds: the project's parity contract (contract_tol) in f, feq, rho, u, v and nutrient_bounds in psi and F, as tests/test_nutrient_cpu.py
states them."""
import ctypes as ct
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import nutrient_stream_scenarios as NS
from conftest import ROOT, golden
from nutrient_model import PARAMS, NutrientModel
from scalar_model import contract_tol
from spectral_model import noisy_droplet
from test_nutrient_cpu import PHASES, RUN_FIXTURES, STEPS, compare, maxdiff, recorded

pytestmark = pytest.mark.gpu

F = np.float32
# model / fixture name -> Nutrient_Set.get_fields key
KEYS = dict(f="f", feq="feq", rho="rho", u="u", v="v", psi="psi", Fx="pseudo_force_x", Fy="pseudo_force_y")
BOXES = ((270, 12), (1000, 12), (12, 1000))                           # test_row_across_the_tile_boundary_follows_the_model's
CASE = dict(G=0.01, scale=-0.05, rho_o=1., G_chen=-1., lam=1.)        # the issue's case at N = 10, vc = 0.5


def all_keys(clumpy):
    return ("f", "rho", "u", "v") + (("psi", "Fx", "Fy") if clumpy else ())


def got_of(s, which):
    g = s.get_fields(tuple(KEYS[k] for k in which))
    return {k: g[KEYS[k]] for k in which}


def set_of(nx, ny, omegas, params, clumpy, f0, planar=None):
    from LB_D2Q9.nutrient_set import Nutrient_Set
    s = Nutrient_Set(nx, ny, F(omegas[0]), F(omegas[1]), lam=float(params["lam"]), dx=0.1, planar=planar)
    s.set_params(clumpy=bool(clumpy), **{k: params[k] for k in ("G", "scale", "rho_o", "G_chen")})
    s.set_f(f0)
    return s


def set_of_fixture(d, planar=None, tag=""):
    params = dict(zip(PARAMS, [float(x) for x in d[tag + "params"]]))
    return set_of(int(d["nx"]), int(d["ny"]), d["omega"], params, bool(d[tag + "clumpy"]), d["f0"], planar), params


def droplet_case(nx, ny, clumpy, dtype=np.float64):
    """the issue's case on another grid: the model holding 1.2 x the seeded droplet on a uniform nutrient, at equilibrium"""
    m = NutrientModel(nx, ny, 0.8, 1.25, clumpy=clumpy, dtype=dtype, **CASE)
    rho0 = np.ones((nx, ny, 2), F)
    rho0[:, :, 0] = F(1.2) * noisy_droplet(nx, ny, 10, 0.5, 20240611)
    m.redo_initial_condition(rho0)
    m.set_f(m.f.astype(F))
    return m


def same_bits(a, b):
    return [k for k in b if not np.array_equal(a[k], b[k], equal_nan=True)]


def digest(s):
    g = s.get_fields(("f", "rho", "u", "v", "psi", "pseudo_force_x", "pseudo_force_y"))
    h = hashlib.sha256()
    for k in sorted(g):
        h.update(np.ascontiguousarray(g[k]).tobytes())
    return h.hexdigest()


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planar", (None, True))
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_run_follows_reference_fixture(lbhip, name, planar):
    d = golden(name)
    s, params = set_of_fixture(d, planar)
    done = 0
    for n in STEPS:
        s.run(n - done)
        done = n
        compare("%s after %d steps%s / reference" % (name, n, ", planar" if planar else ""), params, n,
                got_of(s, all_keys(bool(d["clumpy"]))), recorded(d, n))
    s.close()


@pytest.mark.parametrize("box", BOXES, ids=lambda b: "%dx%d" % b)
@pytest.mark.parametrize("clumpy", (False, True))
def test_row_across_the_tile_boundary_follows_the_model(lbhip, clumpy, box):
    """270 x 12, 1000 x 12, 12 x 1000: no fixture; the float64 model from the same float32 start, within the contract at 1, 10 and 50
    steps."""
    nx, ny = box
    m = droplet_case(nx, ny, clumpy)
    s = set_of(nx, ny, (0.8, 1.25), CASE, clumpy, m.f)
    done = 0
    for n in STEPS:
        s.run(n - done), m.run(n - done)
        done = n
        assert float(np.sqrt(m.u ** 2 + m.v ** 2).max()) < 0.15
        compare("%dx%d %s after %d steps / float64 model" % (nx, ny, "clumpy" if clumpy else "plain", n), m.params, n, got_of(s, all_keys(clumpy)), m.state())
    s.close()


@pytest.mark.parametrize("variant", ("plain", "clumpy"))
def test_stages_follow_phases_fixture_and_the_fused_step(lbhip, variant):
    d = golden(PHASES)
    tag, clumpy = variant + "_", variant == "clumpy"
    s, params = set_of_fixture(d, tag=tag)
    stages = (("move", s.move, ("f",)), ("update_hydro", s.update_hydro, ("rho",)), ("update_velocity", s.update_velocity, ("u", "v")),
              ("update_forces", s.update_forces, ("psi", "Fx", "Fy") if clumpy else ()), ("update_feq", s.update_feq, ("feq",)),
              ("collide", s.collide_particles, ("f",)))
    rho_max = float(d[tag + "rho_after_update_hydro"][:, :, 0].max())
    for stage, call, writes in stages:
        call()
        if writes:
            want = {k: d["%s%s_after_%s" % (tag, k, stage)] for k in writes}
            compare("%s after %s / reference" % (variant, stage), params, 1, got_of(s, writes), dict(want, rho=d[tag + "rho_after_update_hydro"]))
    staged = got_of(s, all_keys(clumpy))
    fused, _ = set_of_fixture(d, tag=tag)
    fused.run(1)
    got = got_of(fused, all_keys(clumpy))
    compare("%s fused / reference" % variant, params, 1, got, {k: d["%s%s_after_%s" % (tag, k, st)] for st, _, ws in stages for k in ws if k != "feq"})
    compare("%s fused / stages" % variant, params, 1, got, staged)
    # what does not cross the relaxation is the same arithmetic in both: the same bits
    assert not same_bits({k: got[k] for k in got if k != "f"}, {k: staged[k] for k in staged if k != "f"})
    assert rho_max > 1.
    s.close(), fused.close()


# ---- what the product computes twice: bitwise ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((5, 4), (30, 18), (270, 12), (1000, 12)))
@pytest.mark.parametrize("clumpy", (False, True))
def test_one_run_equals_single_steps_bitwise(lbhip, shape, clumpy):
    m = droplet_case(shape[0], shape[1], clumpy)
    whole, single, split = (set_of(shape[0], shape[1], (0.8, 1.25), CASE, clumpy, m.f) for _ in range(3))
    whole.run(7)
    for _ in range(7):
        single.run(1)
    for n in (3, 4):
        split.run(n, wait=False)
    want = got_of(whole, all_keys(clumpy))
    assert not same_bits(got_of(single, all_keys(clumpy)), want)
    assert not same_bits(got_of(split, all_keys(clumpy)), want)
    for s in (whole, single, split):
        s.close()


@pytest.mark.parametrize("streamed", (0, 1))
def test_velocity_is_the_spectral_velocity_in_both_members(lbhip, streamed):
    from LB_D2Q9.simulation import Simulation
    nx, ny = 30, 18
    m = droplet_case(nx, ny, False)
    s = set_of(nx, ny, (0.8, 1.25), CASE, False, m.f)
    s.update_hydro()
    plain = Simulation(nx, ny, F(0.8), bc="periodic", semantics="diffusion")
    plain.set_f(m.f[:, :, 0])
    plain.update_hydro()
    L = lbhip
    assert L.lb_spectral_velocity(s.solver._h, plain._h, -0.05, streamed) == 0
    plain.sync()
    want = plain.get_fields(("rho", "u", "v"))
    s.update_velocity(streamed=bool(streamed))
    for i in range(2):
        got = s.members[i].get_fields(("u", "v"))
        assert np.array_equal(got["u"], want["u"]) and np.array_equal(got["v"], want["v"]), i
    assert np.array_equal(s.members[0].get_fields(("rho",))["rho"], want["rho"])
    assert np.abs(want["u"]).max() > 1e-3
    s.close(), plain.close()


@pytest.mark.parametrize("shape", ((3, 3), (30, 18), (270, 12)))
def test_without_coupling_each_member_is_a_diffusion_lattice_bitwise(lbhip, shape):
    """G = 0, scale = 0, clumpy = 0: each member after lb_run_nutrient(n) is a twin periodic diffusion handle after lb_run(n) with
    set_variant(0) and zero velocity, bit for bit: the cell arithmetic is k_ad_step's."""
    from LB_D2Q9.simulation import Simulation
    nx, ny = shape
    n = 6
    m = droplet_case(nx, ny, False)
    rng = np.random.default_rng(8)
    f0 = (m.f * (1. + 0.05 * rng.uniform(-1., 1., m.f.shape))).astype(F)
    s = set_of(nx, ny, (0.8, 1.25), dict(CASE, G=0., scale=0.), False, f0)
    s.run(n)
    got = s.get_fields(("f", "rho", "u", "v"))
    assert not got["u"].any() and not got["v"].any()
    zero = np.zeros((nx, ny), F)
    for i, om in enumerate((0.8, 1.25)):
        twin = Simulation(nx, ny, F(om), bc="periodic", semantics="diffusion")
        twin.set_variant(0)
        twin.set_fields(zero, zero, zero)
        twin.set_f(f0[:, :, i])
        twin.run(n)
        want = twin.get_fields(("f", "rho"))
        assert np.array_equal(got["f"][:, :, i], want["f"]) and np.array_equal(got["rho"][:, :, i], want["rho"]), i
        twin.close()
    s.close()


# ---- the stencil ---------------------------------------------------------------------------------------------------------------------
def test_force_reads_exactly_the_cell_and_its_eight_neighbours(lbhip):
    """Adding 0.25 to rho_p at one cell changes F after update_forces at exactly that cell and its eight neighbours (wrapped); psi at
    that cell only."""
    nx, ny = 30, 18
    m = droplet_case(nx, ny, True)
    s = set_of(nx, ny, (0.8, 1.25), CASE, True, m.f)
    s.update_hydro()
    rho = s.get_fields(("rho",))["rho"]
    zero = np.zeros((nx, ny), F)
    s.update_forces()
    base = got_of(s, ("psi", "Fx", "Fy"))
    for cx, cy in ((0, 0), (nx - 1, ny - 1), (14, 9)):
        bumped = rho.copy()
        bumped[cx, cy, 0] += F(0.25)
        s.set_fields(bumped, zero, zero)
        s.update_forces()
        g = got_of(s, ("psi", "Fx", "Fy"))
        changed = (g["Fx"] != base["Fx"]) | (g["Fy"] != base["Fy"])
        want = np.zeros((nx, ny), bool)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                want[(cx + dx) % nx, (cy + dy) % ny] = True
        # (F at the cell itself is psi(x) times a sum that the cell's own psi does not enter: it changes with psi(x))
        assert np.array_equal(changed, want), (cx, cy, np.argwhere(changed != want).tolist())
        assert np.argwhere(g["psi"] != base["psi"]).tolist() == [[cx, cy]]
    s.close()


def test_the_attraction_is_live(lbhip):
    """30 x 18, 50 steps: the clumpy and the plain run differ in rho_p by more than 100 x the tolerance."""
    nx, ny, n = 30, 18, 50
    rho = []
    for clumpy in (False, True):
        s = set_of(nx, ny, (0.8, 1.25), CASE, clumpy, droplet_case(nx, ny, False).f)
        s.run(n)
        rho.append(s.get_fields(("rho",))["rho"][:, :, 0])
        s.close()
    d = maxdiff(rho[0], rho[1])
    print("clumpy - plain in rho_p after %d steps: %.3e (tolerance %.1e)" % (n, d, contract_tol(n)["rho"]))
    assert d > 100. * contract_tol(n)["rho"]


# ---- an external stream --------------------------------------------------------------------------------------------------------------
def test_external_stream_twin(lbhip, tmp_path):
    """tests/nutrient_stream_scenarios.py in a fresh python (torch first: one HIP runtime): the chain on a caller's stream behind a
    delay equals the waiting twin bit for bit, and the delay outlasted four times the enqueue."""
    script = tmp_path / "nutrient_child.py"
    script.write_text(NS.PRELUDE + NS.NUTRIENT + NS.EPILOGUE)
    p = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-lb_amd")],
                       capture_output=True, text=True, timeout=300)
    print("\n".join(l for l in p.stdout.splitlines() if l.startswith(("RATIO", "SCENARIO"))))
    assert p.returncode == 0 and "NUTRIENT_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    assert "SCENARIO nutrient_set_on_an_external_stream OK" in p.stdout


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_reason_and_the_state(lbhip):
    from LB_D2Q9 import _native
    from LB_D2Q9.nutrient_set import Nutrient_Set
    from LB_D2Q9.simulation import Simulation
    L = lbhip
    nx, ny = 30, 18
    m = droplet_case(nx, ny, True)
    s = set_of(nx, ny, (0.8, 1.25), CASE, True, m.f)
    s.run(2)
    before = digest(s)
    other = Nutrient_Set(20, 12, 0.8, 1.25)
    tiny = Nutrient_Set(2, 4, 0.8, 1.25)
    planar = Simulation(nx, ny, 0.8, bc="periodic", semantics="diffusion", planar=True)
    open_box = Simulation(nx, ny, 0.8, bc="open", semantics="diffusion")
    field = Simulation(nx, ny, 0.8, bc="periodic", semantics="multifield")
    p, q, sp = s.members[0]._h, s.members[1]._h, s.solver._h
    arr = lambda *hs: (ct.c_void_p * len(hs))(*hs)
    P = lambda **kw: ct.byref(_native.NutrientParams(*[dict(dict(G=0.01, scale=-0.05, clumpy=1, rho_o=1., G_chen=-1.), **kw)[k]
                                                      for k in ("G", "scale", "clumpy", "rho_o", "G_chen")]))
    ARG = -1

    def refused(rc, *words):
        msg = L.lb_last_error().decode()
        assert rc == ARG, (rc, msg)
        for w in words:
            assert w.lower() in msg.lower(), (w, msg)

    refused(L.lb_run_nutrient(sp, arr(p), 1, P(), 1), "exactly 2", "count")
    refused(L.lb_run_nutrient(sp, arr(p, q, q), 3, P(), 1), "exactly 2", "count")
    refused(L.lb_run_nutrient(sp, arr(p, p), 2, P(), 1), "twice")
    refused(L.lb_run_nutrient(sp, arr(p, field._h), 2, P(), 1), "LB_SEM_DIFFUSION")
    refused(L.lb_run_nutrient(sp, arr(p, open_box._h), 2, P(), 1), "geometry")          # (the family is part of what members share)
    other_open = Simulation(nx, ny, 0.8, bc="open", semantics="diffusion")
    refused(L.lb_run_nutrient(sp, arr(open_box._h, other_open._h), 2, P(), 1), "periodic")
    refused(L.lb_run_nutrient(sp, arr(p, other.members[1]._h), 2, P(), 1), "geometry")
    refused(L.lb_run_nutrient(sp, arr(p, planar._h), 2, P(), 1), "layout")
    refused(L.lb_run_nutrient(other.solver._h, arr(p, q), 2, P(), 1), "spectral solver's grid")
    refused(L.lb_run_nutrient(None, arr(p, q), 2, P(), 1), "null spectral solver")
    refused(L.lb_run_nutrient(sp, arr(p, q), 2, None, 1), "null parameters")
    refused(L.lb_run_nutrient(tiny.solver._h, tiny._handles, 2, P(), 1), "clumpy", ">= 3")
    refused(L.lb_run_nutrient(sp, arr(p, q), 2, P(rho_o=0.), 1), "rho_o")
    for bad in (dict(G=float("nan")), dict(scale=float("inf")), dict(rho_o=float("-inf")), dict(G_chen=float("nan"))):
        refused(L.lb_run_nutrient(sp, arr(p, q), 2, P(**bad), 1), "finite")
    refused(L.lb_run_nutrient(sp, arr(p, q), 2, P(), -1), "negative")
    # the stages refuse alike
    refused(L.lb_nutrient_velocity(sp, arr(p, p), 2, -0.05, 0), "twice")
    refused(L.lb_nutrient_velocity(sp, arr(p, q), 2, float("nan"), 0), "finite")
    refused(L.lb_nutrient_velocity(other.solver._h, arr(p, q), 2, -0.05, 0), "spectral solver's grid")
    refused(L.lb_update_forces_nutrient(arr(p), 1, P()), "exactly 2")
    refused(L.lb_update_forces_nutrient(arr(p, q), 2, P(clumpy=0)), "clumpy")
    refused(L.lb_collide_nutrient(arr(p, q, q), 3, P()), "exactly 2")
    refused(L.lb_collide_nutrient(arr(p, q), 2, P(rho_o=0.)), "rho_o")
    refused(L.lb_get_nutrient_fields(arr(p, field._h), 2, None, None, None), "LB_SEM_DIFFUSION")
    # no kernel has run: the state is what it was, and the set still runs
    assert digest(s) == before
    s.run(2)
    assert all(c["n_nonfinite"] == 0 for c in s.check())
    for x in (s, other, tiny, planar, open_box, other_open, field):
        x.close()
    with pytest.raises(_native.LbError, match="2\\^a"):
        Nutrient_Set(21, 13, 0.8, 1.25)                         # (not a transform length: refused before a device is touched)


# ---- the drop-in classes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clumpy", (False, True))
def test_dropin_class_follows_its_fixture(lbhip, clumpy):
    from LB_D2Q9.reaction_diffusion.surfactant_nutrient_waves import Clumpy_Surfactant_Nutrient_Wave, Surfactant_Nutrient_Wave
    d = golden("sn_clumpy_30x18" if clumpy else "sn_plain_30x18")
    kw = dict(Lx=3, Ly=1.8, N=10, time_prefactor=1, lam=1, R0=0.5, Dn=0.1, vc=0.5, rng=5)
    sim = Clumpy_Surfactant_Nutrient_Wave(rho_o=1., G_chen=-1., **kw) if clumpy else Surfactant_Nutrient_Wave(**kw)
    assert (sim.nx, sim.ny) == (30, 18) and sim.omega == F(d["omega"][0]) and sim.omega_n == F(d["omega"][1])
    # its own seeded start: the noisy droplet on a uniform nutrient, at the equilibrium of the velocity it gives itself
    g = sim.get_fields()
    assert g["rho"].shape == (30, 18, 2) and g["f"].shape == g["feq"].shape == (30, 18, 2, 9) and g["u"].shape == (30, 18)
    assert g["rho"].flags.f_contiguous and g["f"].flags.f_contiguous
    assert np.all(g["rho"][:, :, 1] == 1.) and abs(float(g["rho"][15, 9, 0]) - 1.2) < 0.25 and np.array_equal(g["f"], g["feq"])
    assert np.abs(g["u"]).max() > 1e-3
    if clumpy:
        assert g["psi"].shape == g["pseudo_force_x"].shape == g["pseudo_force_y"].shape == (30, 18) and g["psi"].any()
    # the fixture's start through redo_initial_condition
    sim.redo_initial_condition(d["rho0"])
    assert maxdiff(np.asarray(sim.f), d["f0"]) <= contract_tol(1)["f"]
    params = dict(zip(PARAMS, [float(x) for x in d["params"]]))
    sim.run(10)
    got = dict(f=np.asarray(sim.f), rho=np.asarray(sim.rho), u=np.asarray(sim.u), v=np.asarray(sim.v))
    if clumpy:
        got.update(psi=np.asarray(sim.psi), Fx=np.asarray(sim.pseudo_force_x), Fy=np.asarray(sim.pseudo_force_y))
    compare("%s through its class, 10 steps" % ("clumpy" if clumpy else "plain"), params, 10, got, recorded(d, 10))
    # the phase methods make the reference's step
    before = np.asarray(sim.f).astype(np.float64).sum()
    sim.move(), sim.move_bcs(), sim.update_hydro(), sim.update_feq(), sim.collide_particles()
    assert abs(np.asarray(sim.f).astype(np.float64).sum() - before) < 1e-3
    sim.engine.close()
