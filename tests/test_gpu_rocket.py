"""Surfactant-propelled colonies on the GPU: the one-launch step (k_ry_step), the two-launch step (k_ry_moments + k_ry_collide) and
the un-fused stages against the fixtures recorded from the reference's C and against the numpy model (tests/rocket_model.py); the
three forms against each other, bitwise; split runs, the planar layout, checkpoints and an external stream, bitwise; the plain
diffusion limit; the stencil's locality; the drop-in classes; refusals.
Bounds: the project's parity contract (contract_tol) as tests/test_rocket_cpu.py states it for each array; everything the product
computes twice must agree bit for bit."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from rocket_model import PARAMS, W64, RocketModel, from_fixture
from scalar_model import contract_tol
from test_rocket_cpu import PHASE_FIXTURES, RUN_FIXTURES, compare, recorded, state, writes

pytestmark = pytest.mark.gpu

F = np.float32
MODES = ("flow", "forces")
# model / fixture name -> Surfactant_Colony.get_fields key
KEYS = dict(f="f", feq="feq", rho="rho", u="u", v="v", Fx="pseudo_force_x", Fy="pseudo_force_y", Sx="surface_force_x", Sy="surface_force_y")


def rows():
    from LB_D2Q9 import _native
    return _native.RY_ROWS


def shapes():
    """(3, 3), (5, 4): a lane holding both wraps; (37, 23), (63, 17), (255, 33): a wrap inside a lane's last quad; (64, 16): the wrap at
    a lane boundary; (256, R), (257, R + 1), (258, 9): a tile edge at 256 and two cells past it, row counts below, at and one past a
    workgroup's rows; (1000, 12): four tiles, the last one ragged."""
    R = rows()
    return ((3, 3), (5, 4), (37, 23), (63, 17), (64, 16), (255, 33), (256, R), (257, R + 1), (258, 9), (1000, 12))


def all_keys(mode):
    return ("f", "rho", "u", "v", "op", "Fx", "Fy") + (("Sx", "Sy") if mode == "forces" else ())


def got_of(s, which):
    keys = [KEYS[k] if k != "op" else ("psi" if s.mode == "flow" else "S") for k in which]
    g = s.get_fields(tuple(keys))
    return {k: g[kk] for k, kk in zip(which, keys)}


def colony_of(d, planar=None):
    """a colony in the state of fixture / case d"""
    from LB_D2Q9.coupled import Surfactant_Colony
    s = Surfactant_Colony(int(d["nx"]), int(d["ny"]), F(d["omega"][0]), F(d["omega"][1]), mode=str(d["mode"]), planar=planar)
    s.set_params(**dict(zip(PARAMS, [float(x) for x in d["params"]])))
    s.set_f(d["f0"])
    return s


def smooth_case(nx, ny, mode, seed):
    """a smooth random state with a non-zero surfactant: a few long waves of random phase under 2 % of noise; growth, secretion, both
    stencils and the force term all act"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    wave = lambda: sum(a * np.sin(2. * np.pi * (kx * x / nx + ky * y / ny) + rng.uniform(0., 6.28))
                       for a, kx, ky in ((0.2, 1, 0), (0.15, 0, 1), (0.1, 1, 1)))
    rho = np.stack([0.7 + wave(), 0.6 + wave()], axis=2)
    f0 = W64 * rho[:, :, :, None] * (1. + 0.02 * rng.uniform(-1., 1., (nx, ny, 2, 9)))
    params = dict(G=0.01, G_c=0.02, epsilon=0.5, rho_o=0.9, G_chen=-0.8, c_o=0.25, alpha=2.)
    return dict(nx=nx, ny=ny, mode=mode, omega=np.array([0.8, 1.1], F), params=np.array([params[k] for k in PARAMS], F), f0=f0.astype(F))


def hip_runtime():
    """The HIP runtime the library itself has loaded (one runtime per process: a stream of another one would mean nothing to it)."""
    with open("/proc/self/maps") as maps:
        paths = {line.split()[-1] for line in maps if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = ct.CDLL(paths.pop())
    hip.hipStreamCreateWithFlags.argtypes = [ct.POINTER(ct.c_void_p), ct.c_uint]
    hip.hipStreamSynchronize.argtypes = [ct.c_void_p]
    hip.hipStreamDestroy.argtypes = [ct.c_void_p]
    return hip


def same_bits(a, b):
    return [k for k in b if not np.array_equal(a[k], b[k], equal_nan=True)]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("two launches", "one launch", "stages"))
@pytest.mark.parametrize("name", RUN_FIXTURES)
def test_run_follows_reference_fixture_and_model(lbhip, name, form):
    d = golden(name)
    s, m = colony_of(d), from_fixture(d, F)
    s.set_variant({"two launches": 0, "one launch": 1, "stages": -1}[form])
    done = 0
    for n in [int(k) for k in d["steps"]]:
        if form == "stages":
            for _ in range(n - done):
                s.step_phases()
        else:
            s.run(n - done)
        m.run(n - done)
        done = n
        want = recorded(d, n)
        got = got_of(s, all_keys(s.mode))
        compare("%s after %d steps, %s / reference" % (name, n, form), m, n, got, want)
        compare("%s after %d steps, %s / model" % (name, n, form), m, n, got, state(m), rho_max=float(want["rho"].max()))
    s.close()


@pytest.mark.parametrize("name", PHASE_FIXTURES)
def test_stages_follow_phases_fixture(lbhip, name):
    """move is data movement: exact; the rest within the contract of one step; the floored links exactly the fixture's."""
    d = golden(name)
    s, m = colony_of(d), from_fixture(d, F)
    calls = dict(move="move", update_hydro="update_hydro", update_velocity="update_velocity", update_forces="update_forces",
                 update_feq="update_feq", collide="collide_particles")
    rho_max = float(d["rho_after_update_hydro"].max())
    for stage in m.STAGES:
        getattr(s, calls[stage])()
        want = {k: d["%s_after_%s" % (k, stage)] for k in writes(m.mode, stage)}
        got = got_of(s, list(want))
        if stage == "move":
            assert np.array_equal(got["f"], want["f"].astype(F))
        else:
            compare("%s after %s" % (name, stage), m, 1, got, want, rho_max=rho_max)
    assert np.array_equal(got["f"][:, :, 0, :] == 0, d["clamped"])
    # ... and in both fused forms
    for variant in (0, 1):
        r = colony_of(d)
        r.set_variant(variant)
        r.run(1)
        got = got_of(r, all_keys(r.mode))
        assert np.array_equal(got["f"][:, :, 0, :] == 0, d["clamped"]), variant
        want = {k: d["%s_after_%s" % (k, st)] for st in m.STAGES if st != "move" for k in writes(m.mode, st) if k != "feq"}
        compare("%s, variant %d" % (name, variant), m, 1, got, want, rho_max=rho_max)
        r.close()
    s.close()


# ---- the fused step against the model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("mode", MODES)
def test_fused_step_follows_the_model(lbhip, mode, variant):
    for nx, ny in shapes():
        d = smooth_case(nx, ny, mode, 7 * nx + ny)
        n = 8 + nx % 6
        s, m = colony_of(d), from_fixture(d, np.float64)
        s.set_variant(variant)
        s.run(n)
        m.run(1)
        # (the coupling acts: a velocity and a force well above rounding in the first step; the small boxes smooth out fastest)
        assert np.abs(m.u).max() > (1e-3 if ny > 4 else 1e-5) and np.abs(m.Fx).max() > 1e-4 and m.rho[:, :, 1].min() > 0.1
        m.run(n - 1)
        compare("%dx%d %s variant %d, %d steps" % (nx, ny, mode, variant, n), m, n, got_of(s, all_keys(mode)), state(m))
        s.close()


# ---- what the product computes twice -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_one_launch_equals_two_launches_equals_stages_bitwise(lbhip, mode):
    for nx, ny in shapes():
        d = smooth_case(nx, ny, mode, 100 + nx)
        a, b, c = colony_of(d), colony_of(d), colony_of(d)
        a.set_variant(0)
        c.set_variant(1)
        for n in range(1, 4 if nx > 300 else 6):
            a.run(1)
            b.step_phases()
            c.run(1)
            want = got_of(b, all_keys(mode))
            bad = same_bits(got_of(a, all_keys(mode)), want), same_bits(got_of(c, all_keys(mode)), want)
            assert not bad[0] and not bad[1], (nx, ny, mode, n, bad)
        for s in (a, b, c):
            s.close()


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("mode", MODES)
def test_split_runs_planar_layout_checkpoint_and_stream_are_bitwise(lbhip, tmp_path, mode, variant):
    from LB_D2Q9.coupled import Surfactant_Colony
    hip = hip_runtime()
    for nx, ny in ((37, 23), (257, rows() + 1)):
        d = smooth_case(nx, ny, mode, 5 + nx)
        whole = colony_of(d)
        whole.set_variant(variant)
        whole.run(9)
        want = got_of(whole, all_keys(mode))
        # 9 = 4 + 1 + 4, without a host wait in between
        split = colony_of(d)
        split.set_variant(variant)
        for n in (4, 1, 4):
            split.run(n, wait=False)
        assert not same_bits(got_of(split, all_keys(mode)), want), (nx, ny, "split")
        # each plane contiguous
        planar = colony_of(d, planar=True)
        planar.set_variant(variant)
        planar.run(9)
        assert not same_bits(got_of(planar, all_keys(mode)), want), (nx, ny, "planar")
        # checkpoint after 4 -> restore -> 5 more; the parameters travel with it, the restored fields are the saved ones
        first = colony_of(d)
        first.set_variant(variant)
        first.run(4)
        first.save_checkpoint(tmp_path / "colony")
        saved = got_of(first, all_keys(mode))
        again = Surfactant_Colony.from_checkpoint(tmp_path / "colony")
        assert again.mode == mode and again.get_params() == first.get_params() and again.get_params()["mode"] == mode
        assert not same_bits(got_of(again, all_keys(mode)), saved), (nx, ny, "restored")
        again.set_variant(variant)
        again.run(5)
        assert not same_bits(got_of(again, all_keys(mode)), want), (nx, ny, "checkpoint")
        # an external stream
        ext, stream = colony_of(d), ct.c_void_p()
        assert hip.hipStreamCreateWithFlags(ct.byref(stream), 1) == 0 and stream.value      # (hipStreamNonBlocking)
        ext.set_variant(variant)
        ext.use_stream(stream.value)
        for n in (4, 5):
            ext.run(n, wait=False)
        assert hip.hipStreamSynchronize(stream) == 0
        assert not same_bits(got_of(ext, all_keys(mode)), want), (nx, ny, "stream")
        ext.use_stream(None)
        assert hip.hipStreamDestroy(stream) == 0
        for s in (whole, split, planar, first, again, ext):
            s.close()


@pytest.mark.parametrize("variant", (0, 1))
def test_without_coupling_the_population_is_a_fisher_lattice(lbhip, variant):
    """epsilon = G_chen = G_c = 0 in mode 'flow': the population is a periodic semantics='diffusion' lattice with the same G (no
    velocity), to the contract (the two cells round differently); the surfactant stays identically 0."""
    from LB_D2Q9.coupled import Surfactant_Colony
    from LB_D2Q9.simulation import Simulation
    nx, ny, n = 37, 23, 12
    d = smooth_case(nx, ny, "flow", 77)
    f0 = d["f0"].copy()
    f0[:, :, 1] = 0
    s = Surfactant_Colony(nx, ny, 0.8, 1.1, mode="flow")
    s.set_params(G=0.01, G_c=0., epsilon=0., G_chen=0., rho_o=1.)
    s.set_variant(variant)
    s.set_f(f0)
    ref = Simulation(nx, ny, 0.8, bc="periodic", semantics="diffusion")
    ref.set_reaction(0.01)
    zero = np.zeros((nx, ny), F)
    ref.set_fields(zero, zero, zero)
    ref.set_f(f0[:, :, 0])
    s.run(n)
    ref.run(n)
    got, want = s.get_fields(("f", "rho", "u", "v")), ref.get_fields(("f", "rho"))
    tol = contract_tol(n)
    for k in ("f", "rho"):
        diff = float(np.abs(got[k][:, :, 0].astype(np.float64) - want[k]).max())
        print("%s: %.2e / %.1e" % (k, diff, tol[k]))
        assert diff <= tol[k]
    assert not got["f"][:, :, 1].any() and not got["rho"][:, :, 1].any() and not got["u"].any() and not got["v"].any()
    s.close()
    ref.close()


# ---- the stencil's locality ----------------------------------------------------------------------------------------------------
def test_velocity_reads_exactly_the_eight_neighbours(lbhip):
    """Adding 0.25 to the surfactant at one cell changes u, v after update_velocity at exactly its eight neighbours (wrapped)."""
    from LB_D2Q9.coupled import Surfactant_Colony
    nx, ny = 37, 23
    d = smooth_case(nx, ny, "flow", 9)
    s = colony_of(d)
    s.update_hydro()
    rho = s.get_fields(("rho",))["rho"]
    zero = np.zeros((nx, ny), F)
    s.update_velocity()
    base = s.get_fields(("u", "v"))
    for cx, cy in ((0, 0), (nx - 1, ny - 1), (17, 11)):
        bumped = rho.copy()
        bumped[cx, cy, 1] += F(0.25)
        s.set_fields(bumped, zero, zero)
        s.update_velocity()
        g = s.get_fields(("u", "v"))
        changed = (g["u"] != base["u"]) | (g["v"] != base["v"])
        want = np.zeros((nx, ny), bool)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if dx or dy:
                    want[(cx + dx) % nx, (cy + dy) % ny] = True
        assert np.array_equal(changed, want), (cx, cy, np.argwhere(changed != want).tolist())
    s.close()


# ---- the drop-in classes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_dropin_class_follows_its_fixture(lbhip, mode):
    from LB_D2Q9.rocket_yeast.rocket_yeast import Rocket_Yeast
    from LB_D2Q9.rocket_yeast.rocket_yeast_forces_only import Rocket_Yeast_Forces_Only
    name = "ry_flow_37x23" if mode == "flow" else "ry_forces_37x23"
    d = golden(name)
    cls = Rocket_Yeast if mode == "flow" else Rocket_Yeast_Forces_Only
    sim = cls(Lx=3.7, Ly=2.3, R0=1., Dc=1., N=10, rng=5)
    assert (sim.nx, sim.ny) == (37, 23) and sim.omega == F(d["omega"][0]) and sim.omega_c == F(d["omega"][1])
    # its own seeded start: the droplet at equilibrium, no surfactant, no flow in mode 'flow'; the same with the same seed
    g = sim.get_fields()
    rho0 = g["rho"]
    assert rho0.shape == (37, 23, 2) and g["f"].shape == (37, 23, 2, 9) and not rho0[:, :, 1].any()
    assert abs(float(rho0[18, 11, 0]) - 1.) < 0.2 and rho0[0, 0, 0] < 0.05
    if mode == "flow":
        assert not g["u"].any() and np.abs(g["f"] - (W64 * rho0[:, :, :, None].astype(np.float64))).max() < 2e-7
        assert g["psi"].shape == (37, 23) and g["pseudo_force_x"].shape == (37, 23)
    assert np.array_equal(g["f"], g["feq"])
    twin = cls(Lx=3.7, Ly=2.3, R0=1., Dc=1., N=10, rng=5)
    assert np.array_equal(twin.get_fields()["f"], g["f"])
    twin.engine.close()
    # the fixture's start through redo_initial_condition: f0 = w rho0 is the equilibrium at rest of its own density
    rho_fix = d["f0"].astype(np.float64).sum(axis=3)
    sim.redo_initial_condition(rho_fix)
    if mode == "flow":
        assert np.abs(np.asarray(sim.f) - d["f0"]).max() < 2e-7
    sim.engine.set_f(d["f0"])
    m = from_fixture(d, F)
    done = 0
    for n in [int(k) for k in d["steps"]][:3]:
        sim.run(n - done)
        done = n
        want = recorded(d, n)
        got = dict(rho=np.asarray(sim.rho), u=np.asarray(sim.u), v=np.asarray(sim.v), Fx=np.asarray(sim.pseudo_force_x),
                   Fy=np.asarray(sim.pseudo_force_y), op=np.asarray(sim.psi if mode == "flow" else sim.S))
        if mode == "forces":
            got.update(Sx=np.asarray(sim.surface_force_x), Sy=np.asarray(sim.surface_force_y))
        if "f" in want:
            got["f"] = np.asarray(sim.f)
        compare("%s through %s, %d steps" % (name, cls.__name__, n), m, n, got, want)
    sim.engine.close()


def test_check_max_ulb_warns_once_per_run(lbhip, capsys):
    from LB_D2Q9.rocket_yeast.rocket_yeast import Rocket_Yeast
    sim = Rocket_Yeast(Lx=2., Ly=1.5, R0=1., Dc=1., N=10, rng=1, check_max_ulb=True, mach_tolerance=1e-6)
    capsys.readouterr()
    sim.run(5)
    assert capsys.readouterr().out.count("max_ulb is greater than cs/10!") == 1
    sim.engine.close()


# ---- health, refusals ------------------------------------------------------------------------------------------------------------
def test_check_works_on_both_members(lbhip):
    d = smooth_case(37, 23, "flow", 3)
    s = colony_of(d)
    s.run(3)
    g = s.get_fields(("f", "u", "v"))
    for i, c in enumerate(s.check()):
        assert c["n_nonfinite"] == 0 and abs(c["sum_rho"] - float(g["f"][:, :, i].astype(np.float64).sum())) < 1e-3
        want = float(np.sqrt(3. * (g["u"].astype(np.float64) ** 2 + g["v"].astype(np.float64) ** 2).max()))
        assert abs(c["max_mach"] - want) < 1e-6
    s.close()


def test_refusals_are_status_codes_with_the_named_words(lbhip):
    from LB_D2Q9 import _native
    from LB_D2Q9.coupled import Surfactant_Colony
    from LB_D2Q9.simulation import Simulation
    L = lbhip
    s = Surfactant_Colony(16, 12, 0.8, 0.9)
    other = Surfactant_Colony(20, 12, 0.8, 0.9)
    planar = Surfactant_Colony(16, 12, 0.8, 0.9, planar=True)
    plain = Simulation(16, 12, 0.8, bc="periodic", semantics="diffusion")
    p, c = s.members[0]._h, s.members[1]._h
    arr = lambda *hs: (ct.c_void_p * len(hs))(*hs)
    ARG, STATE = -1, -3

    def refused(rc, code, *words):
        msg = L.lb_last_error().decode()
        assert rc == code, (rc, msg)
        for w in words:
            assert w.lower() in msg.lower(), (w, msg)

    # lb_run_rocket: LB_ERR_ARG naming the reason
    refused(L.lb_run_rocket(arr(p), 1, 1), ARG, "exactly 2", "count")
    refused(L.lb_run_rocket(arr(p, c, c), 3, 1), ARG, "exactly 2", "count")
    refused(L.lb_run_rocket(arr(p, other.members[1]._h), 2, 1), ARG, "geometry")
    refused(L.lb_run_rocket(arr(p, planar.members[1]._h), 2, 1), ARG, "layout")
    refused(L.lb_run_rocket(arr(p, p), 2, 1), ARG, "twice")
    refused(L.lb_run_rocket(arr(p, plain._h), 2, 1), ARG, "non-rocket")
    refused(L.lb_run_rocket(arr(p, c), 2, -1), ARG, "negative")
    bad = _native.RocketParams(7, 0., 0., 0., 1., 0., 1., 1.)
    refused(L.lb_set_rocket(arr(p, c), 2, ct.byref(bad)), ARG, "mode")
    bad = _native.RocketParams(0, 0., 0., 0., 0., 0., 1., 1.)
    refused(L.lb_set_rocket(arr(p, c), 2, ct.byref(bad)), ARG, "rho_o")
    bad = _native.RocketParams(1, 0., 0., 0., 1., 0., 0., 1.)
    refused(L.lb_set_rocket(arr(p, c), 2, ct.byref(bad)), ARG, "c_o")
    refused(L.lb_set_variant(p, 2), STATE, "LB_SEM_ROCKET")
    # what a lattice of a colony does not take: LB_ERR_STATE naming the semantics
    for h in (p, c):
        buf = np.zeros(16 * 12 * 9, F)
        i32 = np.zeros(16 * 13, np.int32)
        calls = dict(
            lb_run=lambda: L.lb_run(h, 1), lb_run_coupled=lambda: L.lb_run_coupled(arr(h), 1, 1), lb_run_batch=lambda: L.lb_run_batch(arr(h), 1, 1),
            lb_run_fluids=lambda: L.lb_run_fluids(arr(h), 1, 1), lb_run_group=lambda: L.lb_run_group(arr(h), 1, 1),
            lb_collide_particles=lambda: L.lb_collide_particles(h),
            lb_set_mask=lambda: L.lb_set_mask(h, i32.ctypes.data), lb_set_mask_halo=lambda: L.lb_set_mask_halo(h, i32.ctypes.data, i32.ctypes.data),
            lb_step_boundary=lambda: L.lb_step_boundary(h, 0), lb_step_interior=lambda: L.lb_step_interior(h, 0), lb_step_finish=lambda: L.lb_step_finish(h),
            lb_halo_export=lambda: L.lb_halo_export(h, 0, buf.ctypes.data), lb_halo_import=lambda: L.lb_halo_import(h, 0, buf.ctypes.data),
            lb_halo_floats=lambda: L.lb_halo_floats(h), lb_set_slab_cycle=lambda: L.lb_set_slab_cycle(h, 3),
            lb_autotune=lambda: L.lb_autotune(h), lb_autotune_quick=lambda: L.lb_autotune_quick(h, 100),
            lb_solve=lambda: L.lb_solve(h, 1, None, None, None), lb_solve_reset=lambda: L.lb_solve_reset(h),
            lb_set_poisson=lambda: L.lb_set_poisson(h, 0., 1., 1e-6), lb_set_source=lambda: L.lb_set_source(h, buf.ctypes.data, 0),
            lb_set_reaction=lambda: L.lb_set_reaction(h, 0.1), lb_set_velocity_from=lambda: L.lb_set_velocity_from(h, plain._h),
            lb_set_porous=lambda: L.lb_set_porous(h, 1., 0., 1., 0.), lb_set_body_force=lambda: L.lb_set_body_force(h, 0., 0.),
            lb_set_interactions=lambda: L.lb_set_interactions(arr(h), 1, None, 0), lb_set_reactions=lambda: L.lb_set_reactions(arr(h), 1, None, 0),
            lb_get_interactions=lambda: L.lb_get_interactions(h, None, None), lb_get_reactions=lambda: L.lb_get_reactions(h, None, None),
            lb_edge_floats=lambda: L.lb_edge_floats(h), lb_get_edge_state=lambda: L.lb_get_edge_state(h, buf.ctypes.data),
            lb_set_edge_state=lambda: L.lb_set_edge_state(h, buf.ctypes.data), lb_get_corner_state=lambda: L.lb_get_corner_state(h, buf.ctypes.data),
            lb_set_corner_state=lambda: L.lb_set_corner_state(h, buf.ctypes.data))
        for name, call in calls.items():
            refused(call(), STATE, "LB_SEM_ROCKET", name)
    # the rocket calls on other handles
    refused(L.lb_get_rocket(plain._h, ct.byref(_native.RocketParams())), STATE, "LB_SEM_ROCKET")
    # ... and the colony is untouched: it still runs, in the kernel the planner names
    assert s.hot_kernel().startswith("k_ry_step") and "%d owned rows" % rows() in s.hot_kernel()
    assert s.members[0].steps_per_launch() == 1 and s.members[0].plan_launches(3) == [1, 1, 1]
    s.set_variant(0)
    assert s.hot_kernel().startswith("k_ry_moments + k_ry_collide")
    s.set_f(smooth_case(16, 12, "flow", 1)["f0"])
    s.run(2)
    assert all(c["n_nonfinite"] == 0 for c in s.check())
    for x in (s, other, planar, plain):
        x.close()
