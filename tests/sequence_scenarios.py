"""Random call sequences for every handle kind, and the players that run one (test infrastructure; not a test module).

A sequence is a list of ops, each a tuple of plain Python values (a name, then ints, floats, tuples or None), drawn from a
seeded numpy generator: the same (kind, family, seed) always gives the same list.  Arrays never sit in an op: an op carries a
payload seed and `payload()` makes the array from it, the same one for every player.

  EFFECTIVE ops change the physics; every player makes them:  run(n), phase_step, set_f, and the kind's own state-changing
  calls (E_OPS below) -- among them fed_phase_step, the phases with a supplied field of normals on every noisy lattice
  (set_noise_field(z), the phases, set_noise_field(None)).
  TRANSPARENT ops must change nothing; only the subject makes them: reads, the planner's answers, set_variant, the mask
  uploaded again, a set's own solver used on an unrelated charge, a checkpoint round trip through a closed handle (T_OPS below; a set
  without a file format of its own goes member by member into a fresh set), and run(n) split into run(a, wait=False); run(n - a)
  (the third entry of a run op; the other players ignore it).  They are shuffled and land at random places of the list, except
  that every variant word stands directly in front of a run (so that it selects something), one read at least lies behind a
  stepping op, and the mask is uploaded again or taken off and on while one is set.

Three players (tests/test_gpu_sequences.py): the subject (a GPU handle, E and T ops, from the automatic variant), the twin (a
GPU handle pinned to the plainest kernel, E ops only, every run(n) as n x run(1)) and the reference (oracle.O2Sim for the
flow kinds, the kind's numpy model in float64 otherwise).  tests/test_sequences_cpu.py plays the
references alone.

Amplitudes, tables and parameters are chosen so that every reference stays in the range the parity contract was established
in (rho 0.5 ... 1.5, |u| < 0.15 for the flow kinds) over the 120 steps a sequence may take, mid-life changes included; where a
collision has thresholds (the noisy lattices, the strains on a nutrient, the colony) every thresholded quantity stays far from its
threshold (STEP_CAP below), so that every cell is compared.

The kinds 'rocket' (coupled.Surfactant_Colony), 'nutrient' (nutrient_set.Nutrient_Set), 'noise' (noisy_simulation.NoisySimulation),
'expansion' (expansion_set.Expansion_Set) and 'screened' (a scalar lattice and a spectral_poisson.Screened_Poisson under
lb_run_screened / lb_spectral_velocity: ScreenedWave below) came after the first six; their keys into the generators follow the first
six's, whose op lists have not moved (tests/test_sequences_cpu.py holds a digest of each).

The kind 'advected' (coupled.Advected_Scalars under lb_run_advected: a flow and the scalars it carries) came last, its key behind the
others'.  Its members are unlike lattices that also step alone between the set's runs, so it has a generator (_generate_advected), players
(AdvectedGpu, AdvectedRef) and a hold (hold_advected) of its own; cut_points, counts and the tables above serve it as they are.
"""
import os

import numpy as np

F = np.float32
W64 = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)

KINDS = ("flow", "scalar", "multifield", "poisson", "porous", "multifluid", "rocket", "nutrient", "noise", "expansion", "screened", "advected")
SEEDS = tuple(range(6))
RUN_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 13, 16, 17, 33, 40)     # every fused depth, the 16-launch graph replay and its remainder
MAX_E, MAX_T, MAX_STEPS = 10, 15, 120
# The steps of a life of the kinds whose collision has thresholds (rho < zero_cutoff -> 0, a link < 0 -> 0, rho outside [0, 1] -> NaN):
# the largest cap, at most MAX_STEPS, at which the float64 model of every one of the kind's twelve cases keeps each thresholded quantity
# further from its threshold than twice the contract's bound (tests/test_sequences_cpu.py holds this and prints the smallest margin =
# distance / (2 x bound) per kind).  All three hold at the full 120 -- the longest lives of these seeds take 101, 82 and 67 steps -- with margins
#   rocket     the population's links 1.2e3
#   noise      rho against 0 and 1  5.1e3, the links 1.8e2
#   expansion  rho against zero_cutoff  8.2e3, the links 3.9e2
# so no kind is cut short.  What keeps them there: entering edge links of the size w_k rho of the densities inside (payload), the
# strengths of tests/test_gpu_noise.py's and tests/test_gpu_expansion.py's smooth cases.
STEP_CAP = dict(rocket=120, noise=120, expansion=120)
N_VARIANTS, VARIANT_DEPTH = 2, 8               # variant words per sequence; the steps in one call that let every word's kernel run

FAMILIES = dict(
    flow=("pipe", "pipe-eager", "periodic", "periodic-eager", "cavity", "cavity-eager", "velocity_inlet", "velocity_inlet-eager"),
    scalar=("periodic", "open"),
    multifield=("box", "periodic"),
    poisson=("dirichlet",),
    porous=("periodic", "zero_gradient"),
    multifluid=("periodic", "zero_gradient"),
    rocket=("flow", "forces"),
    nutrient=("plain", "clumpy"),                   # (the value of `clumpy` a life starts with; it is toggled both ways inside one)
    noise=("periodic", "open"),
    expansion=("periodic", "open"),
    screened=("periodic", "open"),
    advected=("eager", "lazy"),                     # (the flow handle's flag)
)

# The smallest shapes at which each mechanism still engages.
#   flow, periodic: 516 x 130 -- nx >= 512 and >= 128 rows, so that every marching kernel and the LDS tiles apply, nx % 4 == 0 as the
#       periodic marches need; <= 768^2, so that single steps replay from the captured graph.
#   flow, walled and velocity inlet: 517 x 131 -- the same with an odd width (the east wall a lane's first cell) and an odd height.
#   scalar: 130 x 50 -- two workgroups in x, nx no multiple of 4, more than one tile of k_ad_tile4 each way.
#   multifield: 258 x 9 -- two workgroups in x with two cells in the second, three fields.
#   poisson: 261 x 9 -- two workgroups in x, three in y, nx no multiple of 4, the last lane straddling the east wall.
#   porous: 261 x 9 (as above) and 256 x 4 (exactly one workgroup, the east edge inside a lane), alternating with the seed.
#   multifluid: 517 x 5 with three fluids (three workgroups in x: one has neighbours on both sides of its column halo; ny = 2 * 2 + 1
#       for the two rows a workgroup of k_mc_step owns), 261 x 9 and 6 x 13 with two (ny = 2 * 6 + 1 for its six rows), by seed % 3.
#   noise: the scalar kind's 130 x 50 -- with it, a width that is no multiple of 4: the periodic seam of k_ad_tile4 takes the per-cell noise path.
#   expansion: 261 x 9 (two workgroups in x, the last lane straddling the east edge) and 37 x 23 (nx % 4 == 1, several workgroups in y, the
#       last ragged), alternating with the seed; 1 + seed % 3 strains.
#   nutrient, screened: 270 x 12 (a second workgroup in x, 270 % 4 == 2, three workgroups of k_sn_step in y) and 30 x 18; both axes
#       2^a 3^b 5^c, as the transform requires.
#   rocket: 261 x 11 (k_ry_step owns RY_ROWS = 10 rows of a 256-cell tile: a second workgroup in x whose last lane straddles the edge, a
#       second in y that owns one row) and 6 x 21 (narrower than a lane and its halo cells: both column halos are the wrap; ny = 2 * 10 + 1).
FLOW_SHAPES = dict(periodic=(516, 130), pipe=(517, 131), cavity=(517, 131), velocity_inlet=(517, 131))
POROUS_SHAPES = ((261, 9), (256, 4))
MULTIFLUID_SHAPES = ((517, 5, 3), (261, 9, 2), (6, 13, 2))
ROCKET_SHAPES = ((261, 11), (6, 21))
EXPANSION_SHAPES = ((261, 9), (37, 23))
SPECTRAL_SHAPES = ((270, 12), (30, 18))
#   advected: tests/test_gpu_advected.py's 37 x 23 (padding lanes, a ragged last block row) and 260 x 6 (a second workgroup in x, the x-wrap across
#       the tile seam), alternating with the seed, the other way round in the second family: 1 + seed % 2 scalars meet both.
ADVECTED_SHAPES = ((37, 23), (260, 6))

E_OPS = dict(
    flow=("run", "phase_step", "set_f", "init_equilibrium", "set_obstacle_mask", "clear_obstacle_mask"),
    scalar=("run", "phase_step", "set_f", "set_reaction", "set_fields", "set_edge_state"),
    multifield=("run", "phase_step", "set_f", "set_corner_state"),
    poisson=("run", "phase_step", "set_f", "set_source", "solve", "solve_reset"),
    porous=("run", "phase_step", "set_f", "set_body_force", "set_force_field", "clear_force_field", "set_porous"),
    multifluid=("run", "phase_step", "set_f", "set_body_force", "set_force_field", "clear_force_field", "set_interactions", "set_reactions"),
    rocket=("run", "phase_step", "set_f", "set_params"),
    nutrient=("run", "phase_step", "set_f", "set_params"),
    noise=("run", "phase_step", "set_f", "set_reaction", "set_fields", "set_edge_state", "set_noise", "fed_phase_step"),
    expansion=("run", "phase_step", "fed_phase_step", "set_f", "set_noise", "set_reaction", "set_fields", "set_edge_state"),
    screened=("run", "phase_step", "set_f", "redo_initial_condition", "set_reaction"),
    advected=("run", "member_run", "set_f", "init_equilibrium", "set_reaction", "set_fields"),
)
# effective ops a life makes more than once: the parameter tables of a colony, `clumpy` there and back and two more parameters, the noise
# switched off and back on (the periodic family, which has the slot that the open one gives to set_edge_state)
MORE_E = dict(rocket=("set_params",), nutrient=("set_params",) * 3, noise=("set_noise",))
_READS = ("get_fields", "hot_kernel", "plan_launches", "steps_per_launch", "layout", "sync", "checkpoint", "split_run")
T_OPS = dict(
    flow=_READS + ("check", "set_variant", "reupload_mask", "mask_off_on"),
    scalar=_READS + ("check", "set_variant"),
    multifield=_READS + ("check",),
    poisson=_READS,
    porous=_READS,
    multifluid=_READS + ("set_variant",),
    rocket=_READS + ("check", "set_variant", "get_params", "get_own"),
    nutrient=_READS + ("check", "get_own", "solver_scribble"),
    noise=_READS + ("check", "set_variant", "noise", "noise_fill"),
    expansion=_READS + ("check", "noise", "noise_fill", "get_edge_state"),
    screened=_READS + ("check", "solver_scribble"),
    advected=("get_fields", "member_fields", "hot_kernel", "sync", "checkpoint", "split_run", "check", "set_variant"),
)
STEPPING = ("run", "phase_step", "solve", "fed_phase_step", "member_run")
FIELD_NAMES = dict(
    flow=("f", "rho", "u", "v", "feq"), scalar=("f", "rho", "u", "v", "feq"), multifield=("f", "rho", "u", "v", "feq"),
    poisson=("f", "rho", "feq"),
    porous=("f", "feq", "rho", "u", "v", "u_bary", "v_bary", "Gx", "Gy"),
    multifluid=("f", "feq", "rho", "u", "v", "Gx", "Gy", "u_bary", "v_bary"),
    rocket=("f", "feq", "rho", "u", "v"), nutrient=("f", "feq", "rho", "u", "v"), noise=("f", "rho", "u", "v", "feq"),
    expansion=("f", "feq", "rho", "u", "v"), screened=("f", "rho", "u", "v", "feq"),
    advected=("f", "feq", "rho", "u", "v", "rho_flow", "f_flow", "feq_flow"),      # (the set's own get_fields; a member's: MEMBER_FIELDS)
)
MEMBER_FIELDS = ("f", "rho", "u", "v", "feq")
# what a set keeps beside its members' arrays (get_own reads them; `op` is psi in mode 'flow' and S in mode 'forces')
OWN_NAMES = dict(
    rocket=dict(flow=dict(op="psi", Fx="pseudo_force_x", Fy="pseudo_force_y"),
                forces=dict(op="S", Fx="pseudo_force_x", Fy="pseudo_force_y", Sx="surface_force_x", Sy="surface_force_y")),
    nutrient=dict(psi="psi", Fx="pseudo_force_x", Fy="pseudo_force_y"),
)


def _r32(x):
    return float(F(x))


def _rows32(*tables):
    """Tables whose every float is a float32 value, as the handle stores them: the float64 model then gets the same parameters."""
    return tuple([tuple(_r32(x) if isinstance(x, float) else x for x in row) for row in t] for t in tables)


# multifluid tables, gentle enough that two or three noisy fluids stay mixed and slow for 120 steps: every fluid is in some entry
# (the bound on G follows from the entries), all three potentials and a self term occur, couplings well below demixing
INTERACTIONS = {
    2: _rows32([(0, 1, 0.25, "linear", 0.), (0, 0, -0.1, "shan_chen", 1.)],
               [(0, 1, 0.15, "pow", 1.5), (1, 1, 0.1, "linear", 0.)],
               [(0, 1, 0.2, "shan_chen", 0.8)]),
    3: _rows32([(0, 1, 0.2, "linear", 0.), (1, 2, 0.15, "shan_chen", 0.8), (0, 0, -0.1, "shan_chen", 1.)],
               [(0, 2, 0.15, "linear", 0.), (1, 0, 0.1, "pow", 1.5), (2, 2, 0.05, "pow", 2.)],
               [(0, 1, 0.1, "shan_chen", 1.), (1, 2, 0.2, "linear", 0.), (0, 2, 0.1, "linear", 0.)]),
}
# (the windows of 'grow' and the cutoff of 'eat' lie far from every density a sequence reaches: a threshold crossed in one
#  precision and not in the other is no rounding difference)
REACTIONS = {
    2: _rows32([("grow", 0, 0.3, 3., 2e-4)], [("eat", 0, 1, 2e-4, 0.6), ("grow", 1, 0.3, 3., 1e-4)], []),
    3: _rows32([("grow", 0, 0.3, 3., 2e-4)], [("eat", 0, 1, 2e-4, 0.6), ("eat", 2, 1, 1e-4, 0.6), ("grow", 1, 0.3, 3., 3e-4)], []),
}


# colony tables: every parameter its mode reads changes between them; growth, secretion and couplings gentle enough that 120 steps keep
# the population inside (0, 1), the surfactant below 1.5 and the speed below 0.15 even in the box of six cells
ROCKET_TABLES = dict(
    flow=tuple(dict((k, _r32(v)) for k, v in t.items()) for t in (
        dict(G=0.01, G_c=0.004, epsilon=0.5, rho_o=0.9, G_chen=-0.8, c_o=0.25, alpha=2.),
        dict(G=0.005, G_c=0.002, epsilon=0.3, rho_o=1.2, G_chen=-0.5, c_o=0.25, alpha=2.),
        dict(G=0., G_c=0.006, epsilon=0.4, rho_o=0.9, G_chen=0.4, c_o=0.25, alpha=2.))),
    forces=tuple(dict((k, _r32(v)) for k, v in t.items()) for t in (
        dict(G=0.01, G_c=0.004, epsilon=0.5, rho_o=0.9, G_chen=-0.8, c_o=0.25, alpha=2.),
        dict(G=0.005, G_c=0.002, epsilon=0.3, rho_o=0.7, G_chen=0.5, c_o=0.4, alpha=1.5),
        dict(G=0., G_c=0.006, epsilon=-0.4, rho_o=0.9, G_chen=-0.4, c_o=0.3, alpha=1.))),
)
ROCKET_OMEGAS = (F(0.8), F(1.1))
# a population and its nutrient: the values set_params deals (the first of each is the one a life starts with)
NUTRIENT_VALUES = dict(G=(0.01, 0.02, 0.), scale=(-0.05, -0.03, 0.), G_chen=(-1., -0.6, 0.5), rho_o=(1., 0.8))
NUTRIENT_OMEGAS, NUTRIENT_LAM, NUTRIENT_DX = (F(0.8), F(1.25)), 1., 0.1
# noisy strains (tests/test_gpu_expansion.py's OMEGAS, GS, DGS: its fixtures keep every density above twice the cutoff for 50 steps)
EX_OMEGAS, EX_OMEGA_N, EX_GS, EX_DGS, EX_CUT = (1.1, 0.9, 1.25), 1.3, (0.01, 0.014, 0.012), (2.0e-3, 1.0e-3, 5.0e-4), 0.01
NOISE_DGS = (1e-4, 2e-4, 5e-5)                  # (tests/test_gpu_noise.py's case: a hundred steps inside (0, 1) at 1e-4)


def variant_words(kind):
    from LB_D2Q9.variants import (AUTO, K_DEEP2, K_DEEP6, K_DEEP7, K_STEP, K_STEP2, K_STEP3, K_STEP4, K_STEP5, K_TILE4, NT_STORES, ROWS_2,
                                  TILES, XCD_ORDER)
    if kind == "flow":
        return (AUTO, K_STEP, K_STEP2, K_STEP3, K_STEP4, K_STEP5, K_DEEP6, K_DEEP7, K_DEEP2, K_TILE4, NT_STORES | ROWS_2, XCD_ORDER)
    if kind == "scalar":
        return (AUTO, K_STEP, TILES | 1 << 2, TILES | 2 << 2, TILES | 3 << 2)
    if kind == "noise":                             # (the scalar kind's, and both noise plans of k_ad_tile4)
        from LB_D2Q9.variants import STEP4_NO_AHEAD
        return (AUTO, K_STEP, TILES | 1 << 2, TILES | 2 << 2, TILES | 3 << 2, TILES | STEP4_NO_AHEAD, TILES | 2 << 2 | STEP4_NO_AHEAD)
    if kind in ("multifluid", "rocket"):
        return (-1, 0, 1)
    if kind == "advected":
        return tuple(sorted(set(sum(advected_words(), ()))))
    return ()


def advected_words():
    """(the flow's words in front of a set run, the flow's in front of a run of its own, a scalar's in front of a run of its own).  The
    first: what flow_step_macro (form 0) takes from the flow handle's word -- the block shape, the non-temporal bits -- and a marching
    word it must not act on; the second: the marching words and the tiles, which these shapes decline; the third: the three tile shapes
    of k_ad_tile4."""
    from LB_D2Q9.variants import (K_DEEP2, K_DEEP6, K_DEEP7, K_STEP2, K_STEP3, K_STEP4, K_STEP5, K_TILE4, NT_LOADS, NT_STORES, ROWS_1, ROWS_2,
                                  TILES)
    return ((ROWS_1, ROWS_2, NT_STORES | NT_LOADS, K_DEEP7), (K_STEP2, K_STEP3, K_STEP4, K_STEP5, K_DEEP6, K_DEEP2, K_TILE4),
            (TILES | 1 << 2, TILES | 2 << 2, TILES | 3 << 2))


def _key(kind, family, seed):
    return [KINDS.index(kind), FAMILIES[kind].index(family), int(seed)]


# ---- the case: what a player is built from -------------------------------------------------------------------------------------------
def case_of(kind, family, seed):
    """Sizes, parameters and the initial state of (kind, family, seed), as a dict; arrays float32."""
    rng = np.random.default_rng(_key(kind, family, seed) + [1])
    c = dict(kind=kind, family=family, seed=int(seed))
    if kind == "flow":
        bc = family.split("-")[0]
        c.update(bc=bc, eager=family.endswith("-eager"), omega=_r32(rng.uniform(0.8, 1.6)), inlet_rho=1., lid_u=0., inlet_u=0., outlet_u=0.)
        c["nx"], c["ny"] = FLOW_SHAPES[bc]
        if bc == "pipe":
            c["inlet_rho"] = _r32(1. + rng.uniform(0.002, 0.01))
        if bc == "cavity":
            c["lid_u"] = _r32(rng.uniform(0.02, 0.08))
        if bc == "velocity_inlet":
            c["inlet_u"], c["outlet_u"] = 0.03, 0.028
            c["u0"], c["v0"] = (0.01 * rng.standard_normal((2, c["nx"], c["ny"]))).astype(F)
        c["mask"] = payload(c, "set_obstacle_mask", 1000) if starts_masked(family, seed) else None
    elif kind == "scalar":
        c.update(nx=130, ny=50, bc=family, omega=_r32(rng.uniform(0.8, 1.6)), G=(0., 0.01)[int(rng.integers(0, 2))])
        c["u"], c["v"] = payload(c, "set_fields", 1000)
    elif kind == "multifield":
        c.update(nx=258, ny=9, bc=family, nf=3, omegas=(F(0.9), F(1.3), F(1.1)), Gs=(F(0.02), F(0.01), F(0.015)))
        c["u"], c["v"] = payload(c, "set_fields", 1000)
    elif kind == "poisson":
        c.update(nx=261, ny=9, omega=_r32(rng.uniform(0.6, 1.4)), rho_on_boundary=_r32(0.3), react_factor=_r32(0.5))
        c["source"] = payload(c, "set_source", 1000)
    elif kind == "porous":
        c["nx"], c["ny"] = POROUS_SHAPES[seed % 2]
        c.update(bc=family, omega=_r32(rng.uniform(0.8, 1.5)), porous=payload(c, "set_porous", 1000), g=(_r32(2e-3), _r32(-1e-3)))
    elif kind == "multifluid":
        c["nx"], c["ny"], c["nf"] = MULTIFLUID_SHAPES[seed % 3]
        c.update(bc=family, omegas=(F(1.25), F(0.9), F(1.05))[:c["nf"]], rhos=(1., 0.9, 0.8)[:c["nf"]],
                 g=((_r32(2e-3), _r32(-1e-3)), (0., _r32(1e-3)), (_r32(-1e-3), 0.))[:c["nf"]], interactions=seed % 3, reactions=(seed + 1) % 3)          # (the tables it starts with: indices into INTERACTIONS, REACTIONS)
    elif kind == "rocket":
        c["nx"], c["ny"] = ROCKET_SHAPES[seed % 2]
        c.update(mode=family, omegas=ROCKET_OMEGAS, table=seed % 3)                   # (the table it starts with: an index into ROCKET_TABLES)
    elif kind == "nutrient":
        c["nx"], c["ny"] = SPECTRAL_SHAPES[seed % 2]
        c.update(omegas=NUTRIENT_OMEGAS, lam=NUTRIENT_LAM, dx=NUTRIENT_DX, clumpy=family == "clumpy",
                 params={k: _r32(v[0]) for k, v in NUTRIENT_VALUES.items()})
    elif kind == "noise":
        c.update(nx=130, ny=50, bc=family, omega=_r32(rng.uniform(0.8, 1.6)), G=(0., 0.01)[int(rng.integers(0, 2))], Dg=_r32(NOISE_DGS[0]),
                 noise_seed=int(rng.integers(1, 1 << 62)))
        c["u"], c["v"] = payload(c, "set_fields", 1000)
    elif kind == "expansion":
        c["nx"], c["ny"] = EXPANSION_SHAPES[seed % 2]
        n = _nf(kind, seed)
        c.update(bc=family, ns=n, omegas=tuple(F(o) for o in EX_OMEGAS[:n]), omega_n=F(EX_OMEGA_N), Gs=tuple(_r32(g) for g in EX_GS[:n]),
                 Dgs=tuple(_r32(d) for d in EX_DGS[:n]), cut=_r32(EX_CUT), noise_seed=int(rng.integers(1, 1 << 62)))
        c["u"], c["v"] = payload(c, "set_fields", 1000)
    elif kind == "screened":
        c["nx"], c["ny"] = SPECTRAL_SHAPES[seed % 2]
        # (spectral_model.fisher_lattice_parameters at N = 10: omega = 0.8, G = 0.01, scale = -0.1; a gentler scale keeps |u| < 0.15)
        c.update(bc=family, omega=_r32(0.8), G=0.01, lam=1., dx=0.1, scale=_r32(-rng.uniform(0.04, 0.07)))
        c["rho0"] = payload(c, "redo_initial_condition", 1000)
    elif kind == "advected":
        fi = FAMILIES[kind].index(family)
        c["nx"], c["ny"] = nx, ny = ADVECTED_SHAPES[(seed + fi) % 2]
        ns = 1 + seed % 2
        c.update(ns=ns, eager=family == "eager", planar_flow=bool(rng.integers(0, 2)), planar_scalars=bool(rng.integers(0, 2)),
                 omega=_r32(rng.uniform(1.0, 1.6)), omegas=ADVECTED_OMEGAS[:ns], Gs=advected_rates(family, seed)[0])
        # tests/test_gpu_advected.py's start with the case's own draws: a shear layer with a transverse kick (|u| <= 0.05), a striped dye
        # per scalar, every population perturbed
        x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        c["u"] = (0.04 * np.tanh((y - 0.5 * ny + 0.5) / max(ny / 8., 1.))).astype(F)
        c["v"] = (0.01 * np.sin(2 * np.pi * (x + 0.5) / nx)).astype(F)
        assert float(np.max(np.hypot(c["u"], c["v"]))) <= 0.05
        c["rho"] = np.ones((nx, ny), F)
        # (stripes of 0.25 and 0.55: at omega = 1.6 a step of the dye overshoots by a third of its height in the first steps, and a growing
        #  dye must stay below 1 for MAX_STEPS steps)
        c["dyes"] = [((0.4 + 0.15 * np.sign(np.sin(2 * np.pi * (x + 2 * i) / max(nx / 3., 2.)))).astype(F),
                      (1 + 0.01 * rng.standard_normal((nx, ny, 9))).astype(F)) for i in range(ns)]
        c["f0"] = (1 + 0.01 * rng.standard_normal((nx, ny, 9))).astype(F)      # (here: the factors on the flow's first equilibrium)
        return c
    else:
        raise ValueError(kind)
    c["f0"] = payload(c, "set_f", 1000)
    return c


# a flow and the scalars it carries: the scalars' rates as in tests/test_gpu_advected.py; growth switched between 0 and ADVECTED_G, gentle
# enough that a dye of 0.2 ... 0.8 stays inside (0, 1) for MAX_STEPS steps (tests/test_sequences_cpu.py holds that and prints the margin)
ADVECTED_OMEGAS, ADVECTED_G = (F(1.6), F(1.1)), 0.01


def advected_rates(family, seed):
    """(the growth rate every scalar starts with, the scalar whose rate set_reaction switches -- to the other of 0 and ADVECTED_G,
    between the life's first and second set run, and back between the second and the third).  Over the seeds every scalar starts both
    ways; with two scalars the other one has either rate."""
    fi, ns = FAMILIES["advected"].index(family), 1 + seed % 2
    who = (seed // 2) % ns
    gs = [_r32(ADVECTED_G) if (seed // 2 + fi + i) % 2 else 0. for i in range(ns)]
    gs[who] = _r32(ADVECTED_G) if (seed + fi) % 2 else 0.
    return tuple(gs), who


def payload(c, name, pseed, who=None):
    """The array(s) of op `name` with payload seed `pseed` on case c; who: the member of a set of unlike lattices (-1: the flow)."""
    kind, nx, ny = c["kind"], c["nx"], c["ny"]
    rng = np.random.default_rng(_key(kind, c["family"], c["seed"]) + [2, int(pseed)])
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    phase = rng.uniform(0., 2. * np.pi, 2)
    wave = lambda p: np.sin(2. * np.pi * y / ny + p[0]) * np.cos(2. * np.pi * x / nx + p[1])
    if name == "set_f":
        if kind == "advected" and who == -1:        # the flow kind's
            return (W64 * (1. + 0.02 * rng.standard_normal((nx, ny, 9)))).astype(F)
        if kind == "advected":                      # the noise kind's blob: rho 0.15 ... 0.75 grows for 120 steps inside (0, 1)
            rho = 0.15 + 0.6 * np.exp(-(((x - rng.uniform(0.3, 0.7) * nx) / (0.2 * nx)) ** 2 + ((y - 0.5 * ny) / (0.25 * ny)) ** 2))
            return (W64 * rho[:, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(F)
        if kind == "flow":
            return (W64 * (1. + 0.02 * rng.standard_normal((nx, ny, 9)))).astype(F)
        if kind == "scalar":
            rho = 0.2 + 0.7 * np.exp(-(((x - rng.uniform(0.3, 0.7) * nx) / (0.2 * nx)) ** 2 + ((y - 0.5 * ny) / (0.25 * ny)) ** 2))
            return (W64 * rho[:, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(F)
        if kind == "multifield":
            f = np.zeros((nx, ny, c["nf"], 9), F)
            for i in range(c["nf"]):
                rho = 0.03 + (0.7 / c["nf"]) * np.exp(-(((x - rng.uniform(0.2, 0.8) * nx) / (0.3 * nx)) ** 2 + ((y - 0.5 * ny) / (0.35 * ny)) ** 2))
                f[:, :, i, :] = W64 * rho[:, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))
            return f
        if kind == "poisson":
            return (W64 * 0.3 * (1. + 0.2 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(F)
        if kind == "porous":
            return (W64 * (1. + 0.1 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(F)
        if kind == "multifluid":
            return (W64 * np.asarray(c["rhos"])[None, None, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, c["nf"], 9)))).astype(F)
        if kind == "rocket":                        # a few long waves of random phase: the population in 0.3 ... 0.9, the surfactant around 0.5
            long_waves = lambda: sum(a * np.sin(2. * np.pi * (kx * x / nx + ky * y / ny) + rng.uniform(0., 2. * np.pi))
                                     for a, kx, ky in ((0.12, 1, 0), (0.1, 0, 1), (0.06, 1, 1)))
            rho = np.stack([0.6 + long_waves(), 0.5 + long_waves()], axis=2)
            return (W64 * rho[:, :, :, None] * (1. + 0.02 * rng.uniform(-1., 1., (nx, ny, 2, 9)))).astype(F)
        if kind == "nutrient":                      # a droplet of the population somewhere in the box on a gently waved nutrient
            cx, cy, r = rng.uniform(0.2, 0.8) * nx, rng.uniform(0.3, 0.7) * ny, 0.5 * max(nx, ny) / 3.
            rho = np.stack([0.05 + 0.8 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / r ** 2), 0.9 + 0.1 * wave(phase)], axis=2)
            return (W64 * rho[:, :, :, None] * (1. + 0.02 * rng.uniform(-1., 1., (nx, ny, 2, 9)))).astype(F)
        if kind == "noise":                         # the scalar kind's blob, lower: rho 0.15 ... 0.75 grows and is kicked for 120 steps inside (0, 1)
            rho = 0.15 + 0.6 * np.exp(-(((x - rng.uniform(0.3, 0.7) * nx) / (0.2 * nx)) ** 2 + ((y - 0.5 * ny) / (0.25 * ny)) ** 2))
            return (W64 * rho[:, :, None] * (1. + 0.05 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(F)
        if kind == "expansion":                     # test_gpu_expansion.smooth_case with random phases: strains 0.15 ... 0.55, the nutrient 0.7 ... 1
            f = np.zeros((nx, ny, c["ns"] + 1, 9), F)
            for i in range(c["ns"] + 1):
                p = rng.uniform(0., 1., 2)
                bump = 0.5 + 0.5 * np.sin(2. * np.pi * (x / nx + p[0])) * np.cos(2. * np.pi * (y / ny - p[1]))
                rho = 0.7 + 0.3 * bump if i == c["ns"] else 0.15 + 0.4 * bump
                f[:, :, i, :] = W64 * rho[:, :, None] * (1. + 0.02 * rng.uniform(-1., 1., (nx, ny, 9)))
            return f
        if kind == "screened":
            return (W64 * _droplet(rng, x, y, nx, ny)[:, :, None] * (1. + 0.02 * rng.uniform(-1., 1., (nx, ny, 9)))).astype(F)
    if name == "redo_initial_condition":            # the density a wave starts again from
        return _droplet(rng, x, y, nx, ny).astype(F)
    if name == "solver_scribble":                   # an unrelated charge
        return (rng.standard_normal((nx, ny)) + 1j * rng.standard_normal((nx, ny))).astype(np.complex64)
    if name == "fed_phase_step":                    # the normals of one collision: one field per strain
        return rng.standard_normal((nx, ny) if kind == "noise" else (nx, ny, c["ns"])).astype(F)
    if kind == "expansion" and name == "set_fields":                 # (smooth_case's 0.05)
        return (0.05 * wave(phase)).astype(F), (-0.05 * wave(phase[::-1])).astype(F)
    # (where a collision floors its links at 0, entering links are those of a density a sequence reaches, w_k rho: an over-relaxed link
    #  far above its equilibrium would be floored in the next collision)
    if kind == "noise" and name == "set_edge_state":
        return _edge_links(rng, nx, ny, 0.12, 0.22)              # (the blob's density at the edges is 0.15; omega reaches 1.6)
    if kind == "expansion" and name == "set_edge_state":             # one row per member, the nutrient last
        return np.stack([_edge_links(rng, nx, ny, *((0.15, 0.5) if i < c["ns"] else (0.7, 1.))) for i in range(c["ns"] + 1)])
    if name == "init_equilibrium":
        rho = 1. + 0.02 * wave(phase) + 0.002 * rng.standard_normal((nx, ny))
        u = 0.03 * wave(phase[::-1]) + 0.002 * rng.standard_normal((nx, ny))
        v = -0.03 * wave(phase + 1.) + 0.002 * rng.standard_normal((nx, ny))
        return rho.astype(F), u.astype(F), v.astype(F)
    if name == "set_obstacle_mask":
        m = rng.random((nx, ny)) < 0.03
        m[0, :] = m[-1, :] = False                  # the border stays clear: obstacles on it have their own file
        m[:, 0] = m[:, -1] = False
        return m
    if name == "set_fields":                        # a scalar lattice's imposed velocity
        return (0.06 * wave(phase)).astype(F), (-0.06 * wave(phase[::-1])).astype(F)
    if name == "set_edge_state":
        return rng.uniform(0., 0.04, 6 * (nx + ny)).astype(F)
    if name == "set_corner_state":
        shape = (c["nf"], 8) if kind == "multifield" else (8,)
        return rng.uniform(0., 0.02, shape).astype(F)
    if name == "set_source":
        return (0.002 * rng.uniform(size=(nx, ny))).astype(F)
    if name == "set_force_field":
        return tuple((1e-3 * rng.uniform(-1., 1., (2, nx, ny))).astype(F))
    if name == "set_porous":                        # epsilon, nu_fluid, K, Fe
        return (_r32(rng.uniform(0.5, 0.9)), _r32(rng.uniform(0.1, 0.2)), _r32(rng.uniform(5., 30.)), (0., _r32(rng.uniform(0.1, 0.5)))[int(rng.integers(0, 2))])
    raise ValueError((kind, name))


def _edge_links(rng, nx, ny, lo, hi):
    """An edge state (include/lb_hip.h: west k = 1, 5, 8, east 3, 6, 7 of ny links each, south 2, 5, 6, north 4, 7, 8 of nx each) of links
    w_k rho with rho uniform in lo ... hi."""
    return np.concatenate([W64[k] * rng.uniform(lo, hi, n) for n, ks in ((ny, (1, 5, 8, 3, 6, 7)), (nx, (2, 5, 6, 4, 7, 8))) for k in ks]).astype(F)


def _droplet(rng, x, y, nx, ny):
    """A Gaussian droplet (spectral_model.noisy_droplet's, R0 = 0.5 at N = max(nx, ny) / 3) of random height and place, 5 % noise."""
    cx, cy, r = rng.uniform(0.3, 0.7) * nx, rng.uniform(0.3, 0.7) * ny, 0.5 * max(nx, ny) / 3.
    rho = rng.uniform(0.6, 0.9) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / r ** 2)
    return rho * (1. + 0.05 * rng.standard_normal((nx, ny)))


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
def generate(kind, family, seed):
    """The op list of (kind, family, seed): at most MAX_E effective and MAX_T transparent ops, at most MAX_STEPS steps, a stepping
    op last.  Every effective op of the kind that the family has occurs once, runs fill the rest."""
    if kind == "advected":
        return _generate_advected(family, seed)
    rng = np.random.default_rng(_key(kind, family, seed) + [3])
    names = [n for n in E_OPS[kind] if not (n == "set_edge_state" and family != "open")]
    if not (kind == "noise" and family == "open"):
        names += MORE_E.get(kind, ())
    names += ["run"] * (MAX_E - 1 - len(names))
    rng.shuffle(names)
    names.append("run")
    steps_left, pseed, ops = STEP_CAP.get(kind, MAX_STEPS), 0, []
    state = dict(table=seed % 3, react=(seed + 1) % 3)          # (as case_of)
    state.update(noisy=True, clumpy=family == "clumpy", toggles=0, dealt={k: 0 for k in NUTRIENT_VALUES})

    # run lengths are dealt from one deck per kind, so that the committed seeds of a kind cover every length
    deck = [int(n) for n in np.random.default_rng([KINDS.index(kind), 5]).permutation(RUN_LENGTHS)]
    dealt = [(FAMILIES[kind].index(family) * len(SEEDS) + int(seed)) * sum(n in ("run", "solve") for n in names)]

    def length(keep):
        n = deck[dealt[0] % len(deck)]
        dealt[0] += 1
        return n if n <= steps_left - keep else max([m for m in RUN_LENGTHS if m <= steps_left - keep] or [1])

    for i, name in enumerate(names):
        pseed += 1
        last = i == len(names) - 1
        if name in ("run", "solve"):
            n = length(0 if last else 1)                                 # (one step is kept for the last op)
            steps_left -= n
            ops.append((name, n, 0) if name == "run" else (name, n))
        elif name == "phase_step":
            steps_left -= 1
            ops.append((name,))
        elif name == "fed_phase_step":
            steps_left -= 1
            ops.append((name, pseed))
        elif name in ("set_f", "init_equilibrium", "set_obstacle_mask", "set_fields", "set_edge_state", "set_corner_state", "set_source",
                      "redo_initial_condition"):
            ops.append((name, pseed))
        elif name in ("clear_obstacle_mask", "solve_reset"):
            ops.append((name,))
        elif name == "set_reaction" and kind == "expansion":            # one strain's growth rate
            ops.append((name, int(rng.integers(0, _nf(kind, seed))), _r32((0.006, 0.016, 0.)[int(rng.integers(0, 3))])))
        elif name == "set_reaction":
            ops.append((name, "toggle"))
        elif name == "set_params" and kind == "rocket":
            state["table"] = (state["table"] + int(rng.integers(1, 3))) % 3
            ops.append((name, state["table"]))
        elif name == "set_params":                                      # nutrient: `clumpy` the other way, then the next value of a parameter, in turns
            state["toggles"] += 1
            if state["toggles"] % 2:
                state["clumpy"] = not state["clumpy"]
                ops.append((name, "clumpy", state["clumpy"]))
            else:
                k = str(rng.choice(sorted(NUTRIENT_VALUES)))
                state["dealt"][k] += 1
                ops.append((name, k, _r32(NUTRIENT_VALUES[k][state["dealt"][k] % len(NUTRIENT_VALUES[k])])))
        elif name == "set_noise" and kind == "noise":                   # off where the family has a second call to switch it on again, or the seed is odd
            nseed = int(rng.integers(1, 1 << 62))
            off = state["noisy"] and (family == "periodic" or seed % 2 == 1)
            state["noisy"] = not off
            ops.append((name, 0. if off else _r32(NOISE_DGS[int(rng.integers(0, len(NOISE_DGS)))]), nseed))
        elif name == "set_noise":                                       # expansion: the strengths dealt anew, every other time one strain without noise
            n = _nf(kind, seed)
            dgs = [_r32(d) for d in rng.permutation(EX_DGS)[:n]]
            if rng.integers(0, 2):
                dgs[int(rng.integers(0, n))] = 0.
            ops.append((name, tuple(dgs), int(rng.integers(1, 1 << 62))))
        elif name == "set_porous":
            ops.append((name, pseed))
        elif name == "set_body_force":
            g = (_r32(rng.uniform(-2e-3, 2e-3)), _r32(rng.uniform(-2e-3, 2e-3)))
            ops.append((name,) + g if kind == "porous" else (name, int(rng.integers(0, _nf(kind, seed)))) + g)
        elif name == "set_force_field":
            ops.append((name, pseed) if kind == "porous" else (name, int(rng.integers(0, _nf(kind, seed))), pseed))
        elif name == "clear_force_field":
            ops.append((name,) if kind == "porous" else (name, int(rng.integers(0, _nf(kind, seed)))))
        elif name == "set_interactions":
            state["table"] = (state["table"] + int(rng.integers(1, 3))) % 3
            ops.append((name, state["table"]))
        elif name == "set_reactions":
            state["react"] = (state["react"] + int(rng.integers(1, 3))) % 3
            ops.append((name, state["react"]))
        else:
            raise ValueError(name)
    assert steps_left >= 0 and len(ops) <= MAX_E

    runs = [i for i, op in enumerate(ops) if op[0] == "run" and op[1] >= 2]
    if runs:                                        # split_run: one run made in two calls, the first un-waited
        i = int(rng.choice(runs))
        ops[i] = ("run", ops[i][1], int(rng.integers(1, ops[i][1])))

    # the variant words: each directly in front of a run of its own, so that every word selects something; runs of at least
    # VARIANT_DEPTH steps in one call first (the deepest marching kernels take seven steps a launch), and the words in front of those
    # dealt from a deck per kind, so that the committed seeds put every word in front of such a run
    words = variant_words(kind)
    variants = {}
    if words:
        deep = [i for i, op in enumerate(ops) if op[0] == "run" and max(op[2], op[1] - op[2]) >= VARIANT_DEPTH]
        flat = [i for i, op in enumerate(ops) if op[0] == "run" and i not in deep]
        rng.shuffle(deep)
        rng.shuffle(flat)
        word_deck = [int(w) for w in np.random.default_rng([KINDS.index(kind), 7]).permutation(words)]
        sequence = FAMILIES[kind].index(family) * len(SEEDS) + int(seed)
        for k, i in enumerate((deep + flat)[:N_VARIANTS]):
            variants[i] = word_deck[(sequence + k * (len(words) // 2)) % len(words)] if i in deep else int(rng.choice(words))

    # the other transparent ops: each of the kind's once, then more reads and a second checkpoint, shuffled, each at a random place in
    # front of an effective op (never behind the last op: the final comparison follows it).  The first read of a list lies behind
    # a stepping op, the mask is uploaded again and taken off and on where a mask is set.
    t_names = [n for n in T_OPS[kind] if n not in ("split_run", "set_variant")]
    t_names = (t_names + ["get_fields", "get_fields", "checkpoint"])[:MAX_T - 1 - len(variants)]
    rng.shuffle(t_names)
    first_step = min(i for i, op in enumerate(ops) if op[0] in STEPPING)
    masked, has_mask = [], kind == "flow" and starts_masked(family, seed)
    for i, op in enumerate(ops):                    # (place i: in front of op i)
        if has_mask:
            masked.append(i)
        has_mask = op[0] == "set_obstacle_mask" or (has_mask and op[0] != "clear_obstacle_mask")
    t_ops, where = [], []
    for name in t_names:
        if name == "get_fields":
            k = int(rng.integers(1, len(FIELD_NAMES[kind]) + 1))
            which = tuple(sorted(str(s) for s in rng.choice(FIELD_NAMES[kind], size=k, replace=False)))
            t_ops.append((name, which + ("feq",) if "feq" not in which and rng.integers(0, 2) else which))
        elif name == "plan_launches":
            t_ops.append((name, int(rng.choice(RUN_LENGTHS))))
        elif name == "noise_fill":                  # (a counter; on a set: a strain and a counter)
            t_ops.append((name, int(rng.integers(0, 1000))) if kind == "noise" else (name, int(rng.integers(0, _nf(kind, seed))), int(rng.integers(0, 1000))))
        elif name == "solver_scribble":             # (a payload seed)
            t_ops.append((name, 2000 + len(t_ops)))
        else:
            t_ops.append((name,))
        if name in ("reupload_mask", "mask_off_on"):
            where.append(int(rng.choice(masked)))
        elif name == "get_fields" and "get_fields" not in [t[0] for t in t_ops[:-1]]:
            where.append(int(rng.integers(first_step + 1, len(ops))))
        else:
            where.append(int(rng.integers(0, len(ops))))
    out = []
    for i, op in enumerate(ops):
        out += [t for t, p in zip(t_ops, where) if p == i]
        if i in variants:                           # (last: a handle restored from a checkpoint chooses its kernel anew)
            out.append(("set_variant", variants[i]))
        out.append(op)
    return out


ADVECTED_FLOW_RUNS = (17, 33, 40)                  # a flow run of its own: longer than the 16 steps of the captured graph
ADVECTED_SCALAR_RUNS = ((1, 2, 3, 5), (8, 13, 16))  # a scalar's: short, or at least VARIANT_DEPTH steps behind a tile word


def _generate_advected(family, seed):
    """The life of a flow and the 1 + seed % 2 scalars it carries.  Ten effective ops: three runs of the set, the last one last; between
    the first and the second, and between the second and the third, set_reaction switches one scalar's growth rate to the other of 0 and
    ADVECTED_G and back (advected_rates); at random places around them a run of the flow alone (ADVECTED_FLOW_RUNS), set_fields on a
    scalar with that scalar's own run directly behind it -- the next set run replaces the velocity --, set_f on one member,
    init_equilibrium on the flow.  Ops: ('run', n, split, form) -- split and form are the subject's alone --, ('member_run', n, 0, who),
    ('set_f', payload seed, who), ('init_equilibrium', payload seed), ('set_reaction', who, G), ('set_fields', payload seed, who); who:
    -1 the flow, else the scalar.  Two variant words: one of the flow's in front of its own run; the other either one of the flow's in
    front of the longest set run, at least VARIANT_DEPTH steps in one call and of form 0, which alone reads the word, or a tile shape on
    the scalar in front of its own run.  The other transparent ops as in generate(): get_fields is the set's own, member_fields reads
    every member."""
    kind = "advected"
    fi, seed = FAMILIES[kind].index(family), int(seed)
    rng = np.random.default_rng(_key(kind, family, seed) + [3])
    sequence, ns = fi * len(SEEDS) + seed, 1 + seed % 2
    gs, who = advected_rates(family, seed)
    set_words, own_words, scalar_words = advected_words()
    scalar_word = (seed // 2 + fi) % 2 == 1
    turn = (sequence // 4) * 2 + sequence % 2       # 0 ... 5 among the six lives with either kind of second word

    fl_len = ADVECTED_FLOW_RUNS[sequence % len(ADVECTED_FLOW_RUNS)]
    sc_len = ADVECTED_SCALAR_RUNS[1][turn % 3] if scalar_word else int(rng.choice(ADVECTED_SCALAR_RUNS[0]))
    steps_left = MAX_STEPS - fl_len - sc_len
    deck = [int(n) for n in np.random.default_rng([KINDS.index(kind), 5]).permutation(RUN_LENGTHS)]
    lengths = []
    for k in range(3):                              # (one step is kept for every set run still to come)
        n, room = deck[(3 * sequence + k) % len(deck)], steps_left - (2 - k)
        n = n if n <= room else max(m for m in RUN_LENGTHS if m <= room)
        lengths.append(n)
        steps_left -= n
    if not scalar_word and max(lengths) < VARIANT_DEPTH:
        steps_left -= VARIANT_DEPTH - max(lengths)
        lengths[lengths.index(max(lengths))] = VARIANT_DEPTH
    assert steps_left >= 0
    word_run = None if scalar_word else lengths.index(max(lengths))
    forms = [0 if k == word_run else (-1, 0, 1)[(sequence + k) % 3] for k in range(3)]

    pseed = iter(range(1, 100))
    sc_who = int(rng.integers(0, ns))
    members = [-1] + list(range(ns))
    other = ADVECTED_G if gs[who] == 0. else 0.
    blocks = dict(FL=[("member_run", fl_len, 0, -1)], SC=[("set_fields", next(pseed), sc_who), ("member_run", sc_len, 0, sc_who)],
                  SF=[("set_f", next(pseed), members[(sequence // 2) % len(members)])], IE=[("init_equilibrium", next(pseed))],
                  SR1=[("set_reaction", who, _r32(other))], SR2=[("set_reaction", who, gs[who])])
    gaps = [[], ["SR1"], ["SR2"]]                   # in front of the first set run, of the second, of the third
    for name in ("FL", "SC", "SF", "IE"):
        gaps[int(rng.integers(0, 3))].append(name)
    ops, run_at = [], []
    for k, gap in enumerate(gaps):
        for j in rng.permutation(len(gap)):
            ops += blocks[gap[int(j)]]
        run_at.append(len(ops))
        ops.append(("run", lengths[k], 0, forms[k]))
    assert len(ops) == MAX_E

    splittable = [i for k, i in enumerate(run_at) if lengths[k] >= 2 and k != word_run]
    if splittable:
        i = int(rng.choice(splittable))
        ops[i] = ("run", ops[i][1], int(rng.integers(1, ops[i][1])), ops[i][3])

    variants = {ops.index(blocks["FL"][0]): (int(own_words[sequence % len(own_words)]), -1)}
    if scalar_word:
        variants[ops.index(blocks["SC"][1])] = (int(scalar_words[turn % len(scalar_words)]), sc_who)
    else:
        variants[run_at[word_run]] = (int(set_words[turn % len(set_words)]), -1)

    t_names = [n for n in T_OPS[kind] if n not in ("split_run", "set_variant")]
    t_names = (t_names + ["get_fields", "member_fields", "checkpoint"])[:MAX_T - 1 - len(variants)]
    rng.shuffle(t_names)
    first_step = min(i for i, op in enumerate(ops) if op[0] in STEPPING)
    t_ops, where = [], []
    for name in t_names:
        if name in ("get_fields", "member_fields"):
            names = FIELD_NAMES[kind] if name == "get_fields" else MEMBER_FIELDS
            k = int(rng.integers(1, len(names) + 1))
            which = tuple(sorted(str(s) for s in rng.choice(names, size=k, replace=False)))
            t_ops.append((name, which + ("feq",) if "feq" not in which and rng.integers(0, 2) else which))
        else:
            t_ops.append((name,))
        if name == "get_fields" and "get_fields" not in [t[0] for t in t_ops[:-1]]:
            where.append(int(rng.integers(first_step + 1, len(ops))))
        else:
            where.append(int(rng.integers(0, len(ops))))
    out = []
    for i, op in enumerate(ops):
        out += [t for t, p in zip(t_ops, where) if p == i]
        if i in variants:                           # (last: a set restored from a checkpoint has fresh handles, which choose anew)
            out.append(("set_variant",) + variants[i])
        out.append(op)
    return out


def starts_masked(family, seed):
    """Whether the flow case (family, seed) starts with an obstacle mask."""
    return bool(np.random.default_rng(_key("flow", family, seed) + [6]).integers(0, 2))


def _nf(kind, seed):
    if kind == "expansion":                         # (the strains: every count the engine builds)
        return 1 + seed % 3
    return MULTIFLUID_SHAPES[seed % 3][2] if kind == "multifluid" else 1


_EFFECTIVE = frozenset(sum(E_OPS.values(), ()))


def is_effective(op):
    return op[0] in _EFFECTIVE


def cut_points(ops, kind, family, seed):
    """Indices into ops behind which the players are compared: two inside the list and the last op.  Inside: behind a stepping op,
    where every array is fresh, or -- two times in three where the list has one -- behind a set_f that follows a stepping op, where
    the populations are new and rho, u, v, feq and the forces are still those of the step before, as in the reference."""
    rng = np.random.default_rng(_key(kind, family, seed) + [4])
    inner = [i for i, op in enumerate(ops[:-1]) if op[0] in STEPPING]
    effective = [i for i, op in enumerate(ops) if is_effective(op)]
    behind_step = [i for a, i in zip(effective, effective[1:]) if ops[i][0] == "set_f" and ops[a][0] in STEPPING]
    picked = []
    if behind_step and rng.random() < 2. / 3.:
        picked.append(int(rng.choice(behind_step)))
    phases = [i for i in inner if ops[i][0] == "phase_step"]
    if phases and rng.random() < 0.5:               # (the one step by phases of a list: every other time)
        picked.append(int(rng.choice(phases)))
    rest = [i for i in inner if i not in picked]
    picked += [int(i) for i in rng.choice(rest, size=min(2 - len(picked), len(rest)), replace=False)]
    return sorted(picked) + [len(ops) - 1]


def counts(ops):
    """(effective ops, transparent ops -- a split run counts as one --, steps)"""
    e = [op for op in ops if is_effective(op)]
    t = len(ops) - len(e) + sum(1 for op in e if op[0] == "run" and op[2])
    steps = sum(op[1] if op[0] in ("run", "solve", "member_run") else 1 for op in e if op[0] in STEPPING)
    return len(e), t, steps


# ---- the players ---------------------------------------------------------------------------------------------------------------------------
class Player(object):
    """What the driver needs of a player: the effective ops by name, fields() for the contract, `steps` since the populations were
    set and `macro_steps`, the steps behind rho, u, v, feq and the forces (set_f leaves those as the last step made them)."""

    def __init__(self, case):
        self.case, self.kind = case, case["kind"]
        self.steps = self.macro_steps = 0
        self.G = case.get("G", 0.)

    def effective(self, op):
        name = op[0]
        if name in STEPPING:
            if name == "run":
                self.run(op[1], op[2])
            elif name == "solve":
                self.solve(op[1])
            elif name == "fed_phase_step":
                self.fed_phase_step(payload(self.case, name, op[1]))
            else:
                self.phase_step()
            self.steps += op[1] if name in ("run", "solve") else 1
            self.macro_steps = self.steps
        else:
            if name in ("set_f", "init_equilibrium", "redo_initial_condition"):
                self.steps = 0
            if name in ("init_equilibrium", "redo_initial_condition"):
                self.macro_steps = 0
            if name == "set_reaction" and self.kind == "expansion":
                self.set_reaction(op[1], op[2])
            elif name == "set_reaction":
                self.G = 0.01 if self.G == 0. else 0.
                self.set_reaction(self.G)
            elif name in ("set_f", "init_equilibrium", "set_obstacle_mask", "set_fields", "set_edge_state", "set_corner_state", "set_source",
                          "set_porous", "redo_initial_condition"):
                getattr(self, name)(payload(self.case, name, op[1]))
            elif name == "set_force_field":
                getattr(self, name)(*(op[1:-1] + (payload(self.case, name, op[-1]),)))
            else:
                getattr(self, name)(*op[1:])


def restorer(seed, saves):
    """The class that restores the `saves`-th checkpoint (1, 2 ...) of a noise sequence."""
    return ("Simulation", "NoisySimulation")[(int(seed) + int(saves)) % 2]


def _flow_code(oracle, bc):
    return dict(pipe=oracle.BC_PIPE, periodic=oracle.BC_PERIODIC, cavity=oracle.BC_CAVITY, velocity_inlet=oracle.BC_VELOCITY_INLET)[bc]


class ScreenedWave(object):
    """A scalar lattice of either family whose velocity a Screened_Poisson solves from its density: what Screened_Fisher_Wave drives
    (lb_run_screened, lb_spectral_velocity), with the class's un-fused sequence and its redo_initial_condition.  sim: a restored lattice
    to go on with, behind a fresh solver."""

    def __init__(self, c, sim=None):
        from LB_D2Q9 import _native
        from LB_D2Q9.simulation import Simulation
        from LB_D2Q9.spectral_poisson.screened_poisson import Screened_Poisson
        self.c, self._check = c, _native.check
        self.sim = sim if sim is not None else Simulation(c["nx"], c["ny"], c["omega"], bc=c["bc"], semantics="diffusion")
        self.solver = Screened_Poisson(np.zeros((c["nx"], c["ny"]), np.complex64), lam=c["lam"], dx=c["dx"])
        self.solver.create_grad_fields()
        self._lib = self.sim._lib

    def close(self):
        self.sim.close()
        self.solver.close()

    def update_u_and_v(self):
        self._check(self._lib.lb_spectral_velocity(self.solver._h, self.sim._h, float(self.c["scale"]), 0))
        self.sim.sync()

    def run(self, n, wait=True):
        self._check(self._lib.lb_run_screened(self.solver._h, self.sim._h, float(self.c["scale"]), int(n)))
        if wait:
            self.sim.sync()

    def step_phases(self):
        s = self.sim
        s.move(); s.move_bcs(); s.update_hydro()
        self.update_u_and_v()                       # (the class's update_hydro: the velocity follows the density)
        s.update_feq(); s.collide_particles()

    def redo_initial_condition(self, rho):
        zero = np.zeros((self.c["nx"], self.c["ny"]), F)
        self.sim.set_fields(rho, zero, zero)
        self.update_u_and_v()
        self.sim.update_feq()
        self.sim.init_pop()

    def __getattr__(self, name):                    # set_f, set_reaction, get_fields, check, sync, get_edge_state ...: the lattice's
        return getattr(self.sim, name)


class GpuPlayer(Player):
    """A GPU handle (or set of handles).  plain: the twin -- pinned to the plainest kernel, every run(n) as n x run(1)."""

    def __init__(self, case, plain=False, tmpdir=None):
        Player.__init__(self, case)
        self.plain, self.tmpdir, self.mask, self.saves = plain, tmpdir, case.get("mask"), 0
        self.h = self._create()
        self._load()
        if plain and variant_words(self.kind):
            self.h.set_variant(0)

    # -- construction -----------------------------------------------------------------------------------------------------------------
    def _create(self):
        from LB_D2Q9.coupled import Coupled_Scalars, Shan_Chen_Fluids
        from LB_D2Q9.simulation import Simulation
        c, k = self.case, self.kind
        if k == "flow":
            return Simulation(c["nx"], c["ny"], c["omega"], bc=c["bc"], inlet_rho=c["inlet_rho"], lid_u=c["lid_u"], inlet_u=c["inlet_u"],
                              outlet_u=c["outlet_u"], eager_macro=c["eager"])
        if k == "scalar":
            return Simulation(c["nx"], c["ny"], c["omega"], bc=c["bc"], semantics="diffusion")
        if k == "multifield":
            return Coupled_Scalars(c["nx"], c["ny"], c["omegas"], c["Gs"], bc=c["bc"])
        if k == "poisson":
            return Simulation(c["nx"], c["ny"], c["omega"], bc="dirichlet", semantics="poisson")
        if k == "porous":
            return Simulation(c["nx"], c["ny"], F(c["omega"]), bc=c["bc"], semantics="porous")
        if k == "rocket":
            from LB_D2Q9.coupled import Surfactant_Colony
            return Surfactant_Colony(c["nx"], c["ny"], c["omegas"][0], c["omegas"][1], mode=c["mode"])
        if k == "nutrient":
            from LB_D2Q9.nutrient_set import Nutrient_Set
            return Nutrient_Set(c["nx"], c["ny"], c["omegas"][0], c["omegas"][1], lam=c["lam"], dx=c["dx"])
        if k == "noise":
            from LB_D2Q9.noisy_simulation import NoisySimulation
            return NoisySimulation(c["nx"], c["ny"], c["omega"], bc=c["bc"])
        if k == "expansion":
            from LB_D2Q9.expansion_set import Expansion_Set
            return Expansion_Set(c["nx"], c["ny"], list(c["omegas"]), c["omega_n"], list(c["Gs"]), bc=c["bc"], zero_cutoff=c["cut"])
        if k == "screened":
            return ScreenedWave(c)
        return Shan_Chen_Fluids(c["nx"], c["ny"], list(c["omegas"]), bc=c["bc"])

    def _load(self):
        c, k, h = self.case, self.kind, self.h
        zero = np.zeros((c["nx"], c["ny"]), F)
        if k == "flow":
            if c["mask"] is not None:
                h.set_obstacle_mask(c["mask"])
            if c["bc"] == "velocity_inlet":
                h.set_fields(zero + 1, c["u0"], c["v0"])
        elif k == "scalar":
            h.set_reaction(c["G"])
            h.set_fields(zero, c["u"], c["v"])
        elif k == "multifield":
            h.set_fields(np.zeros((c["nx"], c["ny"], c["nf"]), F), c["u"], c["v"])
        elif k == "poisson":
            h.set_poisson(c["rho_on_boundary"], c["react_factor"], 0.)          # tolerance 0: the stop rule never sits near a threshold
            h.set_source(c["source"])
        elif k == "porous":
            h.set_porous(*c["porous"])
            h.set_body_force(*c["g"])
        elif k == "multifluid":
            for i, g in enumerate(c["g"]):
                h.set_body_force(i, *g)
            h.set_interactions(INTERACTIONS[c["nf"]][c["interactions"]])
            h.set_reactions(REACTIONS[c["nf"]][c["reactions"]])
        elif k == "rocket":
            self.table = c["table"]
            h.set_params(**ROCKET_TABLES[c["mode"]][self.table])
        elif k == "nutrient":
            h.set_params(clumpy=c["clumpy"], **c["params"])
        elif k == "noise":
            h.set_reaction(c["G"])
            h._set_noise(c["Dg"], c["noise_seed"])
            h.set_fields(zero, c["u"], c["v"])
        elif k == "expansion":
            h.set_noise(c["Dgs"], c["noise_seed"])
            h.set_fields(np.zeros((c["nx"], c["ny"], c["ns"] + 1), F), c["u"], c["v"])
        elif k == "screened":
            h.set_reaction(c["G"])
            h.redo_initial_condition(c["rho0"])     # (the velocity of the first density; set_f then replaces the populations)
        h.set_f(c["f0"])

    def first(self):
        return self.h.members[0] if hasattr(self.h, "members") else self.h

    def close(self):
        self.h.close()

    # -- effective ops ------------------------------------------------------------------------------------------------------------------
    def run(self, n, split=0):
        if self.plain:
            for _ in range(n):
                self.h.run(1)
        elif split:
            self.h.run(split, wait=False)
            self.h.run(n - split)
        else:
            self.h.run(n)

    def solve(self, k):
        for n in ([1] * k if self.plain else [k]):
            done, converged, _ = self.h.solve(n)
            assert (done, converged) == (n, False)

    def phase_step(self):
        h = self.h
        if self.kind in ("multifluid", "rocket", "nutrient", "expansion", "screened"):
            h.step_phases()
        elif self.kind == "porous":
            for name in ("move", "move_bcs", "update_hydro", "update_forces", "update_bary_velocity", "update_feq", "collide_particles"):
                getattr(h, name)()
        else:
            h.move(); h.move_bcs(); h.update_hydro(); h.update_feq(); h.collide_particles()

    def noisy_members(self):
        """[(index, handle)] of the lattices whose collision draws just now."""
        members = list(enumerate(self.h.strains)) if self.kind == "expansion" else [(0, self.h)]
        return [(i, m) for i, m in members if m._noise()[0] != 0.]

    def fed_phase_step(self, z):
        """set_noise_field on every noisy lattice, the phases, the fields dropped again."""
        fed = self.noisy_members()
        for i, m in fed:
            m._set_noise_field(z[:, :, i] if self.kind == "expansion" else z)
        self.phase_step()
        for _, m in fed:
            m._set_noise_field(None)

    def set_f(self, f):
        self.h.set_f(f)

    def redo_initial_condition(self, rho):
        self.h.redo_initial_condition(rho)

    def set_params(self, *a):
        if self.kind == "rocket":
            self.table = a[0]
            self.h.set_params(**ROCKET_TABLES[self.case["mode"]][a[0]])
        else:
            self.h.set_params(**{a[0]: a[1]})

    def set_noise(self, dg, seed):
        if self.kind == "expansion":
            self.h.set_noise(dg, seed)
        else:
            self.h._set_noise(dg, seed)         # (the handle may be a plain Simulation by now: a checkpoint restored by that class)

    def noise_counters(self):
        return [m._noise()[2] for m in (self.h.strains if self.kind == "expansion" else [self.h])]

    def init_equilibrium(self, ruv):
        self.h.init_equilibrium(*ruv)

    def set_obstacle_mask(self, m):
        self.mask = m
        self.h.set_obstacle_mask(m)

    def clear_obstacle_mask(self):
        self.mask = None
        self.h.set_obstacle_mask(None)

    def set_reaction(self, *a):                     # (G) or, on a set of strains, (strain, G)
        if self.kind == "expansion":
            self.h.strains[a[0]].set_reaction(a[1])
        else:
            self.h.set_reaction(a[0])

    def set_fields(self, uv):
        c = self.case
        shape = (c["nx"], c["ny"], c["ns"] + 1) if self.kind == "expansion" else (c["nx"], c["ny"])
        self.h.set_fields(np.zeros(shape, F), uv[0], uv[1])

    def set_edge_state(self, e):
        self.h.set_edge_state(e)

    def set_corner_state(self, v):
        self.h.set_corner_state(v)

    def set_source(self, s):
        self.h.set_source(s)

    def solve_reset(self):
        self.h.solve_reset()

    def set_porous(self, p):
        self.h.set_porous(*p)

    def set_body_force(self, *a):
        self.h.set_body_force(*a)

    def set_force_field(self, *a):                  # ([fluid,] (fx, fy))
        self.h.set_force_field(*(a[:-1] + tuple(a[-1])))

    def clear_force_field(self, *fluid):
        self.h.set_force_field(*(fluid + (None, None)))

    def set_interactions(self, i):
        self.h.set_interactions(INTERACTIONS[self.case["nf"]][i])

    def set_reactions(self, i):
        self.h.set_reactions(REACTIONS[self.case["nf"]][i])

    # -- transparent ops ----------------------------------------------------------------------------------------------------------------
    def transparent(self, op):
        name, h, one = op[0], self.h, self.first()
        if name == "get_fields":
            got = h.get_fields(op[1])
            assert set(got) == set(op[1])
        elif name == "check":
            for r in np.atleast_1d(h.check()):
                assert r["n_nonfinite"] == 0
        elif name == "hot_kernel":
            assert one.hot_kernel()
        elif name == "plan_launches":
            plan = one.plan_launches(op[1])
            assert plan is None or sum(plan) == op[1]
        elif name == "steps_per_launch":
            assert 1 <= one.steps_per_launch() <= 7
        elif name == "layout":
            assert one.layout()["bytes"] > 0
        elif name == "sync":
            h.sync()
        elif name == "set_variant":
            h.set_variant(op[1])
        elif name == "reupload_mask":
            h.set_obstacle_mask(self.mask)
        elif name == "mask_off_on":
            h.set_obstacle_mask(None)
            h.set_obstacle_mask(self.mask)
        elif name == "checkpoint":
            self.checkpoint()
        elif name == "get_params":
            assert h.get_params() == dict(ROCKET_TABLES[self.case["mode"]][self.table], mode=self.case["mode"])
        elif name == "get_own":
            own = OWN_NAMES[self.kind][self.case["mode"]] if self.kind == "rocket" else OWN_NAMES[self.kind]
            assert set(h.get_fields(tuple(own.values()))) == set(own.values())
        elif name == "solver_scribble":             # the set's own solver on an unrelated charge: a step solves from its density anew
            h.solver.charge.set(payload(self.case, name, op[1]))
            h.solver.solve_and_update_grad_fields()
        elif name == "noise":
            assert len(self.noise_counters()) == len(np.atleast_1d(self.case.get("Dgs", 0.)))
        elif name == "noise_fill":                  # a pure function of (seed, counter): it draws nothing
            z = one._noise_fill(op[1]) if self.kind == "noise" else h.strains[op[1]]._noise_fill(op[2])
            assert z.shape == (self.case["nx"], self.case["ny"]) and np.isfinite(z).all()
        elif name == "get_edge_state":
            assert h.get_edge_state().shape[0] == self.case["ns"] + 1
        else:
            raise ValueError(name)

    def checkpoint(self):
        """Save, close the handle, go on with what the kind's restore path builds from the checkpoint."""
        from LB_D2Q9.coupled import Coupled_Scalars, Shan_Chen_Fluids
        from LB_D2Q9.simulation import Simulation
        c = self.case
        self.saves += 1
        path = os.path.join(str(self.tmpdir), "ck%d" % self.saves)
        if self.kind == "multifield":               # (no file format of the set's own: every member's arrays)
            arrays = [m.checkpoint_arrays() for m in self.h.members]
            self.h.close()
            self.h = Coupled_Scalars(c["nx"], c["ny"], c["omegas"], [0.] * c["nf"], bc=c["bc"])
            for m, a in zip(self.h.members, arrays):
                m.restore_arrays(a)
            return
        if self.kind == "nutrient":                 # (likewise; the parameters are the set's, psi and the force follow from the densities)
            arrays, params = [m.checkpoint_arrays() for m in self.h.members], dict(self.h.params)
            self.h.close()
            self.h = self._create()
            self.h.set_params(**params)
            for m, a in zip(self.h.members, arrays):
                m.restore_arrays(a)
            self.h.update_forces()
            return
        self.h.save_checkpoint(path)
        self.h.close()
        if self.kind == "rocket":
            from LB_D2Q9.coupled import Surfactant_Colony
            self.h = Surfactant_Colony.from_checkpoint(path)
        elif self.kind == "expansion":
            from LB_D2Q9.expansion_set import Expansion_Set
            self.h = Expansion_Set.from_checkpoint(path)
        elif self.kind == "noise":                  # either class restores the noise: in turns, the first by the seed
            from LB_D2Q9.noisy_simulation import NoisySimulation
            self.h = (NoisySimulation if restorer(self.case["seed"], self.saves) == "NoisySimulation" else Simulation).from_checkpoint(path)
        elif self.kind == "screened":               # the lattice; a fresh solver behind it
            self.h = ScreenedWave(self.case, Simulation.from_checkpoint(path))
        elif self.kind == "multifluid":
            self.h = Shan_Chen_Fluids.from_checkpoint(path)
        elif self.kind == "flow":
            self.h = Simulation.from_checkpoint(path, eager_macro=c["eager"])
        else:
            self.h = Simulation.from_checkpoint(path)

    # -- read-back ------------------------------------------------------------------------------------------------------------------------
    def snapshot(self):
        """Every array the kind exposes, for the bitwise comparison."""
        h, k = self.h, self.kind
        out = dict(h.get_fields(FIELD_NAMES[k]))
        if k == "scalar":
            out["edge_state"] = h.get_edge_state()
        if k in ("multifield", "poisson") or (k == "flow" and self.case["bc"] == "velocity_inlet"):
            out["corner_state"] = h.get_corner_state()
        if k == "poisson":
            out["solve_state"] = np.array(h.solve_state())
            out["source"] = h.get_source()
        if k in ("noise", "expansion", "screened"):
            out["edge_state"] = h.get_edge_state()
        out.update(self._own())
        return out

    def _own(self):
        """psi / S and the forces of the last step, under the models' names; a Nutrient_Set's only while `clumpy` is on (get_fields)."""
        k = self.kind
        if k == "rocket":
            own = OWN_NAMES[k][self.case["mode"]]
        elif k == "nutrient" and self.h.params["clumpy"]:
            own = OWN_NAMES[k]
        else:
            return {}
        g = self.h.get_fields(tuple(own.values()))
        return {name: g[key] for name, key in own.items()}

    def fields(self):
        g = self.h.get_fields(FIELD_NAMES[self.kind])
        ren = dict(u_bary="ub", v_bary="vb") if self.kind in ("porous", "multifluid") else {}
        return dict({ren.get(k, k): v for k, v in g.items()}, **self._own())


class RefPlayer(Player):
    """The kind's reference: oracle.O2Sim (flow; `oracle` = the oracle module) or its numpy model, of dtype where it takes one."""

    def __init__(self, case, dtype=np.float64, oracle=None):
        Player.__init__(self, case)
        c, k = case, self.kind
        self.oracle = oracle
        if k == "flow":
            m = oracle.O2Sim(c["nx"], c["ny"], c["omega"], _flow_code(oracle, c["bc"]), c["inlet_rho"], 1., c["lid_u"], 1., mask=c["mask"],
                             u_w=c["inlet_u"], u_e=c["outlet_u"])
            if c["bc"] == "velocity_inlet":
                m.set_macro(np.ones((c["nx"], c["ny"])), c["u0"], c["v0"])
        elif k == "scalar":
            from scalar_model import ScalarModel
            m = ScalarModel(c["nx"], c["ny"], c["omega"], c["G"], c["bc"], dtype)
            m.set_fields(np.zeros((c["nx"], c["ny"]), F), c["u"], c["v"])
        elif k == "multifield":
            from multifield_model import MultifieldModel
            m = MultifieldModel(c["nx"], c["ny"], c["omegas"], c["Gs"], c["bc"], dtype)
            m.set_fields(np.zeros((c["nx"], c["ny"], c["nf"]), F), c["u"], c["v"])
        elif k == "poisson":
            from poisson_model import PoissonModel
            m = PoissonModel(c["nx"], c["ny"], c["omega"], c["rho_on_boundary"], c["react_factor"], dtype)
            m.set_source(c["source"])
        elif k == "porous":
            from porous_model import PorousModel
            m = PorousModel(c["nx"], c["ny"], F(c["omega"]), *c["porous"], bc=c["bc"], dtype=dtype)
            m.set_body_force(*c["g"])
        elif k == "rocket":
            from rocket_model import RocketModel
            m = RocketModel(c["nx"], c["ny"], c["omegas"][0], c["omegas"][1], c["mode"], dtype, **ROCKET_TABLES[c["mode"]][c["table"]])
        elif k == "nutrient":
            from nutrient_model import NutrientModel
            m = NutrientModel(c["nx"], c["ny"], c["omegas"][0], c["omegas"][1], clumpy=c["clumpy"], dtype=dtype, lam=c["lam"], **c["params"])
        elif k == "noise":
            from noise_model import NoisyScalarModel
            m = NoisyScalarModel(c["nx"], c["ny"], c["omega"], c["G"], c["Dg"], c["noise_seed"], c["bc"], dtype)
            m.set_fields(np.zeros((c["nx"], c["ny"]), F), c["u"], c["v"])
        elif k == "expansion":                      # (the float32 model with the engine's arithmetic: every operation of the Milstein term in float32)
            from expansion_model import ExpansionModel
            m = ExpansionModel(c["nx"], c["ny"], c["omegas"], c["omega_n"], c["Gs"], c["Dgs"], [c["noise_seed"] + i for i in range(c["ns"])],
                               c["cut"], c["bc"], dtype, milstein="single")
            m.set_fields(np.zeros((c["nx"], c["ny"], c["ns"] + 1), F), c["u"], c["v"])
        elif k == "screened":
            from spectral_model import ScreenedFisherModel
            m = ScreenedFisherModel(c["nx"], c["ny"], c["omega"], c["G"], c["lam"], c["scale"], c["bc"], dtype)
            m.redo_initial_condition(c["rho0"])
        else:
            from multifluid_model import MultifluidModel
            m = MultifluidModel(c["nx"], c["ny"], c["omegas"], c["bc"], dtype)
            for i, g in enumerate(c["g"]):
                m.set_body_force(i, *g)
            m.interactions = list(INTERACTIONS[c["nf"]][c["interactions"]])
            m.reactions = list(REACTIONS[c["nf"]][c["reactions"]])
        self.m = m
        m.set_f(c["f0"])

    def run(self, n, split=0):
        self.m.run(n)

    def solve(self, k):
        assert self.m.solve(k, 0.)[:2] == (k, False)

    def phase_step(self):
        m = self.m
        if self.kind in ("porous", "multifluid", "rocket", "nutrient", "expansion", "screened"):
            m.step()                                # (the model's step IS its stages in order)
        elif self.kind in ("scalar", "noise"):
            m.move(); m.update_hydro(); m.update_feq(); m.collide_particles()
        else:
            m.move(); m.move_bcs(); m.update_hydro(); m.update_feq(); m.collide_particles()

    def fed_phase_step(self, z):
        m = self.m
        if self.kind == "expansion":
            m.noise_fields = [z[:, :, i] if m.Dg[i] != 0 else None for i in range(m.np_)]
            m.step()
            m.noise_fields = [None] * m.np_
        else:
            m.noise_field = z
            self.phase_step()
            m.noise_field = None

    def set_f(self, f):
        self.m.set_f(f)

    def redo_initial_condition(self, rho):
        self.m.redo_initial_condition(rho)

    def set_params(self, *a):
        if self.kind == "rocket":
            self.m.set_params(**ROCKET_TABLES[self.case["mode"]][a[0]])
        elif a[0] == "clumpy":
            self.m.clumpy = bool(a[1])
        else:
            self.m.set_params(**{a[0]: a[1]})

    def set_noise(self, dg, seed):
        """lb_set_noise: the strength and the seed, and the counter back to 0 -- also where the strength is 0."""
        m = self.m
        if self.kind == "expansion":
            m.Dg, m.seeds, m.t = [m.T(F(d)) for d in dg], [int(seed) + i for i in range(m.np_)], [0] * m.np_
        else:
            m.Dg, m.seed, m.t = m.T(F(dg)), int(seed), 0

    def noise_counters(self):
        return list(self.m.t) if self.kind == "expansion" else [self.m.t]

    def init_equilibrium(self, ruv):
        self.m.set_macro(*ruv)
        self.m.update_feq()
        self.m.init_pop(None)

    def set_obstacle_mask(self, mask):
        self.m.set_mask(mask)

    def clear_obstacle_mask(self):
        self.m.mask = None

    def set_reaction(self, *a):
        if self.kind == "expansion":
            self.m.G[a[0]] = self.m.T(F(a[1]))
        else:
            self.m.set_reaction(a[0])

    def set_fields(self, uv):
        c = self.case
        shape = (c["nx"], c["ny"], c["ns"] + 1) if self.kind == "expansion" else (c["nx"], c["ny"])
        self.m.set_fields(np.zeros(shape, self.m.T), uv[0], uv[1])

    def set_edge_state(self, e):
        self.m.set_edge_state(e)

    def set_corner_state(self, v):
        self.m.set_corner_state(v)

    def set_source(self, s):
        self.m.set_source(s)

    def solve_reset(self):
        self.m.solve_reset()

    def set_porous(self, p):
        m = self.m
        m.eps, m.nu, m.K, m.Fe = (m.T(x) for x in p)

    def set_body_force(self, *a):
        self.m.set_body_force(*a)

    def set_force_field(self, *a):
        self.m.set_force_field(*(a[:-1] + tuple(a[-1])))

    def clear_force_field(self, *fluid):
        self.m.set_force_field(*(fluid + (None, None)))

    def set_interactions(self, i):
        self.m.interactions = list(INTERACTIONS[self.case["nf"]][i])

    def set_reactions(self, i):
        self.m.reactions = list(REACTIONS[self.case["nf"]][i])

    def fields(self):
        m = self.m
        if self.kind in ("porous", "multifluid"):
            return dict(f=m.f, feq=m.feq, rho=m.rho, u=m.u, v=m.v, ub=m.ub, vb=m.vb, Gx=m.Gx, Gy=m.Gy)
        if self.kind == "rocket":
            return {k: v for k, v in m.get_fields().items() if m.mode == "forces" or k not in ("Sx", "Sy")}
        if self.kind == "nutrient":
            return dict(m.state(), feq=m.feq)
        return m.get_fields()

    def porous_header(self):
        m = self.m
        return dict(epsilon=m.eps, nu_fluid=m.nu, K=m.K, Fe=m.Fe)


# ---- a flow and the scalars it carries (kind 'advected'): a set of unlike lattices whose members also live on their own ------------------
class Clock(object):
    """The steps since a member's populations were set and the steps behind its rho, u, v, feq (Player's two counters, per member)."""

    def __init__(self):
        self.steps = self.macro_steps = 0

    def stepped(self, n):
        self.steps += n
        self.macro_steps = self.steps


class Held(object):
    """What hold_to_contract asks of a reference player, for one member."""

    def __init__(self, fields, clock):
        self._fields, self.steps, self.macro_steps = fields, clock.steps, clock.macro_steps

    def fields(self):
        return self._fields


class AdvectedPlayer(object):
    def __init__(self, case):
        self.case, self.kind, self.ns = case, case["kind"], case["ns"]
        self.G = list(case["Gs"])

    def effective(self, op):
        name, c = op[0], self.case
        if name == "run":
            self.set_run(op[1], op[2], op[3])
        elif name == "member_run":
            self.member_run(op[3], op[1])
        elif name == "set_f":
            self.set_f(op[2], payload(c, name, op[1], who=op[2]))
        elif name == "init_equilibrium":
            self.init_equilibrium(payload(c, name, op[1]))
        elif name == "set_reaction":
            self.G[op[1]] = op[2]
            self.set_reaction(op[1], op[2])
        elif name == "set_fields":
            self.set_fields(op[2], payload(c, name, op[1]))
        else:
            raise ValueError(name)


class AdvectedGpu(AdvectedPlayer):
    """The subject: an Advected_Scalars with the case's flag and layouts, every op.  plain: the twin -- separately created handles in the
    default layout, the flow with eager_macro=True, every member under set_variant(0); a set step is lb_run(flow, 1), then per scalar
    set_velocity_from(flow) and lb_run(scalar, 1), and it records the u, v the flow stored for that step (`history`, of the last set
    run); a member's run(n) is n x run(1).  In the lazy family the twin also keeps what a fresh lazy flow handle makes of its populations
    over the flow's last own run (`alone`): there the subject rebuilds rho, u, v from the post-collision populations -- the same moments
    as the eager twin's stored ones, not the same bits -- and its feq follows them."""

    def __init__(self, case, plain=False, tmpdir=None):
        AdvectedPlayer.__init__(self, case)
        from LB_D2Q9 import _native
        from LB_D2Q9.coupled import Advected_Scalars
        self.plain, self.tmpdir, self.saves, self._check = plain, tmpdir, 0, _native.check
        self.flow_fields_from, self.alone, self.history = "init", None, []
        c = case
        flow = self._flow(True if plain else c["eager"], False if plain else c["planar_flow"])
        flow.init_equilibrium(c["rho"], c["u"], c["v"], c["f0"])
        scalars = []
        for om, G, (dye, factors) in zip(c["omegas"], c["Gs"], c["dyes"]):
            s = self._simulation()(c["nx"], c["ny"], om, bc="periodic", semantics="diffusion", planar=False if plain else c["planar_scalars"])
            s.set_reaction(G)
            s.init_equilibrium(dye, c["u"], c["v"], factors)
            scalars.append(s)
        if plain:
            self._members = [flow] + scalars
            for m in self._members:
                m.set_variant(0)
        else:
            self.set = Advected_Scalars(flow, scalars)

    @staticmethod
    def _simulation():
        from LB_D2Q9.simulation import Simulation
        return Simulation

    def _flow(self, eager, planar):
        c = self.case
        return self._simulation()(c["nx"], c["ny"], c["omega"], bc="periodic", eager_macro=eager, planar=planar)

    def member(self, who):
        """who: -1 the flow, else the scalar"""
        if self.plain:
            return self._members[1 + who]
        return self.set.flow if who == -1 else self.set.members[who]

    def members(self):
        return [self.member(w) for w in range(-1, self.ns)]

    def close(self):
        if self.plain:
            for m in self._members:
                m.close()
        else:
            self.set.close()

    # -- effective ops ------------------------------------------------------------------------------------------------------------------
    def set_run(self, n, split=0, form=-1):
        if not self.plain:
            if split:
                self.set.run(split, wait=False, form=form)
                self.set.run(n - split, form=form)
            else:
                self.set.run(n, form=form)
        else:
            flow, lib = self.member(-1), self.member(-1)._lib
            self.history = []
            for _ in range(n):
                self._check(lib.lb_run(flow._h, 1))
                for s in self._members[1:]:
                    s.set_velocity_from(flow)
                    self._check(lib.lb_run(s._h, 1))
                for m in self._members:
                    m.sync()
                g = flow.get_fields(("u", "v"))
                self.history.append((g["u"], g["v"]))
        self.flow_fields_from = "set"

    def member_run(self, who, n):
        m = self.member(who)
        if not self.plain:
            m.run(n)
        else:
            if who == -1 and not self.case["eager"]:
                lazy = self._flow(False, False)
                lazy.set_variant(0)
                lazy.set_f(m.get_fields(("f",))["f"])
                for _ in range(n):
                    lazy.run(1)
                self.alone = lazy.get_fields(MEMBER_FIELDS)
                lazy.close()
            for _ in range(n):
                m.run(1)
            if who == -1 and not self.case["eager"]:
                assert np.array_equal(self.alone["f"], m.get_fields(("f",))["f"]), "the twin's lazy and eager flow handles part in f"
        if who == -1:
            self.flow_fields_from = "own"

    def set_f(self, who, f):
        self.member(who).set_f(f)

    def init_equilibrium(self, ruv):
        self.member(-1).init_equilibrium(*ruv)
        self.flow_fields_from = "init"

    def set_reaction(self, who, G):
        self.member(who).set_reaction(G)

    def set_fields(self, who, uv):
        self.member(who).set_fields(np.zeros((self.case["nx"], self.case["ny"]), F), uv[0], uv[1])

    # -- transparent ops (the subject's) ----------------------------------------------------------------------------------------------------
    def transparent(self, op):
        name, st = op[0], self.set
        if name == "get_fields":
            assert set(st.get_fields(op[1])) == set(op[1])
        elif name == "member_fields":
            for m in self.members():
                assert set(m.get_fields(op[1])) == set(op[1])
        elif name == "check":
            r = st.check()
            assert r["flow"]["n_nonfinite"] == 0 and all(x["n_nonfinite"] == 0 for x in r["scalars"]) and len(r["scalars"]) == self.ns
        elif name == "hot_kernel":
            assert st.hot_kernel() and st.hot_kernel(0) and st.hot_kernel(1) and all(m.hot_kernel() for m in self.members())
        elif name == "sync":
            st.sync()
        elif name == "set_variant":
            self.member(op[2]).set_variant(op[1])
        elif name == "checkpoint":                  # through a closed set: fresh handles, the flag from the file, the default layout
            from LB_D2Q9.coupled import Advected_Scalars
            self.saves += 1
            path = os.path.join(str(self.tmpdir), "ck%d" % self.saves)
            st.save_checkpoint(path)
            st.close()
            self.set = Advected_Scalars.from_checkpoint(path)
            assert self.set.flow.eager_macro == self.case["eager"] and self.set.num_populations == self.ns
            assert [float(m.G) for m in self.set.members] == [float(F(g)) for g in self.G]
        else:
            raise ValueError(name)

    # -- read-back ------------------------------------------------------------------------------------------------------------------------
    def snapshot(self):
        """Every member's f, rho, u, v, feq.  The twin's, in the lazy family while the flow's fields are those of its own run: the flow's
        rho, u, v, feq of the lazy handle that made the same run (`alone`)."""
        out = {}
        for who, m in zip(range(-1, self.ns), self.members()):
            prefix = "flow_" if who == -1 else "s%d_" % who
            out.update({prefix + k: a for k, a in m.get_fields(MEMBER_FIELDS).items()})
        if self.plain and not self.case["eager"] and self.flow_fields_from == "own":
            out.update({"flow_" + k: self.alone[k] for k in ("rho", "u", "v", "feq")})
        return out


class AdvectedRef(AdvectedPlayer):
    """The references: oracle.O2Sim for the flow, a float64 ScalarModel per scalar.  A set step is a step of the flow and, per scalar, a
    step under the velocity of `feed` for that step -- what the GPU twin stored (AdvectedGpu.history): the scalar contract was
    established for an imposed velocity with the same bits on both sides, the velocity itself is the flow's hold --; without a feed,
    O2Sim's own."""

    def __init__(self, case, oracle):
        AdvectedPlayer.__init__(self, case)
        from scalar_model import ScalarModel
        c = case
        self.flow = oracle.O2Sim(c["nx"], c["ny"], c["omega"], oracle.BC_PERIODIC, 1., 1.)
        self.flow.set_macro(c["rho"], c["u"], c["v"])
        self.flow.update_feq()
        self.flow.init_pop(c["f0"])
        self.scalars = []
        for om, G, (dye, factors) in zip(c["omegas"], c["Gs"], c["dyes"]):
            m = ScalarModel(c["nx"], c["ny"], om, G, "periodic", np.float64)
            m.set_fields(dye, c["u"], c["v"])
            m.update_feq()
            m.set_f(m.feq * factors)
            self.scalars.append(m)
        self.clocks = [Clock() for _ in range(1 + self.ns)]         # the flow's, then every scalar's
        self.feed = None

    def clock(self, who):
        return self.clocks[1 + who]

    def set_run(self, n, split=0, form=-1):
        assert self.feed is None or len(self.feed) == n
        for k in range(n):
            self.flow.run(1)
            u, v = self.feed[k] if self.feed is not None else (self.flow.u.T, self.flow.v.T)
            for m in self.scalars:
                m.u, m.v = np.array(u, np.float64), np.array(v, np.float64)
                m.step()
        self.feed = None
        for c in self.clocks:
            c.stepped(n)

    def member_run(self, who, n):
        (self.flow if who == -1 else self.scalars[who]).run(n)
        self.clock(who).stepped(n)

    def set_f(self, who, f):
        (self.flow if who == -1 else self.scalars[who]).set_f(f)
        self.clock(who).steps = 0

    def init_equilibrium(self, ruv):
        self.flow.set_macro(*ruv)
        self.flow.update_feq()
        self.flow.init_pop(None)
        self.clock(-1).steps = self.clock(-1).macro_steps = 0

    def set_reaction(self, who, G):
        self.scalars[who].set_reaction(G)

    def set_fields(self, who, uv):
        self.scalars[who].set_fields(np.zeros((self.case["nx"], self.case["ny"])), uv[0], uv[1])


def hold_advected(label, twin, ref):
    """Property B of a carried set, by the two existing contracts: the twin's flow against O2Sim under the flow contract
    (hold_to_contract('flow')), every scalar of the twin against its float64 model under the scalar contract (test_gpu_scalar.assert_close:
    f for the steps since it was set, rho and feq for the steps behind them), u, v -- imposed, with the same bits -- equal.  Every cell."""
    from test_gpu_scalar import assert_close
    hold_to_contract("flow", label + ", the flow", twin.member(-1).get_fields(MEMBER_FIELDS), Held(ref.flow.get_fields(), ref.clock(-1)))
    for i, m in enumerate(ref.scalars):
        have, want, what = twin.member(i).get_fields(MEMBER_FIELDS), m.get_fields(), "%s, scalar %d" % (label, i)
        assert all(np.isfinite(np.asarray(want[k])).all() for k in want), what
        assert_close(have, want, ref.clock(i).steps, ("f",), what)
        assert_close(have, want, ref.clock(i).macro_steps, ("rho", "feq"), what)
        assert np.array_equal(have["u"], want["u"]) and np.array_equal(have["v"], want["v"]), what


def play(player, ops, at=None, cuts=(), transparent=False):
    """Play ops on a player; after the op at each index of `cuts` call at(index).  transparent: make the T ops too (the subject)."""
    for i, op in enumerate(ops):
        if is_effective(op):
            player.effective(op)
        elif transparent:
            player.transparent(op)
        if at is not None and i in cuts:
            at(i)


def hold_to_contract(kind, label, have, ref):
    """Property B: `have` (fields() of a player) against the reference player `ref` within the kind's own comparison: the populations
    for the ref.steps steps since they were set, everything else for the ref.macro_steps steps behind it (the two differ only right
    behind a set_f).  Each comparison prints measured / bound."""
    want = ref.fields()
    n, nm = ref.steps, ref.macro_steps
    if kind == "flow":
        from test_gpu_parity import assert_fields_close, contract_tol
        print(label, end=": ")
        assert_fields_close(have, want, dict(contract_tol(nm), f=contract_tol(n)["f"]))
    elif kind in ("scalar", "multifield", "poisson"):
        assert_close = __import__("test_gpu_" + kind).assert_close
        assert_close(have, want, n, ("f",), label)
        assert_close(have, want, nm, ("rho", "feq"), label)
        if kind != "poisson":
            assert np.array_equal(have["u"], want["u"]) and np.array_equal(have["v"], want["v"])       # imposed: no run writes them
    elif kind in ("noise", "expansion", "screened"):        # scalar lattices: the scalar contract, in every cell -- no mask, no NaN allowance
        from test_gpu_scalar import assert_close
        assert all(np.isfinite(np.asarray(want[k])).all() for k in want), label
        assert_close(have, want, n, ("f",), label)
        assert_close(have, want, nm, ("rho", "feq"), label)
        if kind == "screened":                      # a velocity that is computed
            assert_close(have, want, nm, ("u", "v"), label)
        else:
            assert np.array_equal(have["u"], want["u"]) and np.array_equal(have["v"], want["v"])
        if kind == "expansion":                     # the links and densities that are exactly 0 (tests/test_expansion_cpu.py's hold): there are none
            for k in ("f", "rho"):
                assert np.array_equal(np.asarray(have[k]) == 0, np.asarray(want[k]) == 0) and not (np.asarray(want[k]) == 0).any(), (label, k)
    elif kind == "rocket":
        from test_rocket_cpu import compare
        assert all(np.isfinite(np.asarray(want[k])).all() for k in want), label
        compare("%s after %d steps" % (label, n), ref.m, n, have, want, ["f"])
        compare("%s after %d steps" % (label, nm), ref.m, nm, have, want, [k for k in want if k != "f"])
    elif kind == "nutrient":
        from test_nutrient_cpu import compare
        assert all(np.isfinite(np.asarray(want[k])).all() for k in want) and set(have) == set(want), label
        compare("%s after %d steps" % (label, n), ref.m.params, n, dict(f=have["f"]), dict(f=want["f"], rho=want["rho"]))
        compare("%s after %d steps" % (label, nm), ref.m.params, nm, {k: v for k, v in have.items() if k != "f"}, {k: v for k, v in want.items() if k != "f"})
    else:
        compare = __import__("test_%s_cpu" % kind).compare
        about = ref.porous_header() if kind == "porous" else ref.m
        compare("%s after %d steps" % (label, n), about, n, have, want, ["f"])
        compare("%s after %d steps" % (label, nm), about, nm, have, want, [k for k in want if k != "f"])
