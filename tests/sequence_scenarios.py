"""Random call sequences for every handle kind, and the players that run one (test infrastructure; not a test module).

A sequence is a list of ops, each a tuple of plain Python values (a name, then ints, floats, tuples or None), drawn from a
seeded numpy generator: the same (kind, family, seed) always gives the same list.  Arrays never sit in an op: an op carries a
payload seed and `payload()` makes the array from it, the same one for every player.

  EFFECTIVE ops change the physics; every player makes them:  run(n), phase_step, set_f, and the kind's own state-changing
  calls (E_OPS below).
  TRANSPARENT ops must change nothing; only the subject makes them: reads, the planner's answers, set_variant, the mask
  uploaded again, a checkpoint round trip through a closed handle (T_OPS below), and run(n) split into run(a, wait=False); run(n - a)
  (the third entry of a run op; the other players ignore it).  They are shuffled and land at random places of the list, except
  that every variant word stands directly in front of a run (so that it selects something), one read at least lies behind a
  stepping op, and the mask is uploaded again or taken off and on while one is set.

Three players (tests/test_gpu_sequences.py): the subject (a GPU handle, E and T ops, from the automatic variant), the twin (a
GPU handle pinned to the plainest kernel, E ops only, every run(n) as n x run(1)) and the reference (oracle.O2Sim for the
flow kinds, the kind's numpy model in float64 otherwise).  tests/test_sequences_cpu.py plays the
references alone.

Amplitudes, tables and parameters are chosen so that every reference stays in the range the parity contract was established
in (rho 0.5 ... 1.5, |u| < 0.15 for the flow kinds) over the 120 steps a sequence may take, mid-life changes included.
"""
import os

import numpy as np

F = np.float32
W64 = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)

KINDS = ("flow", "scalar", "multifield", "poisson", "porous", "multifluid")
SEEDS = tuple(range(6))
RUN_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 13, 16, 17, 33, 40)     # every fused depth, the 16-launch graph replay and its remainder
MAX_E, MAX_T, MAX_STEPS = 10, 15, 120
N_VARIANTS, VARIANT_DEPTH = 2, 8               # variant words per sequence; the steps in one call that let every word's kernel run

FAMILIES = dict(
    flow=("pipe", "pipe-eager", "periodic", "periodic-eager", "cavity", "cavity-eager", "velocity_inlet", "velocity_inlet-eager"),
    scalar=("periodic", "open"),
    multifield=("box", "periodic"),
    poisson=("dirichlet",),
    porous=("periodic", "zero_gradient"),
    multifluid=("periodic", "zero_gradient"),
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
FLOW_SHAPES = dict(periodic=(516, 130), pipe=(517, 131), cavity=(517, 131), velocity_inlet=(517, 131))
POROUS_SHAPES = ((261, 9), (256, 4))
MULTIFLUID_SHAPES = ((517, 5, 3), (261, 9, 2), (6, 13, 2))

E_OPS = dict(
    flow=("run", "phase_step", "set_f", "init_equilibrium", "set_obstacle_mask", "clear_obstacle_mask"),
    scalar=("run", "phase_step", "set_f", "set_reaction", "set_fields", "set_edge_state"),
    multifield=("run", "phase_step", "set_f", "set_corner_state"),
    poisson=("run", "phase_step", "set_f", "set_source", "solve", "solve_reset"),
    porous=("run", "phase_step", "set_f", "set_body_force", "set_force_field", "clear_force_field", "set_porous"),
    multifluid=("run", "phase_step", "set_f", "set_body_force", "set_force_field", "clear_force_field", "set_interactions", "set_reactions"),
)
_READS = ("get_fields", "hot_kernel", "plan_launches", "steps_per_launch", "layout", "sync", "checkpoint", "split_run")
T_OPS = dict(
    flow=_READS + ("check", "set_variant", "reupload_mask", "mask_off_on"),
    scalar=_READS + ("check", "set_variant"),
    multifield=_READS + ("check",),
    poisson=_READS,
    porous=_READS,
    multifluid=_READS + ("set_variant",),
)
STEPPING = ("run", "phase_step", "solve")
FIELD_NAMES = dict(
    flow=("f", "rho", "u", "v", "feq"), scalar=("f", "rho", "u", "v", "feq"), multifield=("f", "rho", "u", "v", "feq"),
    poisson=("f", "rho", "feq"),
    porous=("f", "feq", "rho", "u", "v", "u_bary", "v_bary", "Gx", "Gy"),
    multifluid=("f", "feq", "rho", "u", "v", "Gx", "Gy", "u_bary", "v_bary"),
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


def variant_words(kind):
    from LB_D2Q9.variants import (AUTO, K_DEEP2, K_DEEP6, K_DEEP7, K_STEP, K_STEP2, K_STEP3, K_STEP4, K_STEP5, K_TILE4, NT_STORES, ROWS_2,
                                  TILES, XCD_ORDER)
    if kind == "flow":
        return (AUTO, K_STEP, K_STEP2, K_STEP3, K_STEP4, K_STEP5, K_DEEP6, K_DEEP7, K_DEEP2, K_TILE4, NT_STORES | ROWS_2, XCD_ORDER)
    if kind == "scalar":
        return (AUTO, K_STEP, TILES | 1 << 2, TILES | 2 << 2, TILES | 3 << 2)
    if kind == "multifluid":
        return (-1, 0, 1)
    return ()


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
    else:
        raise ValueError(kind)
    c["f0"] = payload(c, "set_f", 1000)
    return c


def payload(c, name, pseed):
    """The array(s) of op `name` with payload seed `pseed` on case c."""
    kind, nx, ny = c["kind"], c["nx"], c["ny"]
    rng = np.random.default_rng(_key(kind, c["family"], c["seed"]) + [2, int(pseed)])
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    phase = rng.uniform(0., 2. * np.pi, 2)
    wave = lambda p: np.sin(2. * np.pi * y / ny + p[0]) * np.cos(2. * np.pi * x / nx + p[1])
    if name == "set_f":
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


# ---- the generator ---------------------------------------------------------------------------------------------------------------------
def generate(kind, family, seed):
    """The op list of (kind, family, seed): at most MAX_E effective and MAX_T transparent ops, at most MAX_STEPS steps, a stepping
    op last.  Every effective op of the kind that the family has occurs once, runs fill the rest."""
    rng = np.random.default_rng(_key(kind, family, seed) + [3])
    names = [n for n in E_OPS[kind] if not (n == "set_edge_state" and family != "open")]
    names += ["run"] * (MAX_E - 1 - len(names))
    rng.shuffle(names)
    names.append("run")
    steps_left, pseed, ops = MAX_STEPS, 0, []
    state = dict(table=seed % 3, react=(seed + 1) % 3)          # (as case_of)

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
        elif name in ("set_f", "init_equilibrium", "set_obstacle_mask", "set_fields", "set_edge_state", "set_corner_state", "set_source"):
            ops.append((name, pseed))
        elif name in ("clear_obstacle_mask", "solve_reset"):
            ops.append((name,))
        elif name == "set_reaction":
            ops.append((name, "toggle"))
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


def starts_masked(family, seed):
    """Whether the flow case (family, seed) starts with an obstacle mask."""
    return bool(np.random.default_rng(_key("flow", family, seed) + [6]).integers(0, 2))


def _nf(kind, seed):
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
    steps = sum(op[1] if op[0] in ("run", "solve") else 1 for op in e if op[0] in STEPPING)
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
            else:
                self.phase_step()
            self.steps += 1 if name == "phase_step" else op[1]
            self.macro_steps = self.steps
        else:
            if name in ("set_f", "init_equilibrium"):
                self.steps = 0
            if name == "init_equilibrium":
                self.macro_steps = 0
            if name == "set_reaction":
                self.G = 0.01 if self.G == 0. else 0.
                self.set_reaction(self.G)
            elif name in ("set_f", "init_equilibrium", "set_obstacle_mask", "set_fields", "set_edge_state", "set_corner_state", "set_source",
                          "set_porous"):
                getattr(self, name)(payload(self.case, name, op[1]))
            elif name == "set_force_field":
                getattr(self, name)(*(op[1:-1] + (payload(self.case, name, op[-1]),)))
            else:
                getattr(self, name)(*op[1:])


def _flow_code(oracle, bc):
    return dict(pipe=oracle.BC_PIPE, periodic=oracle.BC_PERIODIC, cavity=oracle.BC_CAVITY, velocity_inlet=oracle.BC_VELOCITY_INLET)[bc]


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
        if self.kind == "multifluid":
            h.step_phases()
        elif self.kind == "porous":
            for name in ("move", "move_bcs", "update_hydro", "update_forces", "update_bary_velocity", "update_feq", "collide_particles"):
                getattr(h, name)()
        else:
            h.move(); h.move_bcs(); h.update_hydro(); h.update_feq(); h.collide_particles()

    def set_f(self, f):
        self.h.set_f(f)

    def init_equilibrium(self, ruv):
        self.h.init_equilibrium(*ruv)

    def set_obstacle_mask(self, m):
        self.mask = m
        self.h.set_obstacle_mask(m)

    def clear_obstacle_mask(self):
        self.mask = None
        self.h.set_obstacle_mask(None)

    def set_reaction(self, G):
        self.h.set_reaction(G)

    def set_fields(self, uv):
        self.h.set_fields(np.zeros((self.case["nx"], self.case["ny"]), F), uv[0], uv[1])

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
        self.h.save_checkpoint(path)
        self.h.close()
        if self.kind == "multifluid":
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
        return out

    def fields(self):
        g = self.h.get_fields(FIELD_NAMES[self.kind])
        ren = dict(u_bary="ub", v_bary="vb") if self.kind in ("porous", "multifluid") else {}
        return {ren.get(k, k): v for k, v in g.items()}


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
        if self.kind in ("porous", "multifluid"):
            m.step()                                # (the model's step IS its stages in order)
        elif self.kind == "scalar":
            m.move(); m.update_hydro(); m.update_feq(); m.collide_particles()
        else:
            m.move(); m.move_bcs(); m.update_hydro(); m.update_feq(); m.collide_particles()

    def set_f(self, f):
        self.m.set_f(f)

    def init_equilibrium(self, ruv):
        self.m.set_macro(*ruv)
        self.m.update_feq()
        self.m.init_pop(None)

    def set_obstacle_mask(self, mask):
        self.m.set_mask(mask)

    def clear_obstacle_mask(self):
        self.m.mask = None

    def set_reaction(self, G):
        self.m.set_reaction(G)

    def set_fields(self, uv):
        self.m.set_fields(np.zeros_like(self.m.rho), uv[0], uv[1])

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
        return m.get_fields()

    def porous_header(self):
        m = self.m
        return dict(epsilon=m.eps, nu_fluid=m.nu, K=m.K, Fe=m.Fe)


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
    else:
        compare = __import__("test_%s_cpu" % kind).compare
        about = ref.porous_header() if kind == "porous" else ref.m
        compare("%s after %d steps" % (label, n), about, n, have, want, ["f"])
        compare("%s after %d steps" % (label, nm), about, nm, have, want, [k for k in want if k != "f"])
