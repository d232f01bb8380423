"""The random call sequences of tests/test_gpu_sequences.py without a GPU (tests/sequence_scenarios.py): the generator is
deterministic and covers its tables; on exactly these inputs -- mid-life parameter, table and mask changes included -- the float32
model of every kind that has one stays within the kind's contract of the float64 model, and
the flow kinds' oracle stays in the range the contract was established in; the op lists of the kinds that were here first have not
moved; where a collision has thresholds, the float64 model keeps every thresholded quantity further from its threshold than twice the
contract's bound, so that an implementation inside the contract cannot sit on the other side.  For a flow and the scalars it carries
(kind 'advected') the references are played alone, step by step and on to the full 120 steps: the flow stays in the contract's range,
every growing dye inside (0, 1)."""
import hashlib

import numpy as np
import pytest

import sequence_scenarios as S

CASES = [(k, f, s) for k in S.KINDS for f in S.FAMILIES[k] for s in S.SEEDS]
ids = lambda cases: ["%s-%s-%d" % c for c in cases]
HAVE_DTYPE = ("scalar", "multifield", "poisson", "porous", "multifluid", "rocket", "nutrient", "noise", "expansion", "screened")
# sha1 over repr(generate(kind, family, seed)) for all families and seeds of a kind, taken before the generator learnt further kinds
OLD_DIGESTS = dict(flow="5366cbf62836f6752d9dd508bc3f3c42b99dbceb", scalar="500005ea4af649b7af3a4fe4872ce240dc235b0b",
                   multifield="4758ca676c4fb3b62d99f82d2ee9f5f90d6d4c26", poisson="37d28bcd89142eb087f330d50b352998b3e4d9b2",
                   porous="7dde112a067b46efc2be02930dee8c02e2f48c68", multifluid="a0e62ab06d1ecefccb10fe759f0de28c9317e8cf")
# the same for the five kinds that came next, taken before 'advected' was added, and for 'advected' itself once its lists were final
LATER_DIGESTS = dict(rocket="6462665ec6f23e8e42e49e5536dd108d8803ba98", nutrient="35e0203670bb7504135cc5a04a14e97133def6f9",
                     noise="d82ce5212a4895d2d2fd06112cc098e57d49089a", expansion="de72f120ec9b31fa0e26774899ae7637fc92deee",
                     screened="6c2e4dd2df30d3a102ce3ddddbe1d024d195ca16", advected="39e2dddd2b63b87ae25c6278b327b3bddd0d9cab")


@pytest.mark.parametrize("kind,family,seed", CASES, ids=ids(CASES))
def test_generator_is_deterministic_and_within_its_limits(kind, family, seed):
    ops = S.generate(kind, family, seed)
    assert ops == S.generate(kind, family, seed)
    e, t, steps = S.counts(ops)
    assert 1 <= e <= S.MAX_E and 1 <= t <= S.MAX_T and 1 <= steps <= S.STEP_CAP.get(kind, S.MAX_STEPS) <= S.MAX_STEPS, (e, t, steps)
    assert ops[-1][0] == "run"
    for op in ops:                                      # plain values only: the lists above compare by value
        assert all(isinstance(a, (str, int, float, tuple, type(None))) and not isinstance(a, np.generic) for a in op), op
        if op[0] in ("run", "solve", "plan_launches"):
            assert op[1] in S.RUN_LENGTHS
    cuts = S.cut_points(ops, kind, family, seed)
    assert cuts == S.cut_points(ops, kind, family, seed) and cuts[-1] == len(ops) - 1 and len(cuts) == 3
    assert all(ops[i][0] in S.STEPPING + ("set_f",) for i in cuts) and len(set(cuts)) == 3
    a, b = S.case_of(kind, family, seed), S.case_of(kind, family, seed)
    assert np.array_equal(a["f0"], b["f0"]) and a["f0"].dtype == np.float32


@pytest.mark.parametrize("kind", S.KINDS)
def test_every_op_of_the_tables_occurs(kind):
    """Over the committed seeds of a kind: every effective and every transparent op, every variant word the kind's handles accept,
    every run length, both directions of a toggle."""
    ops = [op for f in S.FAMILIES[kind] for s in S.SEEDS for op in S.generate(kind, f, s)]
    names = {op[0] for op in ops}
    assert set(S.E_OPS[kind]) <= names, set(S.E_OPS[kind]) - names
    assert set(S.T_OPS[kind]) - {"split_run"} <= names, set(S.T_OPS[kind]) - names
    assert any(op[0] == "run" and op[2] for op in ops)                                          # split_run
    assert {op[1] for op in ops if op[0] == "set_variant"} == set(S.variant_words(kind))
    assert {op[1] for op in ops if op[0] in ("run", "solve")} == set(S.RUN_LENGTHS)
    assert any("feq" in op[1] for op in ops if op[0] == "get_fields")
    behind = {S.generate(kind, f, s)[i][0] for f in S.FAMILIES[kind] for s in S.SEEDS for i in S.cut_points(S.generate(kind, f, s), kind, f, s)}
    assert behind >= ({"run", "member_run", "set_f"} if kind == "advected" else {"run", "phase_step", "set_f"}), behind     # what a comparison follows
    if kind == "multifluid":
        for name in ("set_interactions", "set_reactions"):
            assert {op[1] for op in ops if op[0] == name} == {0, 1, 2}
        assert {S.case_of(kind, "periodic", s)["nf"] for s in S.SEEDS} == {2, 3}
    if kind == "flow":
        assert {S.case_of(kind, f, s)["mask"] is None for f in S.FAMILIES[kind] for s in S.SEEDS} == {True, False}
    if kind == "scalar":
        assert {S.case_of(kind, f, s)["G"] for f in S.FAMILIES[kind] for s in S.SEEDS} == {0., 0.01}
    lives = [S.generate(kind, f, s) for f in S.FAMILIES[kind] for s in S.SEEDS]
    if kind == "rocket":
        for f in S.FAMILIES[kind]:                      # every table of a mode, set in the middle of a life
            assert {op[1] for s in S.SEEDS for op in S.generate(kind, f, s) if op[0] == "set_params"} == {0, 1, 2}
        assert {S.case_of(kind, "flow", s)["nx"] for s in S.SEEDS} == {n for n, _ in S.ROCKET_SHAPES}
    if kind == "nutrient":
        for life in lives:                              # `clumpy` both ways inside every life
            assert {op[2] for op in life if op[:2] == ("set_params", "clumpy")} == {True, False}
        assert {op[1] for op in ops if op[0] == "set_params"} == {"clumpy"} | set(S.NUTRIENT_VALUES)
    if kind == "noise":
        switched = [[op[1] for op in life if op[0] == "set_noise"] for life in lives]
        assert any(d[0] == 0. and any(x != 0. for x in d[1:]) for d in switched)                 # off and back on
        assert any(d == [0.] for d in switched) and any(len(d) == 1 and d[0] != 0. for d in switched)
        restored = {S.restorer(s, k + 1) for f in S.FAMILIES[kind] for s in S.SEEDS
                    for k in range(sum(op[0] == "checkpoint" for op in S.generate(kind, f, s)))}
        assert restored == {"Simulation", "NoisySimulation"}                                       # both restoring classes
    if kind == "expansion":
        assert {S.case_of(kind, "open", s)["ns"] for s in S.SEEDS} == {1, 2, 3}                   # every strain count
        strengths = [op[1] for op in ops if op[0] == "set_noise"]
        assert any(0. in d and any(x != 0. for x in d) for d in strengths) and any(0. not in d for d in strengths)
        assert {op[1] for op in ops if op[0] == "set_reaction"} == {0, 1, 2}
    if kind == "screened":
        assert {S.case_of(kind, "open", s)["nx"] for s in S.SEEDS} == {n for n, _ in S.SPECTRAL_SHAPES}
    if kind == "advected":
        the_set_words, own_words, scalar_words = S.advected_words()
        crossed, met = set(), set()                     # (scalar, its rate in three set runs one after the other); (shape, scalars)
        for f in S.FAMILIES[kind]:
            cases = [S.case_of(kind, f, s) for s in S.SEEDS]
            assert [c["ns"] for c in cases] == [1 + s % 2 for s in S.SEEDS] and {c["eager"] for c in cases} == {f == "eager"}
            assert [(c["nx"], c["ny"]) for c in cases[:2]] in (list(S.ADVECTED_SHAPES), list(S.ADVECTED_SHAPES[::-1]))      # alternating
            met.update((c["nx"], c["ny"], c["ns"]) for c in cases)
            for c, s in zip(cases, S.SEEDS):
                life, rates, seen = S.generate(kind, f, s), list(c["Gs"]), [[] for _ in range(c["ns"])]
                assert S.advected_rates(f, s)[0] == c["Gs"] and all(g in (0., S._r32(S.ADVECTED_G)) for g in rates)
                assert any(op[0] == "member_run" and op[3] == -1 and op[1] > 16 for op in life)              # the graph replays
                for op, nxt in zip(life, life[1:] + [None]):
                    if op[0] == "set_reaction":
                        assert op[2] in (0., S._r32(S.ADVECTED_G)) and op[2] != rates[op[1]]
                        rates[op[1]] = op[2]
                    if op[0] == "run":
                        for i, g in enumerate(rates):
                            seen[i].append(g != 0.)
                    if op[0] == "set_fields":           # the scalar's own run uses the velocity, a set run behind it replaces it
                        behind = [o for o in life[life.index(op) + 1:] if S.is_effective(o)]
                        assert behind[0][0] == "member_run" and behind[0][3] == op[2] and any(o[0] == "run" for o in behind)
                    if op[0] == "set_variant":          # each word in front of the run that reads it; the set's run of form 0
                        if nxt[0] == "run":
                            assert op[2] == -1 and op[1] in the_set_words and nxt[3] == 0 and not nxt[2], (op, nxt)
                        else:
                            assert nxt[0] == "member_run" and nxt[3] == op[2] and op[1] in (own_words if op[2] == -1 else scalar_words), (op, nxt)
                for i, marks in enumerate(seen):
                    crossed |= {(i, tuple(marks[k:k + 3])) for k in range(len(marks) - 2)}
        assert met == {(nx, ny, ns) for nx, ny in S.ADVECTED_SHAPES for ns in (1, 2)}, met                # either count of scalars at either shape
        assert crossed >= {(i, way) for i in (0, 1) for way in ((False, True, False), (True, False, True))}, crossed
        assert {c["planar_flow"] for f in S.FAMILIES[kind] for c in [S.case_of(kind, f, s) for s in S.SEEDS]} == {True, False}
        assert {c["planar_scalars"] for f in S.FAMILIES[kind] for c in [S.case_of(kind, f, s) for s in S.SEEDS]} == {True, False}
        assert {op[3] for op in ops if op[0] == "run"} == {-1, 0, 1}                                    # every form
        assert {op[2] for op in ops if op[0] in ("set_f", "set_fields")} == {-1, 0, 1}                      # set_f on the flow and on either scalar
        assert {op[3] for op in ops if op[0] == "member_run"} == {-1, 0, 1}
        assert any("feq_flow" in op[1] for op in ops if op[0] == "get_fields") and any("feq" in op[1] for op in ops if op[0] == "member_fields")


def test_the_cases_that_were_here_first_have_not_moved():
    """Adding kinds shifts no draw of the 102 op lists that the GPU file's measured shares and defect table were recorded on."""
    for kind, want in OLD_DIGESTS.items():
        h = hashlib.sha1()
        for f in S.FAMILIES[kind]:
            for s in S.SEEDS:
                h.update(repr(S.generate(kind, f, s)).encode())
        assert h.hexdigest() == want, kind
    assert sum(len(S.FAMILIES[k]) * len(S.SEEDS) for k in OLD_DIGESTS) == 102


def test_the_later_kinds_have_not_moved_either():
    """The 60 op lists of rocket ... screened as they were before the carried set joined, and the twelve of the carried set that
    tests/test_gpu_sequences.py's defect table was recorded on."""
    for kind, want in LATER_DIGESTS.items():
        h = hashlib.sha1()
        for f in S.FAMILIES[kind]:
            for s in S.SEEDS:
                h.update(repr(S.generate(kind, f, s)).encode())
        assert h.hexdigest() == want, kind
    assert set(OLD_DIGESTS) | set(LATER_DIGESTS) == set(S.KINDS) and S.KINDS[-1] == "advected"


@pytest.mark.parametrize("kind,family,seed", CASES, ids=ids(CASES))
def test_transparent_ops_sit_where_they_can_matter(kind, family, seed):
    """In every sequence: a read lies behind a stepping op (only there can it find macro_valid / feq_valid stale, and only from there
    can it disturb what follows); every variant word stands directly in front of a run, so each selects something; the mask is uploaded
    again, and taken off and put back, only while a mask is set."""
    ops = S.generate(kind, family, seed)
    stepped = [any(o[0] in S.STEPPING for o in ops[:i]) for i in range(len(ops))]
    assert any(op[0] == "get_fields" and stepped[i] for i, op in enumerate(ops))
    words = [i for i, op in enumerate(ops) if op[0] == "set_variant"]
    assert len(words) == (S.N_VARIANTS if S.variant_words(kind) else 0)
    assert all(ops[i + 1][0] in (("run", "member_run") if kind == "advected" else ("run",)) for i in words)     # (a set's run or a member's own)
    has_mask = kind == "flow" and S.case_of(kind, family, seed)["mask"] is not None
    for op in ops:
        if op[0] in ("reupload_mask", "mask_off_on"):
            assert has_mask, ops
        has_mask = op[0] == "set_obstacle_mask" or (has_mask and op[0] != "clear_obstacle_mask")


@pytest.mark.parametrize("kind", S.KINDS)
def test_transparent_ops_are_interleaved_at_random(kind):
    """Over the committed seeds of a kind: no two sequences play their transparent ops in the same order; reads, check() and the
    checkpoint round trip each occur behind a stepping op, a checkpoint also behind a variant word that a run has used; every
    variant word occurs directly in front of a run of at least VARIANT_DEPTH steps in one call, where its kernel can run."""
    lists = [S.generate(kind, f, s) for f in S.FAMILIES[kind] for s in S.SEEDS]
    orders = {tuple(op[0] for op in ops if not S.is_effective(op)) for ops in lists}
    assert len(orders) == len(lists)
    behind_step, behind_word, deep = set(), set(), set()
    for ops in lists:
        stepped = word_used = False
        for op, nxt in zip(ops, ops[1:]):
            if not S.is_effective(op):
                behind_step |= {op[0]} if stepped else set()
                behind_word |= {op[0]} if word_used else set()
            stepped |= op[0] in S.STEPPING
            if op[0] == "set_variant":
                word_used = True                        # (nxt is its run: test_transparent_ops_sit_where_they_can_matter)
                if max(nxt[2], nxt[1] - nxt[2]) >= S.VARIANT_DEPTH:
                    deep.add(op[1])
    assert behind_step >= set(S.T_OPS[kind]) - {"split_run", "set_variant"}, behind_step
    assert deep == set(S.variant_words(kind)), set(S.variant_words(kind)) - deep
    if S.variant_words(kind):
        assert behind_word >= {"checkpoint", "get_fields", "set_variant"}, behind_word


DTYPE_CASES = [c for c in CASES if c[0] in HAVE_DTYPE]


@pytest.mark.parametrize("kind,family,seed", DTYPE_CASES, ids=ids(DTYPE_CASES))
def test_float32_model_stays_within_the_contract_of_the_float64_model(kind, family, seed):
    """Property B of the GPU file with the float32 model in the GPU's place: the reference alone is inside the contract on these
    inputs, so a GPU handle that is not has no excuse in them."""
    case, ops = S.case_of(kind, family, seed), S.generate(kind, family, seed)
    m32, m64 = S.RefPlayer(case, np.float32), S.RefPlayer(case, np.float64)
    cuts = S.cut_points(ops, kind, family, seed)
    for i, op in enumerate(ops):
        if S.is_effective(op):
            m32.effective(op)
            m64.effective(op)
        if i in cuts:
            assert (m64.steps, m64.macro_steps) == (m32.steps, m32.macro_steps) and m64.macro_steps >= 1
            S.hold_to_contract(kind, "%s %s seed %d op %d, float32 model / float64 model" % (kind, family, seed, i), m32.fields(), m64)
    if kind in ("porous", "multifluid"):
        rho = np.asarray(m64.m.rho)
        speed = np.sqrt(np.asarray(m64.m.ub) ** 2 + np.asarray(m64.m.vb) ** 2)
        assert rho.min() > 0.5 and rho.max() < 1.5 and speed.max() < 0.15, (rho.min(), rho.max(), speed.max())
    if kind in ("rocket", "nutrient", "screened"):      # the range rocket_bounds / nutrient_bounds were established in (their fixtures' and
        rho = np.asarray(m64.m.rho)                     # droplet cases': densities 0 ... 1.5, speeds below 0.15); the screened wave's likewise
        speed = np.sqrt(np.asarray(m64.m.u) ** 2 + np.asarray(m64.m.v) ** 2)
        assert rho.min() > 0. and rho.max() < 1.5 and speed.max() < 0.15, (rho.min(), rho.max(), speed.max())


FLOW_CASES = [c for c in CASES if c[0] == "flow"]


@pytest.mark.parametrize("kind,family,seed", FLOW_CASES, ids=ids(FLOW_CASES))
def test_flow_oracle_stays_in_the_contracts_range(oracle, kind, family, seed):
    """rho in 0.5 ... 1.5 and |u| < 0.15 after every stepping op of the sequence: the range the parity contract was established in."""
    case, ops = S.case_of(kind, family, seed), S.generate(kind, family, seed)
    o = S.RefPlayer(case, oracle=oracle)
    worst = [1., 1., 0.]

    def look(i):
        g = o.m
        speed = float(np.sqrt(g.u.astype(np.float64) ** 2 + g.v.astype(np.float64) ** 2).max())
        worst[:] = [min(worst[0], float(g.rho.min())), max(worst[1], float(g.rho.max())), max(worst[2], speed)]
        assert 0.5 < g.rho.min() and g.rho.max() < 1.5 and speed < 0.15, (i, ops[i], float(g.rho.min()), float(g.rho.max()), speed)

    S.play(o, ops, look, [i for i, op in enumerate(ops) if op[0] in S.STEPPING])
    print("%s seed %d: rho %.3f ... %.3f, max |u| %.4f" % (family, seed, worst[0], worst[1], worst[2]))


ADVECTED_CASES = [c for c in CASES if c[0] == "advected"]


@pytest.mark.parametrize("kind,family,seed", ADVECTED_CASES, ids=ids(ADVECTED_CASES))
def test_carried_set_references_stay_in_the_contracts_range(oracle, kind, family, seed):
    """The references of a carried set alone, O2Sim's own u, v standing in for the GPU twin's history, looked at after EVERY step of the
    life and after every other effective op (set_f, init_equilibrium, set_reaction in the middle of it included): the flow inside the
    range the flow contract was established in (rho 0.5 ... 1.5, |u| < 0.15); every scalar finite, and the density of its populations
    inside (0, 1) while its G != 0 (the growth term's fixed points).  Prints the smallest margins of the life."""
    case, ops = S.case_of(kind, family, seed), S.generate(kind, family, seed)
    ref = S.AdvectedRef(case, oracle)
    worst = dict(rho=np.inf, speed=np.inf, dye=np.inf)
    steps = [0]

    def look(op):
        g = ref.flow
        speed = float(np.sqrt(g.u.astype(np.float64) ** 2 + g.v.astype(np.float64) ** 2).max())
        lo, hi = float(g.rho.min()), float(g.rho.max())
        assert 0.5 < lo and hi < 1.5 and speed < 0.15, (steps[0], op, lo, hi, speed)
        worst["rho"], worst["speed"] = min(worst["rho"], lo - 0.5, 1.5 - hi), min(worst["speed"], 0.15 - speed)
        for i, m in enumerate(ref.scalars):
            assert all(np.isfinite(a).all() for a in m.get_fields().values()), (steps[0], op, i)
            if m.G != 0:
                rho = m.f.sum(axis=2)
                assert 0. < rho.min() and rho.max() < 1., (steps[0], op, i, float(rho.min()), float(rho.max()))
                worst["dye"] = min(worst["dye"], float(rho.min()), 1. - float(rho.max()))

    look(None)
    for op in ops:
        if not S.is_effective(op):
            continue
        if op[0] in ("run", "member_run"):              # step by step
            for _ in range(op[1]):
                ref.effective((op[0], 1) + tuple(op[2:]))
                steps[0] += 1
                look(op)
        else:
            ref.effective(op)
            look(op)
    assert steps[0] == S.counts(ops)[2] <= S.MAX_STEPS and all(c.steps <= steps[0] for c in ref.clocks)
    life = steps[0]
    while steps[0] < S.MAX_STEPS:                       # ... and on to the full MAX_STEPS, had the last run been that long
        ref.effective(("run", 1, 0, -1))
        steps[0] += 1
        look(("run", 1, 0, -1))
    print("(the life has %d steps)" % life, end=" ")
    print("%s seed %d, %d steps: smallest margins: the flow's rho %.3f from 0.5 / 1.5, |u| %.4f below 0.15, a growing dye's rho %.3f from 0 / 1"
          % (family, seed, steps[0], worst["rho"], worst["speed"], worst["dye"]))


# ---- the thresholds of the noisy collisions and of the colony -------------------------------------------------------------------------
THRESHOLD_KINDS = ("rocket", "noise", "expansion")
NEW_KINDS = ("rocket", "nutrient", "noise", "expansion", "screened")


def threshold_margins(ref):
    """{quantity: its smallest distance from its threshold / (2 x the contract's bound for it and the steps behind it)} of a float64
    reference player right behind a stepping op.  The populations are held for ref.steps steps, the densities for ref.macro_steps.
      noise      rho against 0 and 1 (outside: NaN), the new links against 0 (below: 0)
      expansion  every member's rho against zero_cutoff (below: 0), the new links against 0
      rocket     the population's new links against 0"""
    from scalar_model import contract_tol
    m, kind = ref.m, ref.kind
    f2, rho2 = 2. * contract_tol(ref.steps)["f"], 2. * contract_tol(ref.macro_steps)["rho"]
    if kind == "noise":
        return dict(rho=float(min(m.rho.min(), (1. - m.rho).min())) / rho2, links=float(m.f.min()) / f2)
    if kind == "expansion":
        g = m.get_fields()
        return dict(rho=float(np.abs(g["rho"] - float(m.cut)).min()) / rho2, links=float(g["f"].min()) / f2)
    return dict(links=float(m.f[:, :, 0].min()) / f2)


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_float64_model_is_finite_and_far_from_every_threshold(kind):
    """After every stepping op of the kind's twelve sequences the float64 reference is finite in every cell of every array, and where
    the collision has thresholds (rho < zero_cutoff -> 0, a link < 0 -> 0, rho outside [0, 1] -> NaN) every thresholded quantity lies more
    than twice its contract bound from its threshold: a margin above 1 below.  A threshold crossed in one precision and not in the other
    is no rounding difference; with these margins every cell can be compared, and is."""
    worst = {}
    for family in S.FAMILIES[kind]:
        for seed in S.SEEDS:
            case, ops = S.case_of(kind, family, seed), S.generate(kind, family, seed)
            ref = S.RefPlayer(case, np.float64)

            def look(i):
                assert all(np.isfinite(np.asarray(a)).all() for a in ref.fields().values()), (family, seed, i, ops[i])
                if kind in THRESHOLD_KINDS:
                    for q, margin in threshold_margins(ref).items():
                        if margin < worst.get(q, (np.inf,))[0]:
                            worst[q] = (margin, family, seed, i, S.counts(ops[:i + 1])[2])

            S.play(ref, ops, look, [i for i, op in enumerate(ops) if op[0] in S.STEPPING])
    for q, (margin, family, seed, i, steps) in sorted(worst.items()):
        print("%s: smallest margin of %s %.3g (x twice the bound; %s seed %d behind op %d, step %d of the life)" % (kind, q, margin, family, seed, i, steps))
    assert set(worst) == ({"links", "rho"} if kind in ("noise", "expansion") else {"links"} if kind == "rocket" else set())
    assert all(w[0] > 1. for w in worst.values()), worst
