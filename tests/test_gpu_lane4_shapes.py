"""Every kernel of the lane-of-four plan (csrc/kernels_lane4.h) at each edge residue and tile seam: the boxes of tests/lane4_shapes.py,
classified there, run here for every handle kind beyond plain flow, boundary family and form.

A case is (kind, family, form, nx, ny), taken from lane4_shapes.cases() -- the function the host test's census reads
(tests/test_lane4_shapes_cpu.py), so the two cannot drift apart.  The inputs are the kinds' own random cases (tests/test_gpu_<kind>.py),
seeded by a function of (nx, ny); the host test has shown that their float32 model sits inside the bound used here and that a misplaced
column or row leaves it by a factor of ten.  Every case

  * compares the handle after 1, 2 and 5 steps -- run(1); run(1); run(3) on one handle (the scalar lattices, whose tile kernel takes four
    steps a launch: run(1); run(4) and, on a second handle, run(2)): a launch that is the run's last, launches that are not, the stored
    moments each time -- with the float64 numpy model (tests/<kind>_model.py) inside the project's parity
    contract (contract_tol and the bounds the kind's host test derives from it), every array the kind's own comparison covers, and
    prints measured / bound;
  * where the product computes the step twice and claims the same bits (the un-fused phases of the Poisson solver, the porous medium,
    the multifluid set and the colony; k_ad_tile4 against k_ad_step with and without noise), holds the two to np.array_equal.  The
    phases of the scalar, noisy, coupled, nutrient and expansion lattices round the relaxation differently from their fused steps by
    design: those are held to the contract, step by step, as their own files hold them;
  * Poisson: the device's ratio of solve(1) against the float64 ratio of the box (1e-5 relative), and again with the row padding
    poisoned where the east wall is the second or third cell of its lane.

The carried scalars (lb_run_advected) stay on their own yardstick: the twin sequence of lb_run calls, bit for bit, at this table's boxes.

One-line defects tried against this file in a scratch copy of the library, value-changing only (a wrong select, constant or component:
no address moves), none kept, each build run once on an MI355X; the new cases each turned red
(of those run for its kinds), and what the kinds' own files before this change (tests/test_gpu_<kind>.py of the kinds that include the helper) made of the same build:
  clamp_x: the select uses j == c + 1                          ->  91 of 270 (porous zero_gradient 22 model + 22 phases, multifluid zero_gradient
                                                                   25 + 22: every box with c != 0); before: 20 of 120 (porous 5, multifluid 15)
  clamp_x: the select is skipped at c == 1 alone               ->  26 of 270 (porous zero_gradient 6 + 6: 6 x 8, 254 x 3, 258 x 11; multifluid
                                                                   zero_gradient 8 + 6); before: test_gpu_porous.py NONE of 36,
                                                                   test_gpu_multifluid.py 6 of 84 (its 6 x 9 and 6 x 13)
  lane_nb_load: the c == 1 substitution returns v.z            ->  26 of 248 (multifluid 14, colony 12: every box with c = 1 in either family);
                                                                   before: 16 of 116 (multifluid's 6 x 9 and 6 x 13, the colony's 258 x 9)
  ad_edge_gather: j == c becomes j == 3                        ->  113 of 352 (scalar open 38, noisy open 50, expansion open 25: every box with
                                                                   c != 3); before: 64 of 165
  row_wall: e = (j == 3) for lanes with 0 <= ce < 4            ->  86 of 169 (Poisson 25 model + 21 phases + 14 ratios, coupled sets box 26: every
                                                                   box with c != 3); before: 31 of 51
  k_ps_step: the `in` selection becomes x4 + j <= a.nx         ->  27 of 93 (the ratio at 20 of 22 boxes -- all but 256 x 4 and 512 x 4, whose
                                                                   rows have no padding -- and all 7 poisoned ones); before: 3 of 20
                                                                   (the ratio at 261 x 9, clean and poisoned, and the checkpoint in mid-solve)
  cell_rho: the periodic east wrap substitutes the cell itself ->  62 of the 162 multifluid and colony cases that had run when the step met its
                                                                   time limit, on a machine that ran the build before it twenty times slower
                                                                   than any other did; not run again, so no count for the kinds' own files
Every defect that ran to the end turned new cases red.  Those that change every width off one residue were seen by the kinds' own files
as well, since every list holds some such width; what the table adds there is where they are seen -- at every residue, on both sides of
a tile seam, in every family and form.  The defect confined to one residue (clamp_x at c == 1) passed the whole of the porous medium's
own file and is seen here at every porous box with c = 1.  No defective build faulted.
"""
import functools

import numpy as np
import pytest

import lane4_shapes as L4
from scalar_model import contract_tol

pytestmark = pytest.mark.gpu

F = np.float32
STEPS = (1, 2, 5)
WORST = {}                          # kind -> the worst measured / bound of the session (printed with every case)


def seed_of(nx, ny):
    return 1000 * nx + ny


def maxratio(have, want, bound):
    """max |have - want| / bound (bound: a number or an array that broadcasts), and max |have - want|"""
    d = np.abs(np.asarray(have, np.float64) - np.asarray(want, np.float64))
    return float(np.max(d / bound)), float(np.max(d))


def hold(kind, label, bounds, have, want, keys):
    """Print measured / bound for every array, then hold each to its bound; returns the worst ratio."""
    meas = {k: maxratio(have[k], want[k], bounds[k]) for k in keys}
    worst = max(r for r, _ in meas.values())
    WORST[kind] = max(WORST.get(kind, 0.), worst)
    print("%s: %s; worst measured / bound %.3f (this kind so far %.3f)"
          % (label, ", ".join("%s %.2e / %.1e" % (k, meas[k][1], float(np.max(bounds[k]))) for k in keys), worst, WORST[kind]))
    for k in keys:
        assert meas[k][0] <= 1., (label, k, meas[k][1], float(np.max(bounds[k])))
    return worst


def same_bits(a, b, keys=None):
    return [k for k in (keys or b) if not np.array_equal(a[k], b[k], equal_nan=True)]


def plain_tol(n):
    tol = contract_tol(n)
    tol["feq"] = tol["f"]
    return tol


# ---- the kinds: inputs (pure numpy), the model, the handle, the bounds ----------------------------------------------------------
# A kind is a class of static methods:
#   inputs(family, form, nx, ny)   the case, a dict of numpy arrays and numbers        model_form(form)   the part of the form the model sees
#   model(d, family, form, dtype)  the numpy model holding the case                    state(m)           its arrays, by the keys of KEYS
#   bounds(d, m, n, want)          the contract bound per array for n steps             open(d, family, form) / got(s)   the handle, its arrays
#   twice(d, family, form)         the product's second computation of the same steps, held bit for bit (or None)
class Scalar:
    RUNS = ((1, 4), (2,))           # k_ad_tile4 takes four steps: run(1); run(4) on one handle, run(2) on another

    @staticmethod
    def keys(form):
        return ("f", "rho", "feq")

    @staticmethod
    def inputs(family, form, nx, ny):
        from test_gpu_scalar import random_case
        c = random_case(nx, ny, seed_of(nx, ny))
        c.update(omega=F(1.25), G=F(0.01))
        return c

    model_form = staticmethod(lambda form: None)

    @staticmethod
    def model(d, family, form, dtype):
        from scalar_model import ScalarModel
        m = ScalarModel(d["nx"], d["ny"], d["omega"], d["G"], family, dtype)
        m.set_fields(np.zeros_like(d["u"]), d["u"], d["v"])
        m.set_f(d["f0"])
        return m

    state = staticmethod(lambda m: m.get_fields())
    bounds = staticmethod(lambda d, m, n, want: plain_tol(n))

    @staticmethod
    def word(form):
        from LB_D2Q9.variants import K_STEP, TILES
        return dict(K_STEP=K_STEP, TILES=TILES)[form]

    @classmethod
    def open(cls, d, family, form):
        from test_gpu_scalar import sim_of
        s = sim_of(d, family)
        s.set_variant(cls.word(form))
        return s

    got = staticmethod(lambda s: s.get_fields())

    @classmethod
    def twice(cls, d, family, form):
        """k_ad_tile4 = four k_ad_step, bit for bit: run(5) is [4, 1] under TILES"""
        a, b = cls.open(d, family, "K_STEP"), cls.open(d, family, form)
        a.run(5), b.run(5)
        bad = same_bits(a.get_fields(("f", "rho")), b.get_fields(("f", "rho")))
        a.close(), b.close()
        assert not bad, bad


class Noisy(Scalar):
    @staticmethod
    def inputs(family, form, nx, ny):
        from test_gpu_noise import case
        return case(nx, ny, seed_of(nx, ny))

    @staticmethod
    def model(d, family, form, dtype):
        from noise_model import NoisyScalarModel
        m = NoisyScalarModel(d["nx"], d["ny"], d["omega"], d["G"], d["Dg"], d["seed"], family, dtype)
        m.set_fields(np.zeros_like(d["u"]), d["u"], d["v"])
        m.set_f(d["f0"])
        return m

    @staticmethod
    def word(form):
        from LB_D2Q9.variants import K_STEP, STEP4_NO_AHEAD, TILES
        return dict(K_STEP=K_STEP, plane=TILES, cell=TILES | STEP4_NO_AHEAD)[form]

    @classmethod
    def open(cls, d, family, form):
        from test_gpu_noise import sim_of
        s = sim_of(d, family)
        s.set_variant(cls.word(form))
        return s

    @classmethod
    def twice(cls, d, family, form):
        """either noise plan of k_ad_tile4 = four noisy k_ad_step, bit for bit"""
        a, b = cls.open(d, family, "K_STEP"), cls.open(d, family, form)
        a.run(5), b.run(5)
        bad = same_bits(a.get_fields(("f", "rho")), b.get_fields(("f", "rho")))
        counters = a.noise()[2], b.noise()[2]
        a.close(), b.close()
        assert not bad and counters == (5, 5), (bad, counters)


class Multifield:
    keys = staticmethod(lambda form: ("f", "rho"))
    model_form = staticmethod(lambda form: form)

    @staticmethod
    def inputs(family, form, nx, ny):
        from test_gpu_multifield import random_case
        return random_case(nx, ny, form, seed_of(nx, ny))

    @staticmethod
    def model(d, family, form, dtype):
        from multifield_model import MultifieldModel
        from test_gpu_multifield import load
        return load(MultifieldModel(d["nx"], d["ny"], d["omega"], d["G"], family, dtype), d)

    state = staticmethod(lambda m: m.get_fields())
    bounds = staticmethod(lambda d, m, n, want: plain_tol(n))

    @staticmethod
    def open(d, family, form):
        from test_gpu_multifield import set_of
        return set_of(d, family)

    got = staticmethod(lambda s: s.get_fields())
    twice = staticmethod(lambda d, family, form: None)


class Poisson:
    keys = staticmethod(lambda form: ("f", "rho", "feq"))
    model_form = staticmethod(lambda form: None)

    @staticmethod
    def inputs(family, form, nx, ny):
        from test_gpu_poisson import random_case
        return random_case(nx, ny, seed_of(nx, ny))

    @staticmethod
    def model(d, family, form, dtype):
        from test_poisson_cpu import model_of
        return model_of(d, dtype)

    state = staticmethod(lambda m: m.get_fields())
    bounds = staticmethod(lambda d, m, n, want: plain_tol(n))

    @staticmethod
    def open(d, family, form):
        """'run': lb_run launches k_ps_step<false>; 'solve': lb_solve with tolerance 0 launches k_ps_step<true> and never stops"""
        from test_gpu_poisson import sim_of
        s = sim_of(d) if form == "run" else sim_of(d, tolerance=0.)
        if form == "solve":
            s.run = lambda n, solve=s.solve: solve(n)
        return s

    got = staticmethod(lambda s: s.get_fields(("f", "rho", "feq")))

    @staticmethod
    def twice(d, family, form):
        """the fused step of either form = the five phases, bit for bit, step by step"""
        fused, phases = Poisson.open(d, family, form), Poisson.open(d, family, "run")
        for n in (1, 2):
            fused.run(1)
            for phase in (phases.move, phases.move_bcs, phases.update_hydro, phases.update_feq, phases.collide_particles):
                phase()
            bad = same_bits(fused.get_fields(("f", "rho")), phases.get_fields(("f", "rho")))
            assert not bad, (n, bad)
        fused.close(), phases.close()


class Porous:
    keys = staticmethod(lambda form: ("f", "feq", "rho", "u", "v", "ub", "vb", "Gx", "Gy"))
    model_form = staticmethod(lambda form: form)

    @staticmethod
    def inputs(family, form, nx, ny):
        from test_gpu_porous import random_case
        return random_case(nx, ny, family, seed_of(nx, ny), field=(form == "field"))

    @staticmethod
    def model(d, family, form, dtype):
        from test_porous_cpu import model_of
        return model_of(d, dtype)

    @staticmethod
    def state(m):
        from test_porous_cpu import state
        return state(m)

    @staticmethod
    def bounds(d, m, n, want):
        from test_porous_cpu import bounds
        return bounds(d, n, want)

    @staticmethod
    def open(d, family, form):
        from test_gpu_porous import sim_of
        return sim_of(d)

    @staticmethod
    def got(s):
        from test_gpu_porous import got_of
        return got_of(s)

    @staticmethod
    def twice(d, family, form):
        from test_gpu_porous import ALL, sim_of, step_by_phases
        a, b = sim_of(d), sim_of(d)
        for n in (1, 2):
            a.run(1)
            step_by_phases(b)
            bad = same_bits(a.get_fields(ALL), b.get_fields(ALL))
            assert not bad, (n, bad)
        a.close(), b.close()


class Multifluid:
    keys = staticmethod(lambda form: ("f", "feq", "rho", "u", "v", "ub", "vb", "Gx", "Gy"))
    model_form = staticmethod(lambda form: None)

    @staticmethod
    def inputs(family, form, nx, ny):
        """two fluids with interactions between and within them, so the density around a cell matters"""
        from test_gpu_multifluid import random_case
        return random_case(nx, ny, family, 2, seed_of(nx, ny))

    @staticmethod
    def model(d, family, form, dtype):
        from test_gpu_multifluid import model_of_case
        return model_of_case(d, dtype)

    @staticmethod
    def state(m):
        from test_multifluid_cpu import state
        return state(m)

    @staticmethod
    def bounds(d, m, n, want):
        from test_multifluid_cpu import bounds
        return bounds(m, n, want)

    @staticmethod
    def open(d, family, form):
        from test_gpu_multifluid import set_of
        s = set_of(d)
        s.set_variant(form)
        return s

    @staticmethod
    def got(s):
        from test_gpu_multifluid import got_of
        return got_of(s)

    @staticmethod
    def twice(d, family, form):
        from test_gpu_multifluid import ALL
        a, b = Multifluid.open(d, family, form), Multifluid.open(d, family, form)
        for n in (1, 2):
            a.run(1)
            b.step_phases()
            bad = same_bits(a.get_fields(ALL), b.get_fields(ALL))
            assert not bad, (n, bad)
        a.close(), b.close()


class Rocket:
    @staticmethod
    def keys(form):
        from test_gpu_rocket import all_keys
        return all_keys(form[1])

    model_form = staticmethod(lambda form: form[1])

    @staticmethod
    def inputs(family, form, nx, ny):
        from test_gpu_rocket import smooth_case
        return smooth_case(nx, ny, form[1], seed_of(nx, ny))

    @staticmethod
    def model(d, family, form, dtype):
        from rocket_model import from_fixture
        return from_fixture(d, dtype)

    @staticmethod
    def state(m):
        from test_rocket_cpu import state
        return state(m)

    @staticmethod
    def bounds(d, m, n, want):
        from test_rocket_cpu import bounds
        return bounds(m, n, float(np.max(want["rho"])))

    @staticmethod
    def open(d, family, form):
        from test_gpu_rocket import colony_of
        s = colony_of(d)
        s.set_variant(form[0])
        return s

    @staticmethod
    def got(s):
        from test_gpu_rocket import all_keys, got_of
        return got_of(s, all_keys(s.mode))

    @staticmethod
    def twice(d, family, form):
        a, b = Rocket.open(d, family, form), Rocket.open(d, family, form)
        for n in (1, 2):
            a.run(1)
            b.step_phases()
            bad = same_bits(Rocket.got(a), Rocket.got(b))
            assert not bad, (n, bad)
        a.close(), b.close()


class Nutrient:
    OMEGAS = (0.8, 1.25)

    @staticmethod
    def keys(form):
        from test_gpu_nutrient import all_keys
        return all_keys(form[0] == "clumpy")

    model_form = staticmethod(lambda form: form[0])

    @staticmethod
    def inputs(family, form, nx, ny):
        """test_gpu_nutrient.droplet_case with a seed of the box, on a rough floor: 0.7 x a noisy droplet + 0.5 (1 +- 10 %) on a uniform
        nutrient, at equilibrium.  (The droplet alone is zero at the edges of a wide box: a wrong east column would change nothing.)"""
        from nutrient_model import NutrientModel
        from spectral_model import noisy_droplet
        from test_gpu_nutrient import CASE
        clumpy = form[0] == "clumpy"
        m = NutrientModel(nx, ny, 0.8, 1.25, clumpy=clumpy, dtype=np.float64, **CASE)
        rho0 = np.ones((nx, ny, 2), F)
        floor = 0.5 * (1. + 0.1 * np.random.default_rng(seed_of(nx, ny)).uniform(-1., 1., (nx, ny)))
        rho0[:, :, 0] = (0.7 * noisy_droplet(nx, ny, 10, 0.5, seed_of(nx, ny)) + floor).astype(F)
        m.redo_initial_condition(rho0)
        return dict(nx=nx, ny=ny, clumpy=clumpy, params=dict(CASE), f0=m.f.astype(F))

    @staticmethod
    def model(d, family, form, dtype):
        from nutrient_model import NutrientModel
        m = NutrientModel(d["nx"], d["ny"], 0.8, 1.25, clumpy=d["clumpy"], dtype=dtype, **d["params"])
        m.set_f(d["f0"])
        return m

    state = staticmethod(lambda m: m.state())

    @staticmethod
    def bounds(d, m, n, want):
        from test_nutrient_cpu import bounds
        return bounds(d["params"], n, float(np.max(np.asarray(want["rho"])[:, :, 0])))

    @staticmethod
    def open(d, family, form):
        from test_gpu_nutrient import set_of
        return set_of(d["nx"], d["ny"], Nutrient.OMEGAS, d["params"], d["clumpy"], d["f0"])

    @staticmethod
    def got(s):
        from test_gpu_nutrient import all_keys, got_of
        return got_of(s, all_keys(s.params["clumpy"]))

    @staticmethod
    def twice(d, family, form):
        """The stages with the velocity of the stored (0) or the streamed (1) density: what does not cross the relaxation is the fused
        step's arithmetic, the same bits; f is held to the contract of one step."""
        a, b = Nutrient.open(d, family, form), Nutrient.open(d, family, form)
        a.run(1)
        if form[1]:                                         # (the streamed density is that of the lattice BEFORE lb_move, as the fused step has it)
            b.update_velocity(streamed=True)
        b.move(), b.move_bcs(), b.update_hydro()
        if not form[1]:
            b.update_velocity(streamed=False)
        b.update_forces(), b.update_feq(), b.collide_particles()
        fused, staged = Nutrient.got(a), Nutrient.got(b)
        a.close(), b.close()
        bad = same_bits(fused, staged, [k for k in staged if k != "f"])
        assert not bad, bad
        assert maxratio(fused["f"], staged["f"], contract_tol(1)["f"])[0] <= 1.


class Expansion:
    keys = staticmethod(lambda form: ("f", "rho"))
    model_form = staticmethod(lambda form: form)
    NOISE_SEED = 40

    @staticmethod
    def inputs(family, form, nx, ny):
        from test_gpu_expansion import smooth_case
        f0, u, v = smooth_case(nx, ny, form, seed_of(nx, ny))
        return dict(nx=nx, ny=ny, ns=form, f0=f0, u=u, v=v)

    @staticmethod
    def model(d, family, form, dtype):
        """the strains draw from the stream under their own seeds (noise_model.normals64 rounded to float32): the draw is fixed"""
        from expansion_model import ExpansionModel
        from test_gpu_expansion import CUT, DGS, GS, OMEGAS
        ns = d["ns"]
        m = ExpansionModel(d["nx"], d["ny"], OMEGAS[:ns], 1.3, GS[:ns], DGS[:ns], [Expansion.NOISE_SEED + i for i in range(ns)], CUT, family,
                           dtype, milstein="single")
        m.set_f(d["f0"])
        m.set_fields(np.zeros((d["nx"], d["ny"], ns + 1), F), d["u"], d["v"])
        return m

    state = staticmethod(lambda m: m.get_fields())
    bounds = staticmethod(lambda d, m, n, want: plain_tol(n))

    @staticmethod
    def open(d, family, form):
        from test_gpu_expansion import DGS, GS, OMEGAS, set_of
        ns = d["ns"]
        return set_of(d["nx"], d["ny"], OMEGAS[:ns], 1.3, GS[:ns], DGS[:ns], Expansion.NOISE_SEED, d["f0"], d["u"], d["v"], family)

    @staticmethod
    def got(s):
        from test_gpu_expansion import state
        return state(s)

    twice = staticmethod(lambda d, family, form: None)


MODELLED = dict(scalar=Scalar, noisy=Noisy, multifield=Multifield, poisson=Poisson, porous=Porous, multifluid=Multifluid, rocket=Rocket,
                nutrient=Nutrient, expansion=Expansion)


@functools.lru_cache(maxsize=None)
def reference(kind, family, model_form, nx, ny, dtype=np.float64):
    """{n: the model's arrays after n steps} for n in STEPS, computed once per box and shared; read-only."""
    K = MODELLED[kind]
    form = next(f for f in L4.KINDS[kind]["forms"] if K.model_form(f) == model_form)
    d = K.inputs(family, form, nx, ny)
    m = K.model(d, family, form, dtype)
    out, done = {}, 0
    for n in STEPS:
        with np.errstate(all="ignore"):
            m.run(n - done)
        done = n
        out[n] = {k: np.array(v, copy=True) for k, v in K.state(m).items() if k in K.keys(form)}
        for a in out[n].values():
            a.setflags(write=False)
    return out, m


def modelled_cases():
    return [pytest.param(kind, *case, id="%s-%s" % (kind, L4.case_id(case))) for kind in MODELLED for case in L4.cases(kind)]


# ---- against the model, and against the product's second computation -------------------------------------------------------------
@pytest.mark.parametrize("kind, family, form, nx, ny", modelled_cases())
def test_follows_the_model(lbhip, kind, family, form, nx, ny):
    K = MODELLED[kind]
    d = K.inputs(family, form, nx, ny)
    want, m = reference(kind, family, K.model_form(form), nx, ny)
    cls = L4.classify(nx, ny, L4.rows_of(kind))
    for runs in getattr(K, "RUNS", ((1, 1, 3),)):
        s = K.open(d, family, form)
        try:
            done = 0
            for n in runs:
                s.run(n)
                done += n
                hold(kind, "%s %s %s %dx%d (c=%d tiles=%s edge_lane=%s rows=%s) after %d step(s), handle / float64 model"
                     % (kind, family, form, nx, ny, cls["c"], cls["tiles"], cls["edge_lane"], cls["rows"], done),
                     K.bounds(d, m, done, want[done]), K.got(s), want[done], K.keys(form))
        finally:
            s.close()


@pytest.mark.parametrize("kind, family, form, nx, ny",
                         [p for p in modelled_cases() if p.values[0] in ("scalar", "noisy", "poisson", "porous", "multifluid", "rocket", "nutrient")
                          and p.values[:3:2] != ("scalar", "K_STEP")          # (k_ad_step is the yardstick of k_ad_tile4)
                          and p.values[3:] in L4.table(p.values[0], p.values[1], "new")])     # (a kind's old boxes: its own file holds these bits)
def test_computed_twice_gives_the_same_bits(lbhip, kind, family, form, nx, ny):
    K = MODELLED[kind]
    K.twice(K.inputs(family, form, nx, ny), family, form)


PHASES = dict(scalar=lambda s: (s.move(), s.move_bcs(), s.update_hydro(), s.update_feq(), s.collide_particles()),
              multifield=lambda s: (s.move(), s.move_bcs(), s.update_hydro(), s.update_feq(), s.collide_particles()),
              expansion=lambda s: s.step_phases())
PHASES["noisy"] = PHASES["scalar"]                          # (without a noise field the un-fused collision draws from the stream itself)


@pytest.mark.parametrize("kind, family, form, nx, ny",
                         [p for p in modelled_cases() if p.values[0] in PHASES and p.values[2] not in ("TILES", "cell")      # (run(1) is k_ad_step under every word)
                          and p.values[3:] in L4.table(p.values[0], p.values[1], "new")])
def test_fused_step_follows_the_phases(lbhip, kind, family, form, nx, ny):
    """The kinds whose un-fused phases round the relaxation differently from the fused step: two steps, one by one, held to the contract
    (as tests/test_gpu_noise.py and tests/test_gpu_expansion.py hold theirs)."""
    K = MODELLED[kind]
    d = K.inputs(family, form, nx, ny)
    a, b = K.open(d, family, form), K.open(d, family, form)
    try:
        for n in (1, 2):
            a.run(1)
            PHASES[kind](b)
            hold(kind + " phases", "%s %s %s %dx%d after %d step(s), fused / phases" % (kind, family, form, nx, ny, n), plain_tol(n),
                 K.got(a), K.got(b), ("f", "rho"))
    finally:
        a.close(), b.close()


# ---- Poisson: the reduction ------------------------------------------------------------------------------------------------------
def poisson_boxes():
    return L4.table("poisson", "dirichlet")


def poisson_ratio(nx, ny, poison):
    """test_gpu_poisson.test_device_ratio_is_the_float64_ratio_of_the_box at any box.  The poison: f1 of the east column, which leaves the
    box and is read by nothing but the first padding column's pull, is NaN before two warm-up iterations; they turn the padding of the
    populations and of rho into NaN and leave every cell of the box as it was.  Data only: every access is the unpoisoned run's."""
    from test_gpu_poisson import sim_of
    d = Poisson.inputs("dirichlet", "solve", nx, ny)
    clean = sim_of(d, tolerance=0.)
    if poison:
        d = dict(d, f0=d["f0"].copy())
        d["f0"][-1, :, 1] = np.nan
    s = sim_of(d, tolerance=0.)
    try:
        for x in (s, clean):
            x.run(2)
        old = s.get_fields(("rho",))["rho"]
        done, converged, ratio = s.solve(1)
        clean.solve(1)
        new, ref = s.get_fields(("f", "rho")), clean.get_fields(("f", "rho"))
    finally:
        s.close(), clean.close()
    assert np.all(np.isfinite(new["rho"])) and not same_bits(new, ref)
    want = np.abs(new["rho"].astype(np.float64) - old).sum() / old.astype(np.float64).sum()
    print("%dx%d%s: device ratio %.9e, float64 %.9e, relative difference %.2e / 1e-5"
          % (nx, ny, " poisoned" if poison else "", ratio, want, abs(ratio - want) / want))
    assert (done, converged) == (1, False) and abs(ratio - want) <= 1e-5 * want


@pytest.mark.parametrize("nx, ny", poisson_boxes(), ids=lambda v: str(v))
def test_poisson_device_ratio_is_the_float64_ratio_of_the_box(lbhip, nx, ny):
    poisson_ratio(nx, ny, False)


@pytest.mark.parametrize("nx, ny", [b for b in poisson_boxes() if (b[0] - 1) % 4 in (1, 2)], ids=lambda v: str(v))
def test_poisson_device_ratio_leaves_out_one_or_two_poisoned_padding_cells(lbhip, nx, ny):
    """c = 1 and c = 2: the sums of k_ps_step<true> leave out exactly two cells and one cell of the edge lane"""
    poisson_ratio(nx, ny, True)


# ---- the carried scalars: the twin sequence, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("family, form, nx, ny", L4.cases("advected"), ids=[L4.case_id(c) for c in L4.cases("advected")])
def test_advected_set_equals_its_twin_sequence(lbhip, family, form, nx, ny):
    import test_gpu_advected as A
    which, ns = form
    want = A.twin(lbhip, nx, ny, ns)
    for runs in ((1, 2), (2,)):                             # (the twin's snapshots at 1, 2, 3: LAST alone; a launch that is not the last, then LAST)
        st = A.make_set(nx, ny, ns)
        try:
            done = 0
            for n in runs:
                st.run(n, form=which)
                done += n
                A.assert_same(A.set_state(st), want[done], "%dx%d, %d scalar(s), form %d, %d step(s)" % (nx, ny, ns, which, done))
        finally:
            st.close()
