"""The set calls' refusals, swept: which status and which sentence wins when a set breaks one rule, or two at once.

Six families of entry points take an array of handles -- lb_*_coupled, lb_*_fluids, lb_*_rocket, lb_*_nutrient, lb_*_expansion and
lb_run_batch.  Each checks its array, its count and its members before it touches the device, and where a family's checks stand
relative to each other decides which sentence a caller reads.  The contract, per member: the coupled, fluid, rocket and nutrient sets
test null, rocket (where the family names it), kind, shared geometry, split step, duplicate; the expansion null, rocket, kind,
duplicate, family, shared geometry, and the whole-grid and split rules only behind the cutoff, the nutrient's growth rate and the
seeds; lb_run_coupled names a porous, multifluid or rocket member before anything else.  Around the members: the expansion tests null
parameters between the null array and the count; the nutrient set its members, then the solver, then the parameters; lb_set_rocket
and the fluids' tables their members, then the parameters.  set_refusals.json holds what the library answered to every call of
the sweep below: each distinct (status, message) once, the calls as indices into that list (-1: the call was not refused).  The test
holds the library to the status and the message, byte for byte, of every refused call, to accepting the others, and to every set
being finite afterwards -- what a change to how set calls check their members has to keep.

Rules the sweep cannot reach, so that no recorded answer is theirs: "inside a split step" of the coupled, rocket, nutrient and
expansion sets and "only available on handles that own the whole grid" (lb_step_boundary and lb_create refuse these kinds: only a
flow handle can be split, which lb_run_batch's answer records); the expansion's "neither open nor periodic" (a scalar lattice has
no other family); a second device (one GPU); the clumpy nutrient's "nx, ny >= 3" (every grid here has interior cells).
"Finite afterwards" is Simulation.check() on every member, except on a fluid of a multicomponent set, a kind lb_check refuses: there
it is every value of f, rho, u and v read back.

The sweep, per family and per entry point, on 8 x 6 handles (the smallest grid every kind accepts that still has interior cells):
a good set of the family's largest size with one member, and two members at two different positions, replaced by intruders -- a
null pointer, the set's first handle again, a whole-grid GPU handle of every semantics, a CPU-backend handle, the right kind at
9 x 6, in the family's other boundary family and with the planar layout, a flow handle inside a split step --; the counts -1, 0, 1,
max and max + 1; the null array; null parameters; and the rules only the family has (SWEEPS below).  Calls that are not refused run
for n_steps = 0 (runs) or once (stages).
"""
import ctypes as ct
import itertools
import json
import os

import numpy as np
import pytest

from conftest import ROOT       # noqa: F401  (puts the package on the path when this file runs as a script: record())
from LB_D2Q9 import _native

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "set_refusals.json")
NX, NY = 8, 6
W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
NAN, INF = float("nan"), float("inf")
# family -> (semantics, boundary family, the family's other boundary family, largest set)
FAMILIES = dict(coupled=("multifield", "periodic", "box", 4), fluids=("multifluid", "periodic", "zero_gradient", 3),
                rocket=("rocket", "periodic", None, 2), nutrient=("diffusion", "periodic", "open", 2),
                expansion=("diffusion", "open", "periodic", 4), batch=("opencl", "periodic", "pipe", 8))
OTHERS = (("opencl", "periodic"), ("diffusion", "periodic"), ("multifield", "periodic"), ("poisson", "dirichlet"), ("porous", "periodic"),
          ("multifluid", "periodic"), ("rocket", "periodic"))


class World(object):
    """Every handle of the sweep, made once; made, swept and closed in one order so that the recorded run and the tested run agree."""

    def __init__(self, L):
        from LB_D2Q9.simulation import Simulation
        self.L, self.all = L, []

        def handle(semantics, bc, nx=NX, planar=False, device=0, rho=0.2):
            s = Simulation(nx, NY, 1.0, bc=bc, semantics=semantics, planar=planar, device=device)
            self.all.append(s)
            if device >= 0:
                s.set_f((W * rho * np.ones((nx, NY, 1))).astype(np.float32))
                s.update_hydro()
            return s

        self.handle = handle
        # the intruders every family meets: (name, handle or None); "first" stands for the set's own first handle
        self.common = [("null", None), ("first", "first")] + [(sem, handle(sem, bc)) for sem, bc in OTHERS]
        noisy = handle("diffusion", "periodic")
        _native.check(L.lb_set_noise(noisy._h, 1.0e-3, 99))
        split = handle("opencl", "periodic")
        _native.check(L.lb_step_boundary(split._h, 0))
        self.common += [("noisy diffusion", noisy), ("cpu", handle("cython", "pipe", device=_native.LB_DEVICE_CPU)), ("split", split)]
        self.sets, self.intruders = {}, {}
        for family, (sem, bc, other, most) in FAMILIES.items():
            self.sets[family] = [handle(sem, bc) for _ in range(most + 1)]       # (the last one: only ever behind a count of max + 1)
            own = [("9 x 6", handle(sem, bc, nx=NX + 1)), ("planar", handle(sem, bc, planar=True))]
            if other:
                own.append(("other family", handle(sem, other)))
            self.intruders[family] = self.common + own
        strains = self.sets["expansion"][:3]
        for i, s in enumerate(strains):
            _native.check(L.lb_set_noise(s._h, 1.0e-3, 41 + i))
        self.sp = ct.c_void_p()
        _native.check(L.lb_spectral_create(NX, NY, 0, 2.0, ct.byref(self.sp)))

    def array(self, family, replaced=()):
        """the family's good set with the members at `replaced` positions exchanged for intruders: (position, intruder index) pairs"""
        good = self.sets[family]
        hs = [s._h.value for s in good]
        for at, k in replaced:
            x = self.intruders[family][k][1]
            hs[at] = None if x is None else good[0]._h.value if x == "first" else x._h.value
        return (ct.c_void_p * len(hs))(*hs)

    def feq_everywhere(self, family):
        for s in self.sets[family]:
            s.update_feq()

    def finite(self):
        def bad(s):
            if s.semantics == "multifluid":         # (lb_check refuses the kind: the populations and the fields themselves)
                return int(sum((~np.isfinite(a)).sum() for a in s.get_fields(("f", "rho", "u", "v")).values()))
            return s.check()["n_nonfinite"]
        return {family: [bad(s) for s in good] for family, good in self.sets.items()}

    def close(self):
        self.L.lb_spectral_destroy(self.sp)
        for s in self.all:
            s.close()


def replacements(most, n_intruders):
    """none; every single replacement; every pair of replacements at two different positions"""
    yield ()
    for at in range(most):
        for k in range(n_intruders):
            yield ((at, k),)
    for a, b in itertools.combinations(range(most), 2):
        for k, m in itertools.product(range(n_intruders), repeat=2):
            yield ((a, k), (b, m))


def members_sweep(w, family, entry_points):
    """what every family is swept over: (label, call) with call() -> status"""
    most = FAMILIES[family][3]
    for name, ep in entry_points:
        for r in replacements(most, len(w.intruders[family])):
            yield "%s %r" % (name, [(at, w.intruders[family][k][0]) for at, k in r]), (lambda ep=ep, r=r: ep(w.array(family, r), most))
        for count in (-1, 0, 1, most, most + 1):
            yield "%s count %d" % (name, count), (lambda ep=ep, count=count: ep(w.array(family), count))
        yield "%s null array" % name, (lambda ep=ep: ep(None, most))


def broken_sets(w, family):
    """(label, array, count): the good set and sets that break one rule of the member check each, to pair with broken parameters --
    which of the two the caller reads pins where the parameter checks stand"""
    most = FAMILIES[family][3]
    yield "the good set", w.array(family), most
    yield "null array", None, most
    for count in (-1, 1, most + 1):
        yield "count %d" % count, w.array(family), count
    for k, (name, _) in enumerate(w.intruders[family]):
        for at in (0, most - 1):
            yield "%s at %d" % (name, at), w.array(family, ((at, k),)), most


def coupled(w):
    L, f = w.L, w.array("coupled")
    yield "collide before feq", lambda: L.lb_collide_coupled(f, 4)
    w.feq_everywhere("coupled")
    yield "negative steps", lambda: L.lb_run_coupled(f, 4, -1)
    for x in members_sweep(w, "coupled", (("lb_run_coupled", lambda a, c: L.lb_run_coupled(a, c, 0)), ("lb_collide_coupled", L.lb_collide_coupled))):
        yield x


def fluids(w):
    L, f = w.L, w.array("fluids")
    eps = (("lb_run_fluids", lambda a, c: L.lb_run_fluids(a, c, 0)), ("lb_set_interactions", lambda a, c: L.lb_set_interactions(a, c, None, 0)),
           ("lb_set_reactions", lambda a, c: L.lb_set_reactions(a, c, None, 0)), ("lb_update_forces_fluids", L.lb_update_forces_fluids),
           ("lb_update_bary_fluids", L.lb_update_bary_fluids), ("lb_react_fluids", L.lb_react_fluids))
    yield "negative steps", lambda: L.lb_run_fluids(f, 3, -1)
    yield "null interactions", lambda: L.lb_set_interactions(f, 3, None, 1)
    yield "null reactions", lambda: L.lb_set_reactions(f, 3, None, 1)
    for x in members_sweep(w, "fluids", eps):
        yield x
    beyond, unknown = _native.Interaction(0, 5, _native.LB_PSI_LINEAR, 0, 0.1, 0.), _native.FluidReaction(9, 0, 0, 0.01, 0., 0.)
    for label, a, c in broken_sets(w, "fluids"):
        yield "lb_set_interactions null table, " + label, (lambda a=a, c=c: L.lb_set_interactions(a, c, None, 1))
        yield "lb_set_interactions fluid 5, " + label, (lambda a=a, c=c: L.lb_set_interactions(a, c, ct.byref(beyond), 1))
        yield "lb_set_reactions null table, " + label, (lambda a=a, c=c: L.lb_set_reactions(a, c, None, 1))
        yield "lb_set_reactions unknown kind, " + label, (lambda a=a, c=c: L.lb_set_reactions(a, c, ct.byref(unknown), 1))
    # a table entry naming a fluid beyond the count: the table of a set of three, then every call on its first two and its first
    inter = _native.Interaction(0, 2, _native.LB_PSI_LINEAR, 0, 0.1, 0.)
    yield "a table for three", lambda: L.lb_set_interactions(f, 3, ct.byref(inter), 1)
    for (name, ep), count in itertools.product(eps, (3, 2, 1)):
        if not (count == 3 and name.startswith("lb_set")):          # (that would clear the table)
            yield "%s count %d under the interaction table" % (name, count), (lambda ep=ep, count=count: ep(f, count))
    yield "no table", lambda: L.lb_set_interactions(f, 3, None, 0)
    react = _native.FluidReaction(_native.LB_REACT_GROW, 2, 0, 0.01, 0., 0.)
    yield "reactions for three", lambda: L.lb_set_reactions(f, 3, ct.byref(react), 1)
    for (name, ep), count in itertools.product(eps, (3, 2, 1)):
        if not (count == 3 and name.startswith("lb_set")):
            yield "%s count %d under the reaction table" % (name, count), (lambda ep=ep, count=count: ep(f, count))
    yield "no reactions", lambda: L.lb_set_reactions(f, 3, None, 0)


def rocket(w):
    L, f = w.L, w.array("rocket")
    P = lambda mode=_native.LB_ROCKET_FLOW, G=0.01, rho_o=0.9, c_o=0.25: ct.byref(_native.RocketParams(mode, G, 0.02, 0.5, rho_o, -0.8, c_o, 2.))
    yield "collide before feq", lambda: L.lb_collide_rocket(f, 2)
    w.feq_everywhere("rocket")
    yield "the parameters", lambda: L.lb_set_rocket(f, 2, P())
    yield "negative steps", lambda: L.lb_run_rocket(f, 2, -1)
    yield "null parameters", lambda: L.lb_set_rocket(f, 2, None)
    yield "unknown mode", lambda: L.lb_set_rocket(f, 2, P(mode=7))
    yield "non-finite parameter", lambda: L.lb_set_rocket(f, 2, P(G=NAN))
    yield "FLOW with rho_o = 0", lambda: L.lb_set_rocket(f, 2, P(rho_o=0.))
    yield "FORCES with c_o = 0", lambda: L.lb_set_rocket(f, 2, P(mode=_native.LB_ROCKET_FORCES, c_o=0.))
    eps = (("lb_set_rocket", lambda a, c: L.lb_set_rocket(a, c, P())), ("lb_run_rocket", lambda a, c: L.lb_run_rocket(a, c, 0)),
           ("lb_update_velocity_rocket", L.lb_update_velocity_rocket), ("lb_update_forces_rocket", L.lb_update_forces_rocket),
           ("lb_collide_rocket", L.lb_collide_rocket), ("lb_get_rocket_fields", lambda a, c: L.lb_get_rocket_fields(a, c, None, None, None, None, None)))
    for x in members_sweep(w, "rocket", eps):
        yield x
    for label, a, c in broken_sets(w, "rocket"):
        for what, p in (("null parameters", lambda: None), ("unknown mode", lambda: P(mode=7)), ("non-finite parameter", lambda: P(G=NAN))):
            yield "lb_set_rocket %s, %s" % (what, label), (lambda a=a, c=c, p=p: L.lb_set_rocket(a, c, p()))


def nutrient(w):
    L, f, sp = w.L, w.array("nutrient"), w.sp
    P = lambda G=0.01, scale=0.5, clumpy=0, rho_o=0.9: ct.byref(_native.NutrientParams(G, scale, clumpy, rho_o, -0.8))
    eps = (("lb_run_nutrient", lambda a, c, **kw: L.lb_run_nutrient(sp, a, c, P(**kw), 0)),
           ("lb_nutrient_velocity", lambda a, c, **kw: L.lb_nutrient_velocity(sp, a, c, kw.get("scale", 0.5), 0)),
           ("lb_update_forces_nutrient", lambda a, c, **kw: L.lb_update_forces_nutrient(a, c, P(**dict(dict(clumpy=1), **kw)))),
           ("lb_collide_nutrient", lambda a, c, **kw: L.lb_collide_nutrient(a, c, P(**kw))),
           ("lb_get_nutrient_fields", lambda a, c, **kw: L.lb_get_nutrient_fields(a, c, None, None, None)))
    yield "collide before feq", lambda: L.lb_collide_nutrient(f, 2, P())
    w.feq_everywhere("nutrient")
    yield "clumpy collide before the forces", lambda: L.lb_collide_nutrient(f, 2, P(clumpy=1))
    yield "forces of the plain variant", lambda: L.lb_update_forces_nutrient(f, 2, P())
    yield "negative steps", lambda: L.lb_run_nutrient(sp, f, 2, P(), -1)
    for name, ep in eps:
        for kw in (dict(clumpy=1, rho_o=0.), dict(G=NAN), dict(scale=INF), dict(clumpy=1)):
            yield "%s %r" % (name, kw), (lambda ep=ep, kw=kw: ep(f, 2, **kw))
    for name, call in (("lb_run_nutrient", lambda sp_, p: L.lb_run_nutrient(sp_, f, 2, p, 0)), ("lb_nutrient_velocity", lambda sp_, p: L.lb_nutrient_velocity(sp_, f, 2, 0.5, 0)),
                       ("lb_update_forces_nutrient", lambda sp_, p: L.lb_update_forces_nutrient(f, 2, p)), ("lb_collide_nutrient", lambda sp_, p: L.lb_collide_nutrient(f, 2, p))):
        yield name + " null solver", (lambda call=call: call(None, P(clumpy=1)))
        yield name + " null parameters", (lambda call=call: call(sp, None))
    open_pair = (ct.c_void_p * 2)(*[s._h.value for s in w.sets["expansion"][3:5]])        # (two of one geometry, neither noisy)
    for name, ep in eps:
        yield name + " on two open lattices", (lambda ep=ep: ep(open_pair, 2))
    member = w.sets["nutrient"][1]
    yield "noise on", lambda: L.lb_set_noise(member._h, 1.0e-3, 7)
    for name, ep in eps:
        yield name + " with a noisy member", (lambda ep=ep: ep(f, 2))
    yield "noise off", lambda: L.lb_set_noise(member._h, 0., 7)
    for x in members_sweep(w, "nutrient", eps):
        yield x
    # members, then the solver, then the parameters: each pair of them broken at once, and all three
    for label, a, c in broken_sets(w, "nutrient"):
        for solver, p, what in ((None, P, "null solver"), (sp, lambda: None, "null parameters"), (None, lambda: None, "null solver and parameters"),
                                (sp, lambda: P(G=NAN), "non-finite parameter"), (None, lambda: P(G=NAN), "null solver, non-finite parameter")):
            yield "lb_run_nutrient %s, %s" % (what, label), (lambda a=a, c=c, solver=solver, p=p: L.lb_run_nutrient(solver, a, c, p(), 0))
            if solver is not None:
                yield "lb_update_forces_nutrient %s, %s" % (what, label), (lambda a=a, c=c, p=p: L.lb_update_forces_nutrient(a, c, p()))
                yield "lb_collide_nutrient %s, %s" % (what, label), (lambda a=a, c=c, p=p: L.lb_collide_nutrient(a, c, p()))
        for solver, scale, what in ((None, 0.5, "null solver"), (sp, INF, "non-finite factor"), (None, INF, "null solver, non-finite factor")):
            yield "lb_nutrient_velocity %s, %s" % (what, label), (lambda a=a, c=c, solver=solver, scale=scale: L.lb_nutrient_velocity(solver, a, c, scale, 0))


def expansion(w):
    L, f = w.L, w.array("expansion")
    P = lambda cut=1.0e-4: ct.byref(_native.ExpansionParams(cut))
    eps = (("lb_run_expansion", lambda a, c, cut=1.0e-4: L.lb_run_expansion(a, c, P(cut), 0)),
           ("lb_update_hydro_expansion", lambda a, c, cut=1.0e-4: L.lb_update_hydro_expansion(a, c, P(cut))),
           ("lb_collide_expansion", lambda a, c, cut=1.0e-4: L.lb_collide_expansion(a, c, P(cut))))
    a, b, _, nut = w.sets["expansion"][:4]
    zeros = np.zeros((NY, NX), np.float32)
    yield "collide before feq", lambda: L.lb_collide_expansion(f, 4, P())
    w.feq_everywhere("expansion")
    yield "negative steps", lambda: L.lb_run_expansion(f, 4, P(), -1)
    yield "null parameters", lambda: L.lb_run_expansion(f, 4, None, 0)
    states = (("a non-finite cutoff", None, None),
              ("the nutrient grows", lambda: L.lb_set_reaction(nut._h, 0.01), lambda: L.lb_set_reaction(nut._h, 0.)),
              ("the nutrient draws", lambda: L.lb_set_noise(nut._h, 1.0e-3, 77), lambda: L.lb_set_noise(nut._h, 0., 77)),
              ("two strains with one seed", lambda: L.lb_set_noise(b._h, 1.0e-3, 41), lambda: L.lb_set_noise(b._h, 1.0e-3, 42)),
              ("a member holds a noise field", lambda: L.lb_set_noise_field(a._h, zeros.ctypes.data, 0), lambda: L.lb_set_noise_field(a._h, None, 0)))
    for what, on, off in states:
        if on:
            yield what + ": on", on
        for name, ep in eps:
            for cut in ((NAN, INF) if not on else (1.0e-4,)):
                yield "%s, %s %r" % (name, what, cut), (lambda ep=ep, cut=cut: ep(f, 4, cut))
            # (two rules at once: which of them the caller reads)
            yield "%s, %s and a non-finite cutoff" % (name, what), (lambda ep=ep: ep(f, 4, NAN))
            yield "%s, %s and a member twice" % (name, what), (lambda ep=ep: ep(w.array("expansion", ((2, 1),)), 4))
        if off:
            yield what + ": off", off
    for x in members_sweep(w, "expansion", eps):
        yield x
    # null parameters stand between the null array and the count; the cutoff behind the members
    raw = (("lb_run_expansion", lambda a, c, p: L.lb_run_expansion(a, c, p, 0)), ("lb_update_hydro_expansion", L.lb_update_hydro_expansion),
           ("lb_collide_expansion", L.lb_collide_expansion))
    for (name, ep), (label, a, c) in itertools.product(raw, broken_sets(w, "expansion")):
        yield "%s null parameters, %s" % (name, label), (lambda ep=ep, a=a, c=c: ep(a, c, None))
        yield "%s non-finite cutoff, %s" % (name, label), (lambda ep=ep, a=a, c=c: ep(a, c, P(NAN)))


def batch(w):
    L, f = w.L, w.array("batch")
    yield "negative steps", lambda: L.lb_run_batch(f, 8, -1)
    for x in members_sweep(w, "batch", (("lb_run_batch", lambda a, c: L.lb_run_batch(a, c, 0)),)):
        yield x


SWEEPS = (coupled, fluids, rocket, nutrient, expansion, batch)


def answers(L):
    """(label, status, message) of every call of the sweep, in its order, and how many non-finite cells every set holds afterwards"""
    w = World(L)
    try:
        out = []
        for family in SWEEPS:
            for label, call in family(w):
                rc = call()
                out.append(("%s: %s" % (family.__name__, label), rc, L.lb_last_error().decode() if rc else ""))
        return out, w.finite()
    finally:
        w.close()


@pytest.mark.gpu
def test_every_set_refusal_keeps_its_status_and_message(lbhip):
    with open(TABLE) as fh:
        table = json.load(fh)
    got, nonfinite = answers(lbhip)
    assert len(table["index"]) == len(got)
    wrong = []
    for (label, rc, message), i in zip(got, table["index"]):
        want = (0, "") if i < 0 else tuple(table["answers"][i])
        if (rc, message) != want:
            wrong.append((label, want, (rc, message)))
    assert not wrong, "%d of %d calls (call, recorded, now), the first: %r" % (len(wrong), len(got), wrong[:5])
    assert sum(i >= 0 for i in table["index"]) > len(got) // 2 and sum(i < 0 for i in table["index"]) > 50
    assert not any(n for ns in nonfinite.values() for n in ns), nonfinite


def record():
    """Writes set_refusals.json.  Run by hand on an MI355X with LB_LIB=<the liblbhip.so of the commit to record>:
        LB_LIB=... python tests/test_gpu_set_refusals.py
    The committed table was recorded at e81b10e ("Add Expansion: noisy strains on a shared nutrient, one launch per step"), whose
    set calls this test came with: no later change to them has been recorded."""
    got, nonfinite = answers(_native.lib())
    assert not any(n for ns in nonfinite.values() for n in ns), nonfinite
    found, index = [], []
    for _, rc, message in got:
        if rc and [rc, message] not in found:
            found.append([rc, message])
        index.append(found.index([rc, message]) if rc else -1)
    with open(TABLE, "w") as fh:
        json.dump(dict(answers=found, index=index), fh, separators=(",", ":"), indent=None)
        fh.write("\n")
    return found, sum(i >= 0 for i in index), len(index)


if __name__ == "__main__":
    found, refused, calls = record()
    for rc, message in found:
        print(rc, message)
    print("%d distinct answers, %d of %d calls refused" % (len(found), refused, calls))
