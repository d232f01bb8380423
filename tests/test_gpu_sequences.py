"""Random call sequences on every handle kind against the models (the generator and the players: tests/sequence_scenarios.py).

The other GPU files meet one entry point with one reference at a time.  Between those points sits host state that decides which
kernel runs on which buffer and what a read returns -- the current lattice, macro_valid / feq_valid, the captured graph's key, the
mask and field flags, the `G != 0` template switch, the multifluid variant word, the edge and corner states, the Poisson iteration
counter, the last launch that alone stores u, v, G -- each correct for the sequences somebody thought of.  Here a handle lives
through a seeded interleaving of its calls, and two properties are held at two cut points inside the sequence and at its end:

  A, bitwise    the SUBJECT (effective and transparent ops, starting from the automatic variant) equals the TWIN (a second handle
                pinned to the plainest kernel that makes the effective ops only, every run(n) as n x run(1)) on every array the kind
                exposes: an observation or a kernel choice never changes the trajectory.
  B, contract   the twin equals the REFERENCE (oracle.O2Sim for the flow kinds, the kind's numpy model in float64 otherwise) within
                the kind's existing comparison for the n steps since the populations were last set: a state-changing call in the
                middle of a life means what the reference says it means.  No new tolerance.

The comparisons follow a stepping op, where every array is fresh, or a set_f behind one, where the populations are new and rho, u, v,
feq and the forces are still the last step's (the populations are then held to the bound of the steps since they were set, the rest
to that of the steps behind it).  On a Poisson handle the iteration count is held to the model's as well; on the noisy kinds the
noise counters of the subject, the twin and the model are equal at every cut.

The kinds that came later -- rocket, nutrient, noise, expansion, screened -- have host state of their own between their entry points:
parameters stored with a set's first member or sent with every call, `clumpy` toggled in the middle of a life, psi / S and the forces
"of the last step", a solver handle that keeps arrays between calls, one noise counter per strain that restarts on set_noise, stands
still at Dg = 0, is advanced by a collision fed a supplied field and carried through a checkpoint by either class.  Where their twin has
no plainer kernel to be pinned to (nutrient, expansion, screened) it differs from the subject in run(n) made as n x run(1), which puts
"the last launch stores" on every launch.  Every cell is compared: no mask, no NaN allowance (tests/test_sequences_cpu.py holds
the references finite and far from every threshold of the collisions).

Shapes: sequence_scenarios.FLOW_SHAPES and its neighbours, with the reason for each.  That the references alone stay inside the
contract on exactly these inputs: tests/test_sequences_cpu.py.

Measured on an MI355X, all 102 cases green, the largest share of its bound that property B used per kind: flow f 95 % (velocity inlet,
seed 5, the one step by phases behind an init_equilibrium: 2.38e-7 of 2.5e-7), rho 60 %, u 17 %, v 8 %; scalar f 43 %, rho 31 %, feq
27 %; multifield f 12 %, rho 8 %, feq 8 %; poisson f 19 %, rho 14 %, feq 20 %; porous f 56 %, feq 40 %, rho 42 %, u, v, u_b, G 5 %;
multifluid f 60 %, feq 40 %, rho 41 %, u, v, u_b, G 5 %.  The flow cases take up to half a second each, the others less.
The 60 cases of the later kinds, all green: rocket f 33 %, feq 28 %, rho 29 %, u 3 %, v 2 %, psi / S 8 %, the forces 2 %; nutrient f 50 %,
feq 36 %, rho 38 %, u 3 %, v < 1 %, psi 10 %, F 1 %; noise f 40 %, rho 26 %, feq 26 %; expansion f 52 %, rho 35 %, feq 35 %; screened f 27 %,
rho 31 %, feq 29 %, u 2 %, v 1 %.  A kind's twelve cases take 1.6 s (noise) to 4.2 s (expansion) together: 0.35 s a case at the most.

The kind 'advected' (a flow and the 1 ... 2 scalars it carries: lb_run_advected, coupled.Advected_Scalars) has a driver of its own,
test_random_call_sequence_of_a_carried_set, since its members are unlike lattices that also live as ordinary handles between the set's
runs: runs of the set in either form and of one member alone (a flow run of more than 16 steps in every life: the captured graph
replays behind a set run of either parity), set_f on a member, init_equilibrium on the flow, a scalar's growth rate switched between 0
and non-zero and back between set runs, set_fields on a scalar with its own run behind it; variant words on the flow in front of a set
run of form 0 and of its own run, tile shapes on a scalar, reads of every member and of the set, a checkpoint through a closed set.
Families: the flow handle's flag.  A lazy flow whose fields are those of its own run holds rho, u, v rebuilt from the post-collision
populations -- the eager twin's moments, not its bits --: there, and only there, the flow's rho, u, v, feq are held bitwise to a fresh lazy
handle given the twin's populations.  Property B uses the two existing contracts unchanged: the flow against O2Sim, every scalar against
its float64 model fed, step by step, the velocity the twin stored.  Measured on an MI355X, twelve cases green in 2.6 s (0.27 s at the
most), the largest share of its bound: the flow's f 60 %, rho 48 %, u 6 %, v 6 %; a scalar's f 50 %, rho 28 %, feq 26 %.  The defects tried
against it: the table in tests/test_gpu_advected.py.

One-line defects tried against this file (value-changing only; none kept), with the cases each turned red:
  lb_set_f without its ensure_macro                                      ->  4 (flow: pipe 3, periodic 1 and 3, cavity 4 -- lazy
                                                                            families, compared behind a set_f; one by A, three by B)
  the captured graph's key without its `cur` bit                         ->  3 (flow: pipe 4, cavity 4, velocity_inlet 4, by A: the graph
                                                                            replays only under a forced K_STEP in runs of > 16 steps)
  lb_run_fluids' one-launch step storing u, v, G, u_b on the FIRST launch -> 12 of 12 multifluid
  lb_set_reaction ignoring a change back to G = 0                        ->  7 of 12 scalar (six by B, one by A)
  lb_solve_reset leaving the iteration counter                           ->  5 of 6 poisson (the count held to the model's)
  lb_set_mask(NULL) leaving has_mask set                                 -> 35 of 48 flow
  run_porous storing rho, u, v, G, u_b on the FIRST launch               -> 12 of 12 porous
  lb_run_coupled storing every field's rho on the FIRST launch           -> 12 of 12 multifield
  lb_set_corner_state without its upload                                 -> 14 (5 of 6 multifield box, 5 of 6 poisson, 4 of 12 velocity
                                                                            inlet: wherever a restored handle gets its corner links)
and against the later kinds (each run on the kind's twelve cases):
  lb_run_expansion advancing ad_t of a strain with Dg == 0                ->  6 of 12 expansion (by the counters)
  k_ex_step storing every rho on the FIRST launch of lb_run_expansion     -> 12 of 12 expansion
  lb_set_noise leaving the noise counter                                  -> 11 of 12 noise, 8 of 12 expansion
  scalar_collide (the un-fused collision) not advancing ad_t              -> 11 of 12 noise (four by the counters alone)
  lb_run_rocket storing psi / S, u, v and the forces on the FIRST launch  -> 12 of 12 rocket
  lb_set_rocket keeping the stored parameters unless the mode changes     -> 12 of 12 rocket
  lb_run_nutrient staying clumpy once psi and the force exist             ->  9 of 12 nutrient
  k_sn_step's growth rate taken from the member, not from the call        -> 12 of 12 nutrient
  lb_run_screened solving the velocity from the stored rho, not the streamed one -> 12 of 12 screened
Not tried: defects in the Python classes (kinds._restore_diffusion without its _set_noise_counter): a library built with a defect can
stand in for the product's, a package cannot.
"""
import numpy as np
import pytest

import sequence_scenarios as S
from kernel_variants import same_bits

pytestmark = pytest.mark.gpu

CASES = [(k, f, s) for k in S.KINDS for f in S.FAMILIES[k] for s in S.SEEDS if k != "advected"]       # (a driver of its own: below)
ADVECTED_CASES = [("advected", f, s) for f in S.FAMILIES["advected"] for s in S.SEEDS]


@pytest.mark.parametrize("kind,family,seed", CASES, ids=["%s-%s-%d" % c for c in CASES])
def test_random_call_sequence(lbhip, oracle, tmp_path, kind, family, seed):
    case, ops = S.case_of(kind, family, seed), S.generate(kind, family, seed)
    cuts = S.cut_points(ops, kind, family, seed)
    subject, twin = S.GpuPlayer(case, tmpdir=tmp_path), S.GpuPlayer(case, plain=True)
    ref = S.RefPlayer(case, np.float64, oracle)
    try:
        for i, op in enumerate(ops):
            if S.is_effective(op):
                for p in (subject, twin, ref):
                    p.effective(op)
            else:
                subject.transparent(op)
            if i in cuts:
                what = "%s %s seed %d, behind op %d %r of %r" % (kind, family, seed, i, op, ops[:i + 1])
                want = twin.snapshot()
                same_bits(subject.snapshot(), want, what, fields=tuple(want))
                assert (twin.steps, twin.macro_steps) == (ref.steps, ref.macro_steps) and ref.macro_steps >= 1
                S.hold_to_contract(kind, "%s %s seed %d op %d, twin / reference" % (kind, family, seed, i), twin.fields(), ref)
                if kind == "poisson":               # the iterations since the last solve_reset: run and solve count, the phases do not
                    assert twin.h.solve_state()[0] == ref.m.iterations, (what, twin.h.solve_state(), ref.m.iterations)
                if kind in ("noise", "expansion"):  # the noisy collisions since the last set_noise, per strain: every player's the same
                    assert subject.noise_counters() == twin.noise_counters() == ref.noise_counters(), \
                        (what, subject.noise_counters(), twin.noise_counters(), ref.noise_counters())
    finally:
        subject.close()
        twin.close()


@pytest.mark.parametrize("kind,family,seed", ADVECTED_CASES, ids=["%s-%s-%d" % c for c in ADVECTED_CASES])
def test_random_call_sequence_of_a_carried_set(lbhip, oracle, tmp_path, kind, family, seed):
    """A flow and the scalars it carries (lb_run_advected) through a life in which the members are ordinary handles between the set's
    runs.  A: the subject (an Advected_Scalars, the family's flag on the flow, drawn layouts, forms, variant words, reads, a checkpoint
    through a closed set) equals the twin (S.AdvectedGpu: the three existing calls per set step) in f, rho, u, v and feq of every member --
    in the lazy family, while the flow's fields are those of a run of its own, the flow's rho, u, v, feq equal those of a lazy handle
    given the twin's populations.  B: the twin's flow against O2Sim under the flow contract, every scalar against its float64 model under the scalar
    contract, the model fed the velocity the twin stored step by step (S.hold_advected)."""
    case, ops = S.case_of(kind, family, seed), S.generate(kind, family, seed)
    cuts = S.cut_points(ops, kind, family, seed)
    subject, twin = S.AdvectedGpu(case, tmpdir=tmp_path), S.AdvectedGpu(case, plain=True)
    ref = S.AdvectedRef(case, oracle)
    try:
        for i, op in enumerate(ops):
            if S.is_effective(op):
                subject.effective(op)
                twin.effective(op)
                if op[0] == "run":
                    ref.feed = twin.history
                ref.effective(op)
            else:
                subject.transparent(op)
            if i in cuts:
                what = "%s %s seed %d, behind op %d %r of %r" % (kind, family, seed, i, op, ops[:i + 1])
                want = twin.snapshot()
                assert subject.flow_fields_from == twin.flow_fields_from
                same_bits(subject.snapshot(), want, what, fields=tuple(sorted(want)))
                S.hold_advected("%s %s seed %d op %d, twin / reference" % (kind, family, seed, i), twin, ref)
    finally:
        subject.close()
        twin.close()
