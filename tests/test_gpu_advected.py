"""A flow and the scalars it carries (lb_run_advected, LB_D2Q9.coupled.Advected_Scalars) on the GPU.

The yardstick is the sequence the call replaces, on separately created handles: per step ``lb_run(flow, 1)`` on an ``eager_macro=True``
flow, then for every scalar ``set_velocity_from(flow)`` and ``lb_run(scalar, 1)`` under ``set_variant(0)``.  Both forms of the set are
held to it with ``np.array_equal`` -- populations, rho, u, v and feq of the flow and of every scalar -- and so to each other.  The twin of
a shape and a tuple of growth rates is run once, to seven steps with copies at 1, 2, 3 and 7, and shared by every case that needs it.

Shapes: 6 x 5 (the wrap in both directions inside one lane-row), 37 x 23 (nx and ny no multiples of 4: padding lanes), 256 x 4 (exactly
one wave and one block row), 260 x 6 (a second workgroup in x holding four cells, the x-wrap across the tile seam).  Initial state: a
shear layer with a transverse kick (|u| <= 0.05), a striped dye, and a seeded perturbation of every population, so that no symmetry
hides a swapped link.

The growth-rate matrix (MATRIX_GS x both forms x 1 and 2 steps at 37 x 23 and 260 x 6) launches every k_fa_step<NS, REACT, LAST> and takes
the per-member branch inside <2, true> in every order; tests/test_advected_cpu.py derives that census from the lists here.  Form 0
runs under the flow handle's variant word (ROWS_1, ROWS_2, NT_STORES | NT_LOADS, K_DEEP7), which form 1 must ignore.  A lazy flow handle
goes on alone behind a set run from either parity of its lattices, the second time through the captured 16-step graph.

One-line defects tried against this file and the carried set's sequences (tests/test_gpu_sequences.py) in a scratch copy of the library,
value-changing only, none kept, each run once on an MI355X; the cases each turned red, and what the 72 in-process cases of this file
before the matrix (test_external_stream aside) made of the same library:
  fa_step() sends ns == 1 && react to the plain instantiation   ->  test_growth_rate_matrix 4 (G0.05, form 1), the sequences 4; before: none
  the branch in k_fa_step tests m.G[0] for every member         ->  test_growth_rate_matrix 4 (G0_0.05, form 1) and 23 earlier cases; before: 23
                                                                    (G = (0, 0.05) takes the plain cell twice; no sequence: the one life
                                                                    with rates (0, g) in a run of form 1 sets the scalar's f behind it)
  fa_scalar_row<true> is given m.G[1 - i]                       ->  test_growth_rate_matrix 16, test_flow_variant_word 8, the sequences 6, 23
                                                                    earlier cases; before: 23
  LAST skips store_moments of scalar 1                          ->  test_growth_rate_matrix 16, test_flow_variant_word 8, the sequences 6, 23
                                                                    earlier cases; before: 23
  form 0 passes store_rho = false on the last step              ->  test_growth_rate_matrix 24, test_flow_variant_word 8, the lazy-flow tests 4,
                                                                    the sequences 8, 32 earlier cases; before: 34
  set_ran leaves a lazy flow's rho, u, v marked stale           ->  test_lazy_flow_handle 4, test_lazy_flow_graph_replay_behind_an_odd_set_run 4,
                                                                    the sequences 6 (every lazy life); before: test_lazy_flow_handle 4
  flow_step_macro sizes the grid for four rows a block whatever
  the ROWS field says, the block by the field (fewer rows
  written, none outside the lattice)                            ->  test_flow_variant_word 4 (ROWS_1, ROWS_2, form 0), the sequences 4; before: none
  lb_set_macro on a scalar lattice drops u, v while feq is
  stale (a scalar's own run behind set_fields keeps the set's
  velocity)                                                     ->  the sequences 12 of 12; before: none
Three of the eight passed every earlier case.  No defective build faulted or hung.
"""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = ((6, 5), (37, 23), (256, 4), (260, 6))
STEPS = (1, 2, 7)
SNAPS = (1, 2, 3, 7)                        # the steps the twin is copied at
OMEGA_FLOW = 1.3
SCALARS = ((1.6, 0.0), (1.1, 0.05))         # (omega, G) per scalar: different rates, one without growth
KEYS = ("f", "rho", "u", "v", "feq")
# the growth-rate matrix: with react = any G != 0 and LAST = the call's last launch (advected.cpp) these reach every k_fa_step<NS, REACT,
# LAST> and, inside <2, true>, every order of the per-member branch; in form 0 every k_ad_step<PERIODIC, REACT> per member
# (tests/test_advected_cpu.py derives the census from these lists and fails when a case leaves them)
MATRIX_GS = {1: ((0.,), (0.05,)), 2: ((0., 0.), (0.05, 0.), (0., 0.05), (0.05, 0.03))}
MATRIX_SHAPES = ((37, 23), (260, 6))        # padding lanes and a ragged last block row; a second workgroup in x and the x-wrap across the seam
MATRIX_STEPS = (1, 2)                       # LAST alone; one launch that is not the last, then LAST
MATRIX_FORMS = (0, 1)
MATRIX = [(gs, form, n) for ns in sorted(MATRIX_GS) for gs in MATRIX_GS[ns] for form in MATRIX_FORMS for n in MATRIX_STEPS]
WORD_GS, WORD_STEPS = (0.05, 0.), 3         # form 0 under the flow handle's variant word
LB_ERR_ARG, LB_ERR_STATE = -1, -3


def start(nx, ny, ns):
    """(rho, u, v, perturbation) of the flow and (rho, perturbation) per scalar"""
    rng = np.random.default_rng(1000 * nx + ny)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    u = (0.04 * np.tanh((y - 0.5 * ny + 0.5) / max(ny / 8., 1.))).astype(np.float32)
    v = (0.01 * np.sin(2 * np.pi * (x + 0.5) / nx)).astype(np.float32)
    assert float(np.max(np.hypot(u, v))) <= 0.05
    flow = (np.ones((nx, ny), np.float32), u, v, (1 + 0.01 * rng.standard_normal((nx, ny, 9))).astype(np.float32))
    dyes = []
    for i in range(ns):
        stripes = (0.5 + 0.3 * np.sign(np.sin(2 * np.pi * (x + 2 * i) / max(nx / 3., 2.)))).astype(np.float32)
        dyes.append((stripes, (1 + 0.01 * rng.standard_normal((nx, ny, 9))).astype(np.float32)))
    return flow, dyes


def make(nx, ny, ns, eager=True, planar_flow=False, planar_scalars=False, gs=None):
    """gs: the growth rates, one per scalar (None: SCALARS')"""
    from LB_D2Q9.simulation import Simulation
    (rho, u, v, pf), dyes = start(nx, ny, ns)
    flow = Simulation(nx, ny, OMEGA_FLOW, bc="periodic", eager_macro=eager, planar=planar_flow)
    flow.init_equilibrium(rho, u, v, pf)
    scalars = []
    assert gs is None or len(gs) == ns
    rates = SCALARS[:ns] if gs is None else [(om, g) for (om, _), g in zip(SCALARS, gs)]
    for (om, G), (c, pc) in zip(rates, dyes):
        s = Simulation(nx, ny, om, bc="periodic", semantics="diffusion", planar=planar_scalars)
        s.set_reaction(G)
        s.init_equilibrium(c, u, v, pc)
        scalars.append(s)
    return flow, scalars


def make_set(nx, ny, ns, **kw):
    from LB_D2Q9.coupled import Advected_Scalars
    flow, scalars = make(nx, ny, ns, **kw)
    return Advected_Scalars(flow, scalars)


def state(flow, scalars):
    out = {"flow_" + k: a for k, a in flow.get_fields(KEYS).items()}
    for i, s in enumerate(scalars):
        out.update({"s%d_%s" % (i, k): a for k, a in s.get_fields(KEYS).items()})
    return out


def set_state(st):
    return state(st.flow, st.members)


def assert_same(got, want, what):
    assert sorted(got) == sorted(want)
    bad = ["%s: %d of %d" % (k, int((got[k] != want[k]).sum()), got[k].size) for k in sorted(got) if not np.array_equal(got[k], want[k])]
    assert not bad, "%s differs from the twin in %s" % (what, "; ".join(bad))


_TWINS = {}


def twin(lbhip, nx, ny, ns, gs=None):
    """{n: state} for n in SNAPS, of the sequence through the existing calls; computed once per shape and growth rates."""
    gs = tuple(float(g) for _, g in SCALARS[:ns]) if gs is None else tuple(float(g) for g in gs)
    key = (nx, ny, gs)
    if key not in _TWINS:
        from LB_D2Q9._native import check
        flow, scalars = make(nx, ny, ns, eager=True, gs=gs)
        for s in scalars:
            s.set_variant(0)
        snaps = {}
        for n in range(1, max(SNAPS) + 1):
            check(lbhip.lb_run(flow._h, 1))
            for s in scalars:
                s.set_velocity_from(flow)
                check(lbhip.lb_run(s._h, 1))
            if n in SNAPS:
                flow.sync()
                for s in scalars:
                    s.sync()
                snaps[n] = state(flow, scalars)
        flow.close()
        for s in scalars:
            s.close()
        for a in (x for st in snaps.values() for x in st.values()):
            a.setflags(write=False)
        _TWINS[key] = snaps
    return _TWINS[key]


@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("ns", (1, 2))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_bitwise_twin(lbhip, shape, ns, form, n):
    """Both forms against the sequence of existing calls (and so form 0 against form 1), every array, bit for bit."""
    want = twin(lbhip, shape[0], shape[1], ns)[n]
    st = make_set(shape[0], shape[1], ns)
    st.run(n, form=form)
    got = set_state(st)
    st.close()
    assert_same(got, want, "%dx%d, %d scalar(s), form %d, %d step(s)" % (shape + (ns, form, n)))


def _gs_id(gs):
    return "G" + "_".join("%g" % g for g in gs)


@pytest.mark.parametrize("gs,form,n", MATRIX, ids=["%s-form%d-n%d" % (_gs_id(gs), form, n) for gs, form, n in MATRIX])
@pytest.mark.parametrize("shape", MATRIX_SHAPES, ids=lambda s: "%dx%d" % s)
def test_growth_rate_matrix(lbhip, shape, gs, form, n):
    """Every k_fa_step<NS, REACT, LAST> and every order of the per-member branch (form 1), every k_ad_step<PERIODIC, REACT> reading the
    flow's planes (form 0), against the sequence of existing calls with the same growth rates: f, rho, u, v and feq of the flow and of
    every scalar, bit for bit."""
    want = twin(lbhip, shape[0], shape[1], len(gs), gs)[n]
    st = make_set(shape[0], shape[1], len(gs), gs=gs)
    assert [float(m.G) for m in st.members] == [float(np.float32(g)) for g in gs]
    st.run(n, form=form)
    got = set_state(st)
    st.close()
    assert_same(got, want, "%dx%d, G %r, form %d, %d step(s)" % (shape + (gs, form, n)))


def flow_words():
    from LB_D2Q9 import variants as V
    return (("ROWS_1", V.ROWS_1), ("ROWS_2", V.ROWS_2), ("NT_STORES_NT_LOADS", V.NT_STORES | V.NT_LOADS), ("K_DEEP7", V.K_DEEP7))


@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("word", range(4), ids=("ROWS_1", "ROWS_2", "NT_STORES_NT_LOADS", "K_DEEP7"))
@pytest.mark.parametrize("shape", MATRIX_SHAPES, ids=lambda s: "%dx%d" % s)
def test_flow_variant_word(lbhip, shape, word, form):
    """Form 0 takes the flow's block shape and its non-temporal bits from the flow handle's variant word (flow_step_macro), form 1 ignores
    the word: no bit moves against the twin either way."""
    name, bits = flow_words()[word]
    want = twin(lbhip, shape[0], shape[1], 2, WORD_GS)[WORD_STEPS]
    st = make_set(shape[0], shape[1], 2, gs=WORD_GS)
    st.flow.set_variant(bits)
    st.run(WORD_STEPS, form=form)
    got = set_state(st)
    st.close()
    assert_same(got, want, "%dx%d, the flow under %s, form %d" % (shape + (name, form)))


@pytest.mark.parametrize("form", (-1, 0, 1))
def test_default_form_and_split_runs(lbhip, form):
    """run(3) then run(4) equals run(7); form -1 is one of the two and has the same bits; step() is run(1)."""
    want = twin(lbhip, 37, 23, 2)
    st = make_set(37, 23, 2)
    st.run(3, form=form)
    st.run(4, form=form)
    assert_same(set_state(st), want[7], "run(3) + run(4), form %d" % form)
    st.close()
    st = make_set(37, 23, 2)
    st.step()
    assert_same(set_state(st), want[1], "step()")
    name = st.hot_kernel(form)
    assert name.startswith("k_fa_step") or name.startswith("k_step<MACRO> + 2 x k_ad_step"), name
    assert st.hot_kernel(1).startswith("k_fa_step") and "NS = 2" in st.hot_kernel(1) and st.hot_kernel(0).startswith("k_step<MACRO> + 2 x")
    assert "k_fa" not in st.flow.hot_kernel() and "k_ad" not in st.flow.hot_kernel()     # (lb_hot_kernel on the flow: lb_run's)
    st.close()


def lazy_flow_alone(f, nx, ny, n):
    """f, rho, u, v of a fresh flow handle that rebuilds its fields on demand, given the populations f and run n x run(1)"""
    from LB_D2Q9.simulation import Simulation
    flow = Simulation(nx, ny, OMEGA_FLOW, bc="periodic", eager_macro=False)
    flow.set_f(f)
    for _ in range(n):
        flow.run(1)
    out = {"flow_" + k: a for k, a in flow.get_fields(("f", "rho", "u", "v")).items()}
    flow.close()
    return out


def lazy_flow_goes_on(lbhip, shape, form, set_steps, own_steps):
    want = twin(lbhip, shape[0], shape[1], 1)[set_steps]
    st = make_set(shape[0], shape[1], 1, eager=False)
    st.run(set_steps, form=form)
    got = set_state(st)
    assert_same(got, want, "lazy flow, form %d" % form)
    st.flow.run(own_steps)
    got = {"flow_" + k: a for k, a in st.flow.get_fields(("f", "rho", "u", "v")).items()}
    st.close()
    assert_same(got, lazy_flow_alone(want["flow_f"], shape[0], shape[1], own_steps),
                "lazy flow alone for %d steps behind %d set steps, form %d" % (own_steps, set_steps, form))


@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("shape", ((37, 23), (260, 6)), ids=lambda s: "%dx%d" % s)
def test_lazy_flow_handle(lbhip, shape, form):
    """A flow handle that rebuilds rho, u, v on demand: the same populations, and after the call the STORED fields of the eager twin.  Then
    the handle goes on alone as a lazy one: run(2) behind the seven set steps, bit for bit -- f, rho, u, v -- what a fresh lazy handle makes
    of the twin's seven-step populations in two single steps."""
    lazy_flow_goes_on(lbhip, shape, form, 7, 2)


@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("shape", ((37, 23), (260, 6)), ids=lambda s: "%dx%d" % s)
def test_lazy_flow_graph_replay_behind_an_odd_set_run(lbhip, shape, form):
    """One set step leaves every member on the other lattice of its pair; the flow's run(33) behind it -- two replays of the captured
    16-step graph, whose key holds that parity, and a single step -- against 33 x run(1) from the twin's one-step populations."""
    lazy_flow_goes_on(lbhip, shape, form, 1, 33)


@pytest.mark.parametrize("form", (0, 1))
@pytest.mark.parametrize("planar", ((True, False), (False, True), (True, True)), ids=("flow", "scalars", "all"))
@pytest.mark.parametrize("shape", ((37, 23), (260, 6)), ids=lambda s: "%dx%d" % s)
def test_planar_layouts(lbhip, shape, planar, form):
    want = twin(lbhip, shape[0], shape[1], 2)[7]
    st = make_set(shape[0], shape[1], 2, planar_flow=planar[0], planar_scalars=planar[1])
    assert st.flow.layout()["planar"] == planar[0] and st.members[0].layout()["planar"] == planar[1]
    st.run(7, form=form)
    got = set_state(st)
    st.close()
    assert_same(got, want, "planar flow %s, planar scalars %s, form %d" % (planar + (form,)))


@pytest.mark.parametrize("form", (0, 1))
def test_checkpoint_continues_bitwise(lbhip, tmp_path, form):
    """Saved after 3 steps, restored into a fresh set, 4 more: the 7-step run.  The set has no state of its own."""
    from LB_D2Q9.coupled import Advected_Scalars
    want = twin(lbhip, 37, 23, 2)[7]
    st = make_set(37, 23, 2)
    st.run(3, form=form)
    path = str(tmp_path / "advected")
    st.save_checkpoint(path)
    st.close()
    back = Advected_Scalars.from_checkpoint(path)
    assert back.num_populations == 2 and back.flow.eager_macro and [m.G for m in back.members] == [np.float32(g) for _, g in SCALARS]
    back.run(4, form=form)
    got = set_state(back)
    back.close()
    assert_same(got, want, "checkpoint after 3 + 4 steps, form %d" % form)


@pytest.mark.parametrize("form", (0, 1))
def test_mass_is_conserved(lbhip, form):
    """G = 0: the dye's sum of rho after 50 steps on 37 x 23 stays within 50 * 37 * 23 * 2^-24 * max rho of the mass it started with (each
    stored sum rounds once per cell and step: an upper bound, not a fit); the flow's likewise."""
    nx, ny, n = 37, 23, 50
    st = make_set(nx, ny, 1)
    assert st.members[0].G == 0.
    before = {"dye": st.get_fields(("f",))["f"][:, :, 0, :], "flow": st.get_fields(("f_flow",))["f_flow"]}
    st.run(n, form=form)
    g = st.get_fields(("rho", "rho_flow"))
    chk = st.check()
    st.close()
    for name, rho in (("dye", g["rho"][:, :, 0]), ("flow", g["rho_flow"])):
        m0, m1 = float(before[name].astype(np.float64).sum()), float(rho.astype(np.float64).sum())
        bound = n * nx * ny * 2. ** -24 * float(np.max(rho))
        print("form %d, %s: mass %.9f -> %.9f, drift %.3e, bound %.3e" % (form, name, m0, m1, abs(m1 - m0), bound))
        assert abs(m1 - m0) <= bound, (name, m0, m1, bound)
    assert chk["flow"]["n_nonfinite"] == 0 and chk["scalars"][0]["n_nonfinite"] == 0 and chk["flow"]["max_mach"] < 0.1


# ---- refusals: one call each, before anything is enqueued; the handles stay usable -------------------------------------------------
def test_refusals(lbhip):
    from LB_D2Q9.simulation import Simulation
    nx, ny = 37, 23
    flow, (dye, other) = make(nx, ny, 2)
    mask = np.zeros((nx, ny), np.int32)
    mask[5:8, 5:8] = 1
    strangers = dict(
        pipe=Simulation(nx, ny, 1.2, bc="pipe"),
        masked=Simulation(nx, ny, 1.2, bc="periodic", obstacle_mask=mask),
        open=Simulation(nx, ny, 1.2, bc="open", semantics="diffusion"),
        field=Simulation(nx, ny, 1.2, bc="periodic", semantics="multifield"),
        noisy=Simulation(nx, ny, 1.2, bc="periodic", semantics="diffusion"),
        grid=Simulation(nx + 1, ny, 1.2, bc="periodic", semantics="diffusion"),
    )
    strangers["noisy"]._set_noise(0.01, 5)
    h = lambda *sims: (ct.c_void_p * 3)(*[s._h for s in sims])
    cases = (
        ("a PIPE flow", strangers["pipe"], h(dye), 1, 1, -1, LB_ERR_ARG, b"the flow is not periodic"),
        ("a flow with a mask", strangers["masked"], h(dye), 1, 1, -1, LB_ERR_STATE, b"obstacle mask"),
        ("a scalar in the OPEN family", flow, h(strangers["open"]), 1, 1, -1, LB_ERR_ARG, b"scalar 0 is not periodic"),
        ("a multifield handle as scalar", flow, h(strangers["field"]), 1, 1, -1, LB_ERR_ARG, b"scalar 0 is not a scalar lattice"),
        ("set_noise on a scalar", flow, h(dye, strangers["noisy"]), 2, 1, -1, LB_ERR_STATE, b"scalar 1 has the noisy collision on"),
        ("count 0", flow, h(dye), 0, 1, -1, LB_ERR_ARG, b"takes 1..2 scalar lattices"),
        ("count 3", flow, h(dye, other, strangers["noisy"]), 3, 1, -1, LB_ERR_ARG, b"takes 1..2 scalar lattices"),
        ("a different grid", flow, h(strangers["grid"]), 1, 1, -1, LB_ERR_ARG, b"must have the flow's grid (37 x 23)"),
        ("the same scalar twice", flow, h(dye, dye), 2, 1, -1, LB_ERR_ARG, b"appears twice"),
        ("form 2", flow, h(dye), 1, 1, 2, LB_ERR_ARG, b"form must be -1"),
        ("negative n", flow, h(dye), 1, -1, -1, LB_ERR_ARG, b"negative step count"),
        ("the flow passed as a scalar", flow, h(flow), 1, 1, -1, LB_ERR_ARG, b"scalar 0 is not a scalar lattice"),
        ("a null member", flow, h(dye), 2, 1, -1, LB_ERR_ARG, b"null handle in the set"),
    )
    before = state(flow, (dye, other))
    for what, fl, arr, count, n, form, status, text in cases:
        rc = lbhip.lb_run_advected(fl._h, arr, count, n, form)
        assert rc == status and text in lbhip.lb_last_error(), (what, rc, lbhip.lb_last_error())
    assert lbhip.lb_run_advected(flow._h, h(dye), 1, 0, -1) == 0          # n_steps == 0 does nothing
    assert_same(state(flow, (dye, other)), before, "after the refusals")
    assert lbhip.lb_run_advected(flow._h, h(dye, other), 2, 2, -1) == 0
    for s in (flow, dye, other):
        s.sync()
    after = state(flow, (dye, other))
    assert all(np.isfinite(a).all() for a in after.values())
    assert_same(after, twin(lbhip, nx, ny, 2)[2], "two steps after the refusals")
    for s in list(strangers.values()) + [flow, dye, other]:
        s.close()


# ---- the set on an external stream: a child process, torch imported first (tests/stream_scenarios.py has the method) -----------------------
CHILD = r'''
CHILD = "ADVECTED"
import test_gpu_advected as T                   # (the tests directory is on the path: the prelude put it there)
from LB_D2Q9.coupled import Advected_Scalars


def one_form(form):
    """The flow on S behind a delay with a run(2) of its own pending, the second scalar with a run(1) pending on its own stream (the
    join), the set's run(4) without a wait, then the first scalar alone on its own stream (the release) and the flow alone on S."""
    nx, ny = 37, 23

    def chain(st, wait):
        st.flow.run(2, wait=wait)
        st.members[1].run(1, wait=wait)
        st.run(4, wait=wait, form=form)
        st.members[0].run(2, wait=wait)
        st.flow.run(1, wait=wait)

    tw = T.make_set(nx, ny, 2)
    chain(tw, True)
    tw.sync()
    want = T.set_state(tw)
    tw.close()
    S = SIDE[0]
    st = T.make_set(nx, ny, 2)
    st.use_stream(S.cuda_stream)
    torch.cuda.synchronize()
    d = Delay(S)
    chain(st, False)
    d.done()
    torch.cuda.synchronize()
    d.check("lb_run_advected, form %d" % form)
    got = T.set_state(st)
    st.use_stream(None)
    st.close()
    assert_same(got, want, "lb_run_advected on S, form %d" % form)


@scenario
def advected_form_0_on_an_external_stream():
    one_form(0)


@scenario
def advected_form_1_on_an_external_stream():
    one_form(1)
'''


def test_external_stream(lbhip, tmp_path):
    """The set with its flow on an external stream, enqueued behind a bounded delay without a host wait, against the waiting twin, bit
    for bit, both forms; the delay must outlast four times the enqueue."""
    import stream_scenarios as S
    from conftest import ROOT
    script = tmp_path / "child_advected.py"
    script.write_text(S.PRELUDE + CHILD + S.EPILOGUE)
    p = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-lb_amd")],
                       capture_output=True, text=True, timeout=300)
    print("\n".join(l for l in p.stdout.splitlines() if l.startswith(("RATIO", "SCENARIO"))))
    assert p.returncode == 0 and "ADVECTED_OK" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    assert [l for l in p.stdout.splitlines() if l.startswith("SCENARIO")] == [
        "SCENARIO advected_form_0_on_an_external_stream OK", "SCENARIO advected_form_1_on_an_external_stream OK"]
