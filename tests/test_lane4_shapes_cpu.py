"""The table of tests/lane4_shapes.py without a GPU: its census per kind and family, the fitness of the inputs tests/test_gpu_lane4_shapes.py
will use -- the float32 model inside the bound the kernel is held to, a misplaced column or row outside it by a factor of ten --, and the
kinds' own shape lists as subsets of the table."""
import os
import re

import numpy as np
import pytest

import lane4_shapes as L4
import test_gpu_lane4_shapes as G
from conftest import ROOT
from scalar_model import CX, CY

KINDS = sorted(L4.KINDS)


def csrc(name):
    return open(os.path.join(ROOT, "2d-lb_amd", "csrc", name)).read()


# ---- the rows of a workgroup, the families: what the table says against the sources --------------------------------------------------
def test_rows_of_a_workgroup_are_the_sources():
    from LB_D2Q9 import _native
    assert int(re.search(r"constexpr int SN_ROWS = (\d+);", csrc("nutrient_launch.h")).group(1)) == _native.SN_ROWS == L4.rows_of("nutrient")
    assert int(re.search(r"constexpr int RY_ROWS = (\d+);", csrc("plan_consts.h")).group(1)) == _native.RY_ROWS == L4.rows_of("rocket")
    few, many = re.search(r"constexpr int step_rows\(\) \{ return NF == 3 \? (\d+) : (\d+); \}", csrc("multifluid.cpp")).groups()
    assert _native.MC_ROWS == {1: int(many), 2: int(many), 3: int(few)} and L4.rows_of("multifluid") == int(many)
    for unit in ("scalar.cpp", "multifield.cpp", "poisson.cpp", "porous.cpp", "expansion.cpp", "advected.cpp"):       # every other kind: 4,
        assert re.search(r"const dim3 block\(64, 4\), grid = step_grid\(", csrc(unit)), unit                           # at the launch of its fused step
    assert re.search(r"block\(64, SN_ROWS\)", csrc("nutrient.cpp")) and re.search(r"constexpr int R = RY_ROWS;", csrc("rocket.cpp"))
    assert len(re.findall(r"block\(64, R \+ 2\)", csrc("rocket.cpp") + csrc("multifluid.cpp"))) == 2                  # the one-launch forms: R rows + halo


KIND_ROWS = [("scalar", "scalar.cpp"), ("noisy", "scalar.cpp"), ("multifield", "multifield.cpp"), ("poisson", "poisson.cpp"),
             ("porous", "porous.cpp"), ("multifluid", "multifluid.cpp"), ("rocket", "rocket.cpp")]


@pytest.mark.parametrize("kind, unit", KIND_ROWS)
def test_families_are_the_kinds_rows(kind, unit):
    """the families lb_create takes for the kind (KIND_ROW's bit set; a noisy scalar lattice is a scalar lattice) are the table's"""
    bits = re.search(r'\(LB_SEM_\w+\)", ((?:1u << LB_BC_\w+(?: \| )?)+),', csrc(unit)).group(1)
    assert {b.lower() for b in re.findall(r"LB_BC_(\w+)", bits)} == set(L4.KINDS[kind]["families"])


@pytest.mark.parametrize("kind, unit", [("nutrient", "nutrient.cpp"), ("expansion", "expansion.cpp"), ("advected", "advected.cpp")])
def test_families_are_what_the_set_calls_take(kind, unit):
    """The sets of scalar lattices are no kind: their run call refuses a member of any other family, and names the families it takes."""
    text = csrc(unit)
    named = set(re.findall(r"LB_BC_(\w+)", " ".join(re.findall(r"\(the famil(?:y|ies) ([^):]*?) only", text))))
    tested = set(re.findall(r"p\.bc_mode != LB_BC_(\w+)", text))
    assert {b.lower() for b in named} == {b.lower() for b in tested} == set(L4.KINDS[kind]["families"]), (named, tested)


def test_classify_by_hand():
    assert L4.classify(2, 2, 4) == dict(c=1, tiles="1", edge_lane="both", rows="below", narrow_y=True)
    assert L4.classify(256, 4, 4) == dict(c=3, tiles="1", edge_lane="last", rows="at", narrow_y=False)
    assert L4.classify(257, 5, 4) == dict(c=0, tiles="2", edge_lane="first", rows="past", narrow_y=False)
    assert L4.classify(260, 11, 4) == dict(c=3, tiles="2", edge_lane="first", rows="ragged", narrow_y=False)
    assert L4.classify(261, 12, 4) == dict(c=0, tiles="2", edge_lane="inner", rows="whole", narrow_y=False)
    assert L4.classify(517, 23, 10) == dict(c=0, tiles="3+", edge_lane="inner", rows="ragged", narrow_y=False)
    assert L4.classify(5, 3, 4)["edge_lane"] == "inner" and L4.classify(1000, 12, 6)["rows"] == "whole"
    assert L4.resolve((8, "2RB+3"), 10) == (8, 23) and L4.resolve((8, "RB-1"), 4) == (8, 3) and L4.resolve((8, "2RB"), 6) == (8, 12)


# ---- 1. the census ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_census(kind):
    """Every kind and family runs every c with one tile, every c with the edge lane first in its tile, the edge lane holding both edges,
    last and inner, three tiles or more, and every class of rows -- but what the kind cannot reach, which is written down with its reason."""
    for family in L4.KINDS[kind]["families"]:
        missing = L4.census(kind, family)
        assert not missing, "%s / %s runs no box of class %s" % (kind, family, missing)
        for form in L4.KINDS[kind]["forms"]:                # ... and every form at every demanded class (the clumpy nutrient set from 3 x 3 on)
            boxes = {(nx, ny) for fam, f, nx, ny in L4.cases(kind) if fam == family and f == form}
            missing = L4.census(kind, family, boxes)
            assert not missing, "%s / %s / %s runs no box of class %s" % (kind, family, form, missing)
        for nx, ny in L4.table(kind, family):
            assert nx <= 1000                               # the widest box is 1000 x 12
    for gone, why in L4.UNREACHABLE.get(kind, {}).items():
        assert why and not any(gone in w for w in L4.demanded(kind))
    if kind in G.MODELLED:                                  # the GPU file reads the same function
        assert [p.values[1:] for p in G.modelled_cases() if p.values[0] == kind] == L4.cases(kind)


# demanded classes the kinds' own lists held before the table, per family (of 17; the nutrient set: of 13)
BEFORE = dict(scalar=[11, 10], noisy=[11, 10], multifield=[11, 11], poisson=[6], porous=[9, 9], multifluid=[10, 10], rocket=[13], nutrient=[8],
              expansion=[5, 5], advected=[9])


def test_census_before():
    """What the kinds' own lists covered (DESIGN.md section 5 records the counts): the holes the table closes are real."""
    before = {kind: {family: L4.census(kind, family, set(L4.table(kind, family, "old"))) for family in L4.KINDS[kind]["families"]} for kind in KINDS}
    assert "c=1 tiles=1" in before["poisson"]["dirichlet"] and "c=2 tiles=1" in before["poisson"]["dirichlet"]
    assert "c=2 edge_lane=first" in before["advected"]["periodic"]
    assert all("c=1 edge_lane=first" in before["multifluid"][f] and "c=2 edge_lane=first" in before["multifluid"][f] for f in before["multifluid"])
    assert {L4.classify(nx, ny, 4)["c"] for nx, ny in L4.table("porous", "zero_gradient", "old") if nx > 4} == {0, 3}
    held = {kind: [len(L4.demanded(kind)) - len(before[kind][f]) for f in L4.KINDS[kind]["families"]] for kind in KINDS}
    assert held == BEFORE, held                             # the figures DESIGN.md section 5 records, per family in the table's order
    for kind in KINDS:
        assert len(L4.demanded(kind)) == (13 if kind == "nutrient" else 17)
        for family, missing in before[kind].items():
            print("%s / %s before: %d of %d demanded classes missing: %s" % (kind, family, len(missing), len(L4.demanded(kind)), ", ".join(missing)))
            assert missing                                  # no kind's own list met the census


def test_the_nutrient_sets_boxes_are_the_spectral_solvers():
    from spectral_model import radix_passes
    for family, form, nx, ny in L4.cases("nutrient"):
        assert set(radix_passes(nx)) | set(radix_passes(ny)) <= {2, 3, 4, 5}
    for lo in (257, 513, 769):                              # ... and why no edge lane of its is the first of a tile
        for nx in range(lo, lo + 4):
            with pytest.raises(AssertionError):
                radix_passes(nx)


# ---- 2. the inputs are fit for the bound --------------------------------------------------------------------------------------------
def model_boxes(kind):
    """(family, a form per model form, nx, ny): every box and model form of the kind's cases, once"""
    K, seen, out = G.MODELLED[kind], set(), []
    for family, form, nx, ny in L4.cases(kind):
        key = (family, K.model_form(form), nx, ny)
        if key not in seen:
            seen.add(key)
            out.append((family, form, nx, ny))
    return out


@pytest.mark.parametrize("kind", sorted(G.MODELLED))
def test_float32_model_sits_inside_the_bound(kind):
    """A condition, not a measurement: from the inputs of the GPU test, after its step counts, the float32 model agrees with the float64
    model within the contract bound the handle will be held to."""
    K = G.MODELLED[kind]
    worst = 0.
    for family, form, nx, ny in model_boxes(kind):
        want, m = G.reference(kind, family, K.model_form(form), nx, ny)
        have, _ = G.reference(kind, family, K.model_form(form), nx, ny, np.float32)
        d = K.inputs(family, form, nx, ny)
        for n in G.STEPS:
            b = K.bounds(d, m, n, want[n])
            for k in K.keys(form):
                r, meas = G.maxratio(have[n][k], want[n][k], b[k])
                worst = max(worst, r)
                assert r <= 1., "%s %s %s %dx%d after %d steps: %s float32 / float64 %.2e > %.1e" % (kind, family, form, nx, ny, n, k, meas, float(np.max(b[k])))
    print("%s: float32 model / float64 model, worst measured / bound %.3f" % (kind, worst))


# ---- 3. the inputs can see a wrong column -------------------------------------------------------------------------------------------
def lattices(m):
    """the objects of a model that stream: itself, or its members (the expansion set)"""
    return getattr(m, "members", [m])


def misplace(m, which, walled):
    """Mutants (a) and (c) of a model, in place.  (a): the east edge column takes its incoming cx = -1 links (f3, f6, f7) from column
    nx - 2 of the lattice before the stream instead of from the wrap or the edge rule; (c): row ny - 1 takes its cy = -1 links (f4, f7, f8)
    from row ny - 2.  In a walled family the corner cells keep the true rule (there the other direction is the edge's as well)."""
    for o in lattices(m):
        before = {}
        move, last_name = o.move, "move_bcs" if hasattr(o, "move_bcs") else "move"

        def moved(o=o, move=move, before=before):
            before["f"] = o.f.copy()
            move()
        o.move = moved
        last = getattr(o, last_name)

        def patched(o=o, last=last, before=before):
            last()
            f, old = o.f, before["f"]
            nx, ny = f.shape[:2]
            if which == "a":
                rows = slice(1, ny - 1) if walled else slice(None)
                for k in (3, 6, 7):
                    f[nx - 1, rows, ..., k] = np.roll(old[nx - 2, ..., k], CY[k], axis=0)[rows]
            else:
                cols = slice(1, nx - 1) if walled else slice(None)
                for k in (4, 7, 8):
                    f[cols, ny - 1, ..., k] = np.roll(old[:, ny - 2, ..., k], CX[k], axis=0)[cols]
        setattr(o, last_name, patched)


class _numpy_with(object):
    """numpy with one function replaced (for a model that calls np.roll in line)"""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getattr__(self, name):
        return getattr(np, name)


def east_density(kind, m, family):
    """Mutant (b): the stencil kinds' density east of cell nx - 1 is the cell itself where it should wrap (periodic), the wrapped cell
    where it should be the cell itself (zero_gradient)."""
    def wrong(shifted, a, cx, cy, same_row):
        if cx == 1:
            shifted = shifted.copy()
            shifted[-1] = same_row(a)[-1 if family == "periodic" else 0]
        return shifted
    if kind == "multifluid":
        shift = m._shift
        m._shift = lambda a, cx, cy: wrong(shift(a, cx, cy), a, cx, cy, lambda a: shift(a, 0, cy))
    elif kind == "rocket":
        at = m._at
        m._at = lambda a, cx, cy: wrong(at(a, cx, cy), a, cx, cy, lambda a: at(a, 0, cy))
    else:
        import nutrient_model
        forces = m.update_forces
        roll = lambda a, shift, axis: wrong(np.roll(a, shift, axis=axis), a, -shift[0], -shift[1], lambda a: np.roll(a, (0, shift[1]), axis=axis))

        def update_forces():
            nutrient_model.np = _numpy_with(roll=roll)
            try:
                forces()
            finally:
                nutrient_model.np = np
        m.update_forces = update_forces


def mutants(kind, family, form, nx, ny):
    """The mutants that apply: in a periodic box two cells wide column nx - 2 IS the wrapped column (two rows high: row ny - 2 the wrapped
    row), so (a) (or (c)) is the true rule there; (b) needs a stencil, and in a zero-gradient box three cells wide the wrapped column and
    the edge column are both copies of the one interior column."""
    out = [which for which, n in (("a", nx), ("c", ny)) if not (family == "periodic" and n == 2)]
    if kind in ("multifluid", "rocket") or (kind == "nutrient" and form[0] == "clumpy"):
        if not (family == "zero_gradient" and nx == 3):
            out.append("b")
    return out


@pytest.mark.parametrize("kind", sorted(G.MODELLED))
def test_a_misplaced_column_or_row_leaves_the_bound(kind):
    """After ONE step from the GPU test's inputs every mutant differs from the true float64 model by ten times the bound of one step or
    more, in some array, at every box: a start too smooth or too symmetric to show a misplaced column fails here, on a host."""
    K = G.MODELLED[kind]
    least = {}
    for family, form, nx, ny in model_boxes(kind):
        d = K.inputs(family, form, nx, ny)
        true = K.model(d, family, form, np.float64)
        with np.errstate(all="ignore"):
            true.run(1)
        want = {k: np.array(v, copy=True) for k, v in K.state(true).items()}
        b = K.bounds(d, true, 1, want)
        for which in mutants(kind, family, form, nx, ny):
            m = K.model(d, family, form, np.float64)
            if which == "b":
                east_density(kind, m, family)
            else:
                misplace(m, which, family in L4.WALLED)
            with np.errstate(all="ignore"):
                m.run(1)
            have = K.state(m)
            r = max(G.maxratio(have[k], want[k], b[k])[0] for k in K.keys(form))
            least[which] = min(least.get(which, np.inf), r)
            assert r >= 10., "%s %s %s %dx%d: mutant (%s) stays within %.2f x the bound of one step" % (kind, family, form, nx, ny, which, r)
    print("%s: the least any mutant leaves the bound by: %s" % (kind, ", ".join("(%s) %.0f x" % kv for kv in sorted(least.items()))))


# ---- 4. the kinds' own lists ---------------------------------------------------------------------------------------------------------
def marked_boxes(test, names):
    """the (nx, ny) a test function is parametrized over under the given argument names"""
    out = []
    for mark in getattr(test, "pytestmark", []):
        if mark.name == "parametrize" and mark.args[0].replace(" ", "") == names:
            out += [tuple(v)[:2] for v in mark.args[1]]
    assert out, (test.__name__, names)
    return out


def own_lists():
    import test_gpu_advected as ad
    import test_gpu_expansion as ex
    import test_gpu_multifield as mf
    import test_gpu_multifluid as mc
    import test_gpu_noise as nf
    import test_gpu_nutrient as sn
    import test_gpu_poisson as ps
    import test_gpu_porous as pm
    import test_gpu_rocket as ry
    import test_gpu_scalar as sc
    return dict(
        scalar=list(sc.TILE_BOXES) + marked_boxes(sc.test_step_kernel_follows_model_on_awkward_boxes, "nx,ny,steps"),
        noisy=list(nf.TILE_BOXES) + marked_boxes(nf.test_noise_fill_follows_the_float64_model, "nx,ny") + [(63, 17), (130, 50)],
        multifield=list(mf.SHAPES),
        poisson=marked_boxes(ps.test_fused_step_equals_phases_bitwise, "shape") + [(261, 9), (21, 13), (37, 23)],
        porous=list(pm.SHAPES) + [(21, 13), (37, 23), (261, 9)],
        multifluid=list(mc.SHAPES),
        rocket=list(ry.shapes()),
        nutrient=list(sn.BOXES) + marked_boxes(sn.test_one_run_equals_single_steps_bitwise, "shape"),
        expansion=marked_boxes(ex.test_runs_repeat_split_and_restore_bitwise, "shape") + marked_boxes(ex.test_fused_step_follows_the_stages, "shape") + [(21, 13)],
        advected=list(ad.SHAPES) + list(ad.MATRIX_SHAPES))


@pytest.mark.parametrize("kind", KINDS)
def test_own_lists_are_subsets_of_the_table(kind):
    mine = own_lists()[kind]
    rb = L4.rows_of(kind)
    table = {L4.resolve(row, rb) for row in (L4.NEW_NUTRIENT if kind == "nutrient" else L4.NEW) + L4.OLD[kind]}
    assert len(mine) >= 4 and set(mine) <= table, sorted(set(mine) - table)
