"""Boxes chosen for the lane-of-four plan (csrc/kernels_lane4.h): the table tests/test_gpu_lane4_shapes.py runs on the GPU for every
handle kind beyond plain flow, and tests/test_lane4_shapes_cpu.py holds, on a host, to the classes it claims (test infrastructure; not a
test module).

On that plan a lane owns four consecutive cells of a row, a wave 256 cells, a workgroup RB rows (the one-launch forms: RB rows plus
halo rows).  What can be wrong there without being wrong everywhere hangs on three numbers, and a row's class names them:

  c          (nx - 1) mod 4: which component of its lane the east edge cell is (clamp_x, lane_nb_load, ad_edge_gather, row_wall,
             gather_merge, k_ps_step's selection of its sums all branch on it)
  tiles      ceil(nx / 256): "1", "2" or "3+"
  edge_lane  where the lane of the east edge sits: "both" (nx <= 4: it holds the west edge as well), "first" ((nx - 1) mod 256 < 4: the
             first lane of its tile -- its west neighbour and its west halo column live in another workgroup), "last" (nx mod 256 == 0),
             "inner"
  rows       ny against RB: "below", "at", "past" (RB + 1), "ragged" (several block rows, ny mod RB != 0), "whole"
  narrow_y   ny <= 3

A row is (nx, ny); ny may be written in the kind's RB -- "RB-1", "RB", "RB+1", "2RB", "2RB+3" -- and is resolved per kind.  The class is
computed, by classify() below, not written down: the host test checks the census of every kind and family against it.

NEW holds the boxes no list had: widths 2 ... 8, 253 ... 260 (every c on both sides of the tile seam, the edge lane last, first and
inner), 512, 513, 517 and 1000; heights 2, 3, RB - 1, RB, RB + 1, 2 RB + 3.  OLD holds, per kind, the boxes its own GPU file already
runs (tests/test_gpu_<kind>.py); the table of a kind is the union.  Width and height 2 belong to the periodic families of the kinds
lb_create lets be that small; the walled families (open, box, dirichlet, zero_gradient) and the kinds with an eight-neighbour stencil
start at 3.  The nutrient set lives on the spectral solver's grid -- nx and ny products of 2, 3 and 5 --, so it has a table of its own
and no box whose edge lane is the first of its tile (none of 257 ... 260, 513 ... 516, 769 ... 772 is such a product).
"""
import re

NEW = [
    (2, 2),             # c=1 both       a periodic box two cells wide and high
    (2, "RB+1"),        # c=1 both       ... with a second block row
    (3, 3),             # c=2 both       the smallest walled box: one interior cell
    (4, "RB"),          # c=3 both       exactly one lane
    (5, "RB+1"),        # c=0 inner      the east edge alone in the second lane
    (6, 2),             # c=1 inner      two rows: each the other's north and south neighbour
    (6, "2RB"),         # c=1 inner      whole block rows
    (7, "RB-1"),        # c=2 inner
    (8, "2RB+3"),       # c=3 inner      ragged
    (253, "RB-1"),      # c=0 tiles=1 inner
    (254, 3),           # c=1 tiles=1 inner, narrow in y
    (255, "RB"),        # c=2 tiles=1 inner
    (256, "RB"),        # c=3 tiles=1 last
    (257, "RB+1"),      # c=0 tiles=2 first: the second tile holds one cell
    (258, "2RB+3"),     # c=1 tiles=2 first
    (259, "RB-1"),      # c=2 tiles=2 first
    (260, "RB+1"),      # c=3 tiles=2 first: the second tile holds exactly one lane
    (512, "RB"),        # c=3 tiles=2 last
    (513, "RB+1"),      # c=0 tiles=3+ first
    (517, "2RB+3"),     # c=0 tiles=3+ inner: a workgroup with neighbours on both sides
    (1000, 12),         # c=3 tiles=3+ inner: four tiles, the last one ragged in x
]

# the spectral solver's grids only (radices 2, 3, 5 on both axes); SN_ROWS = 4
NEW_NUTRIENT = [
    (2, 2), (3, 3), (4, 4), (5, 5), (6, 2), (6, 8), (8, 10),
    (225, 3),           # c=0 tiles=1
    (250, 5),           # c=1 tiles=1
    (243, 4),           # c=2 tiles=1
    (256, 4),           # c=3 tiles=1 last
    (270, 9),           # c=1 tiles=2 inner, ragged
    (512, 4),           # c=3 tiles=2 last
    (1000, 12),         # c=3 tiles=3+
]

# The boxes of NEW / NEW_NUTRIENT that run every form of a kind: between them they hold every class the census demands.  At the other
# boxes the forms take turns (cases()).
EVERY_FORM = [(2, 2), (3, 3), (4, "RB"), (6, "2RB"), (253, "RB-1"), (254, 3), (255, "RB"), (256, "RB"), (257, "RB+1"), (258, "2RB+3"),
              (259, "RB-1"), (260, "RB+1"), (513, "RB+1")]
EVERY_FORM_NUTRIENT = [(3, 3), (4, 4), (5, 5), (6, 8), (225, 3), (250, 5), (243, 4), (256, 4), (270, 9), (1000, 12)]

# per kind, what its own GPU file runs today (the host test holds these to the files' lists)
OLD = dict(
    scalar=[(64, 48), (128, 50), (96, 33), (160, 17), (37, 23), (130, 50), (63, 17), (255, 33), (258, 70), (20, 10), (9, 5), (5, 3), (4, 2), (64, 16)],
    noisy=[(64, 48), (128, 50), (96, 33), (160, 17), (37, 23), (130, 50), (63, 17), (255, 33), (258, 70), (20, 10), (9, 5), (5, 3), (4, 2), (130, 9)],
    multifield=[(37, 23), (63, 17), (64, 16), (255, 33), (258, 9), (5, 4), (3, 3), (1000, 12)],
    poisson=[(5, 4), (37, 23), (261, 9), (256, 4), (21, 13)],
    porous=[(5, 4), (3, 3), (37, 23), (261, 9), (256, 4), (21, 13)],
    multifluid=[(3, 3), (5, 4), (37, 23), (261, 9), (256, 4), (517, 5), (6, 9), (6, 13)],
    rocket=[(3, 3), (5, 4), (37, 23), (63, 17), (64, 16), (255, 33), (256, "RB"), (257, "RB+1"), (258, 9), (1000, 12)],
    nutrient=[(270, 12), (1000, 12), (12, 1000), (5, 4), (30, 18)],
    expansion=[(5, 4), (37, 23), (261, 9), (8, 4), (21, 13)],
    advected=[(6, 5), (37, 23), (256, 4), (260, 6)],
)

# kind -> (boundary families the kind dispatches, its forms, where its RB comes from, the kinds's smallest periodic box).  The forms
# are those whose column, seam or row code differs; RB: "4" (the two-launch plan), or the name of the constant LB_D2Q9._native exports.
KINDS = dict(
    scalar=dict(families=("periodic", "open"), forms=("K_STEP", "TILES"), rb=4, smallest=2),
    noisy=dict(families=("periodic", "open"), forms=("plane", "cell"), rb=4, smallest=2),
    multifield=dict(families=("periodic", "box"), forms=(1, 2), rb=4, smallest=2),
    poisson=dict(families=("dirichlet",), forms=("run", "solve"), rb=4, smallest=3),
    porous=dict(families=("periodic", "zero_gradient"), forms=("plain", "field"), rb=4, smallest=2),
    multifluid=dict(families=("periodic", "zero_gradient"), forms=(0, 1), rb="MC_ROWS", smallest=3),
    rocket=dict(families=("periodic",), forms=((0, "flow"), (0, "forces"), (1, "flow"), (1, "forces")), rb="RY_ROWS", smallest=3),
    nutrient=dict(families=("periodic",), forms=(("plain", 0), ("plain", 1), ("clumpy", 0), ("clumpy", 1)), rb="SN_ROWS", smallest=2),
    expansion=dict(families=("periodic", "open"), forms=(1, 2), rb=4, smallest=2),
    advected=dict(families=("periodic",), forms=((0, 1), (0, 2), (1, 1), (1, 2)), rb=4, smallest=2),
)
WALLED = ("open", "box", "dirichlet", "zero_gradient")
# the classes a kind cannot reach, with the reason (the census leaves out exactly these)
UNREACHABLE = dict(nutrient={"edge_lane=first": "no product of 2, 3 and 5 lies in 257 ... 260, 513 ... 516 or 769 ... 772"})


def rows_of(kind):
    """RB of a kind: rows a workgroup owns (two fluids for the multifluid set: the forms here run two)."""
    rb = KINDS[kind]["rb"]
    if isinstance(rb, int):
        return rb
    from LB_D2Q9 import _native
    value = getattr(_native, rb)
    return value[2] if isinstance(value, dict) else value


def resolve(row, rb):
    """(nx, ny) with ny a number"""
    nx, ny = row
    if isinstance(ny, str):
        m = re.fullmatch(r"(\d*)RB([+-]\d+)?", ny)
        ny = int(m.group(1) or 1) * rb + int(m.group(2) or 0)
    return int(nx), int(ny)


def classify(nx, ny, rb):
    """The class of a box, from nx, ny and the rows of a workgroup."""
    c = (nx - 1) % 4
    n_tiles = -(-nx // 256)
    tiles = "3+" if n_tiles >= 3 else str(n_tiles)
    if nx <= 4:
        edge_lane = "both"
    elif (nx - 1) % 256 < 4:
        edge_lane = "first"
    elif nx % 256 == 0:
        edge_lane = "last"
    else:
        edge_lane = "inner"
    if ny < rb:
        rows = "below"
    elif ny == rb:
        rows = "at"
    elif ny == rb + 1:
        rows = "past"
    elif ny % rb != 0:
        rows = "ragged"
    else:
        rows = "whole"
    return dict(c=c, tiles=tiles, edge_lane=edge_lane, rows=rows, narrow_y=ny <= 3)


def fits(kind, family, nx, ny):
    """lb_create takes the box for this kind and family and every rule of the family is unambiguous in it.  (The clumpy form of the
    nutrient set has a stencil: its forms are filtered in cases().)"""
    least = 3 if family in WALLED else KINDS[kind]["smallest"]
    return nx >= least and ny >= least


def table(kind, family, which="all"):
    """The boxes of a kind and family, resolved, in the table's order without repeats; which: 'new', 'old' or 'all'."""
    rb = rows_of(kind)
    new = NEW_NUTRIENT if kind == "nutrient" else NEW
    rows = dict(new=new, old=OLD[kind], all=list(new) + list(OLD[kind]))[which]
    out = []
    for row in rows:
        box = resolve(row, rb)
        if fits(kind, family, *box) and box not in out:
            out.append(box)
    return out


def cases(kind):
    """[(family, form, nx, ny)]: what the GPU file runs for a kind, and what the host test takes its census and its inputs from.
    Every form at the boxes of EVERY_FORM, which hold every demanded class; at the other new boxes, and at a kind's old boxes, which its
    own file already runs in every form, the forms take turns."""
    out = []
    forms = KINDS[kind]["forms"]
    rb = rows_of(kind)
    every = {resolve(row, rb) for row in (EVERY_FORM_NUTRIENT if kind == "nutrient" else EVERY_FORM)}
    for family in KINDS[kind]["families"]:
        new = table(kind, family, "new")
        turn = 0
        for nx, ny in new + [b for b in table(kind, family, "old") if b not in new]:
            mine = forms
            if (nx, ny) not in every:
                mine, turn = (forms[turn % len(forms)],), turn + 1
            for form in mine:
                if kind == "nutrient" and form[0] == "clumpy" and (nx < 3 or ny < 3):
                    continue                    # (the clumpy variant needs eight neighbours: lb_run_nutrient refuses below 3 x 3)
                out.append((family, form, nx, ny))
    return out


def demanded(kind):
    """The classes the census asks of every (kind, family): 'part=value' strings, and combinations 'c=2 tiles=1'."""
    want = ["c=%d tiles=1" % c for c in range(4)] + ["c=%d edge_lane=first" % c for c in range(4)]
    want += ["edge_lane=%s" % e for e in ("both", "last", "inner")] + ["tiles=3+"]
    want += ["rows=%s" % r for r in ("below", "at", "past", "ragged", "whole")]
    gone = UNREACHABLE.get(kind, {})
    return [w for w in want if not any(g in w for g in gone)]


def census(kind, family, boxes=None):
    """The demanded classes the boxes (default: those of cases(kind) in this family) do NOT cover."""
    rb = rows_of(kind)
    if boxes is None:
        boxes = {(nx, ny) for fam, _, nx, ny in cases(kind) if fam == family}
    classes = [classify(nx, ny, rb) for nx, ny in boxes]
    covers = lambda cl, w: all(str(cl[part.split("=")[0]]) == part.split("=")[1] for part in w.split())
    return [w for w in demanded(kind) if not any(covers(cl, w) for cl in classes)]


def case_id(case):
    family, form, nx, ny = case
    tag = "-".join(str(x) for x in form) if isinstance(form, tuple) else str(form)
    return "%s-%s-%dx%d" % (family, tag, nx, ny)
