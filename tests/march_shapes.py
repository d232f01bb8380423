"""Shapes chosen for the geometry of their marching launch: the table tests/test_gpu_march_geometry.py runs on the GPU, and
tests/test_plan_cpu.py holds, on a host, to the classes it claims.

A row is (family, nx, ny, variant word, class).  The class is what `plan_props --classify nx ny bc depth` (tests/plan_props.cpp)
prints for the word's marching launch of the whole grid on 256 CUs -- the rows were generated with it (the heights of the wall
split with its `--onset`) and are data, not computed here:

  seg_rows, last            rows of an interior segment (k_step4 on: of a pair), and of the last one
  edge_seg_rows, edge_last  the same of the two wall-column strips (0: no wall split)
  extra                     the wall strips' items behind strips x segs
  items, wgs                count mod 64 "+0" (fewer than 64: no XCD transposition), "+64" (one transposed block), "+64k" (several) --
                            of the items, and of the workgroups xcd_item sees (k_step2 / k_step3: four items each)
  strips, segs, row_begin   (row_begin: the velocity-inlet family marches rows [d, ny - d))

What is here and why (256 CUs, nx = 964: four strips of 256 cells, five of 248 / 240):
  * the wall split at its onset -- the smallest height at which plan_march sets edge_seg_rows -- and the smallest height at which
    the last interior pair AND the last wall pair hold one row, so that one wave of each marches none: k_step4, k_step5, k_deep<6>,
    k_deep<7>, k_deep2<7> in a pipe and a cavity, k_step4 and k_step5 in the velocity-inlet family.  At these heights the planner's
    two slot counts still round to the same 16 rows (edge_seg_rows == seg_rows, no extra item): the kernels take the wall strips'
    path with the interior's numbers.  Hence also
  * the smallest heights at which the wall segments ARE shorter (extra items), and at which both last pairs of such a split hold
    one row (pipe and velocity inlet: a cavity's plan is the pipe's);
  * tails of 1, 2 and 3 rows for every depth in a periodic box, 964 x 129 ... 131;
  * item counts for the deep kernels: 48 (no transposition), exactly 64, 64 + 21 (the tails' rows), 128 + 7.
"""
from LB_D2Q9.variants import K_DEEP2, K_DEEP6, K_DEEP7, K_STEP2, K_STEP3, K_STEP4, K_STEP5, depth_of

BC_CODES = dict(pipe=0, periodic=1, cavity=2, velocity_inlet=3)         # lb_bc_mode (include/lb_hip.h)

SHAPES = [
    ("pipe", 964, 3856, K_STEP4, "seg_rows=16 last=16 edge_seg_rows=16 edge_last=16 extra=0 items=4+64k wgs=4+64k strips=4 segs=241 row_begin=0"),  # the split's onset
    ("pipe", 964, 3857, K_STEP4, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=8+64k wgs=8+64k strips=4 segs=242 row_begin=0"),  # ... with one-row tails
    ("pipe", 964, 3969, K_STEP4, "seg_rows=17 last=8 edge_seg_rows=16 edge_last=1 extra=30 items=6+64k wgs=6+64k strips=4 segs=234 row_begin=0"),  # shorter wall segments' onset
    ("pipe", 964, 4177, K_STEP4, "seg_rows=18 last=1 edge_seg_rows=16 edge_last=1 extra=58 items=30+64k wgs=30+64k strips=4 segs=233 row_begin=0"),  # ... with one-row tails
    ("cavity", 964, 3856, K_STEP4, "seg_rows=16 last=16 edge_seg_rows=16 edge_last=16 extra=0 items=4+64k wgs=4+64k strips=4 segs=241 row_begin=0"),  # the split's onset
    ("cavity", 964, 3857, K_STEP4, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=8+64k wgs=8+64k strips=4 segs=242 row_begin=0"),  # ... with one-row tails
    ("velocity_inlet", 964, 3864, K_STEP4, "seg_rows=16 last=16 edge_seg_rows=16 edge_last=16 extra=0 items=4+64k wgs=4+64k strips=4 segs=241 row_begin=4"),  # the split's onset
    ("velocity_inlet", 964, 3865, K_STEP4, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=8+64k wgs=8+64k strips=4 segs=242 row_begin=4"),  # ... with one-row tails
    ("velocity_inlet", 964, 3977, K_STEP4, "seg_rows=17 last=8 edge_seg_rows=16 edge_last=1 extra=30 items=6+64k wgs=6+64k strips=4 segs=234 row_begin=4"),  # shorter wall segments' onset
    ("velocity_inlet", 964, 4185, K_STEP4, "seg_rows=18 last=1 edge_seg_rows=16 edge_last=1 extra=58 items=30+64k wgs=30+64k strips=4 segs=233 row_begin=4"),  # ... with one-row tails
    ("pipe", 964, 3091, K_STEP5, "seg_rows=16 last=3 edge_seg_rows=16 edge_last=3 extra=0 items=10+64k wgs=10+64k strips=5 segs=194 row_begin=0"),  # the split's onset
    ("pipe", 964, 3105, K_STEP5, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=15+64k wgs=15+64k strips=5 segs=195 row_begin=0"),  # ... with one-row tails
    ("pipe", 964, 3196, K_STEP5, "seg_rows=17 last=17 edge_seg_rows=16 edge_last=12 extra=24 items=4+64k wgs=4+64k strips=5 segs=188 row_begin=0"),  # shorter wall segments' onset
    ("pipe", 964, 3265, K_STEP5, "seg_rows=17 last=1 edge_seg_rows=16 edge_last=1 extra=24 items=29+64k wgs=29+64k strips=5 segs=193 row_begin=0"),  # ... with one-row tails
    ("cavity", 964, 3091, K_STEP5, "seg_rows=16 last=3 edge_seg_rows=16 edge_last=3 extra=0 items=10+64k wgs=10+64k strips=5 segs=194 row_begin=0"),  # the split's onset
    ("cavity", 964, 3105, K_STEP5, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=15+64k wgs=15+64k strips=5 segs=195 row_begin=0"),  # ... with one-row tails
    ("velocity_inlet", 964, 3101, K_STEP5, "seg_rows=16 last=3 edge_seg_rows=16 edge_last=3 extra=0 items=10+64k wgs=10+64k strips=5 segs=194 row_begin=5"),  # the split's onset
    ("velocity_inlet", 964, 3115, K_STEP5, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=15+64k wgs=15+64k strips=5 segs=195 row_begin=5"),  # ... with one-row tails
    ("velocity_inlet", 964, 3206, K_STEP5, "seg_rows=17 last=17 edge_seg_rows=16 edge_last=12 extra=24 items=4+64k wgs=4+64k strips=5 segs=188 row_begin=5"),  # shorter wall segments' onset
    ("velocity_inlet", 964, 3275, K_STEP5, "seg_rows=17 last=1 edge_seg_rows=16 edge_last=1 extra=24 items=29+64k wgs=29+64k strips=5 segs=193 row_begin=5"),  # ... with one-row tails
    ("pipe", 964, 1546, K_DEEP6, "seg_rows=16 last=10 edge_seg_rows=16 edge_last=10 extra=0 items=37+64k wgs=37+64k strips=5 segs=97 row_begin=0"),  # the split's onset
    ("pipe", 964, 1553, K_DEEP6, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=42+64k wgs=42+64k strips=5 segs=98 row_begin=0"),  # ... with one-row tails
    ("pipe", 964, 1601, K_DEEP6, "seg_rows=17 last=3 edge_seg_rows=16 edge_last=1 extra=12 items=39+64k wgs=39+64k strips=5 segs=95 row_begin=0"),  # shorter wall segments' onset
    ("pipe", 964, 1633, K_DEEP6, "seg_rows=17 last=1 edge_seg_rows=16 edge_last=1 extra=12 items=49+64k wgs=49+64k strips=5 segs=97 row_begin=0"),  # ... with one-row tails
    ("cavity", 964, 1546, K_DEEP6, "seg_rows=16 last=10 edge_seg_rows=16 edge_last=10 extra=0 items=37+64k wgs=37+64k strips=5 segs=97 row_begin=0"),  # the split's onset
    ("cavity", 964, 1553, K_DEEP6, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=42+64k wgs=42+64k strips=5 segs=98 row_begin=0"),  # ... with one-row tails
    ("pipe", 964, 1546, K_DEEP7, "seg_rows=16 last=10 edge_seg_rows=16 edge_last=10 extra=0 items=37+64k wgs=37+64k strips=5 segs=97 row_begin=0"),  # the split's onset
    ("pipe", 964, 1553, K_DEEP7, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=42+64k wgs=42+64k strips=5 segs=98 row_begin=0"),  # ... with one-row tails
    ("pipe", 964, 1601, K_DEEP7, "seg_rows=17 last=3 edge_seg_rows=16 edge_last=1 extra=12 items=39+64k wgs=39+64k strips=5 segs=95 row_begin=0"),  # shorter wall segments' onset
    ("pipe", 964, 1633, K_DEEP7, "seg_rows=17 last=1 edge_seg_rows=16 edge_last=1 extra=12 items=49+64k wgs=49+64k strips=5 segs=97 row_begin=0"),  # ... with one-row tails
    ("cavity", 964, 1546, K_DEEP7, "seg_rows=16 last=10 edge_seg_rows=16 edge_last=10 extra=0 items=37+64k wgs=37+64k strips=5 segs=97 row_begin=0"),  # the split's onset
    ("cavity", 964, 1553, K_DEEP7, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=42+64k wgs=42+64k strips=5 segs=98 row_begin=0"),  # ... with one-row tails
    ("pipe", 964, 1546, K_DEEP2, "seg_rows=16 last=10 edge_seg_rows=16 edge_last=10 extra=0 items=37+64k wgs=37+64k strips=5 segs=97 row_begin=0"),  # the split's onset
    ("pipe", 964, 1553, K_DEEP2, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=42+64k wgs=42+64k strips=5 segs=98 row_begin=0"),  # ... with one-row tails
    ("pipe", 964, 1601, K_DEEP2, "seg_rows=17 last=3 edge_seg_rows=16 edge_last=1 extra=12 items=39+64k wgs=39+64k strips=5 segs=95 row_begin=0"),  # shorter wall segments' onset
    ("pipe", 964, 1633, K_DEEP2, "seg_rows=17 last=1 edge_seg_rows=16 edge_last=1 extra=12 items=49+64k wgs=49+64k strips=5 segs=97 row_begin=0"),  # ... with one-row tails
    ("cavity", 964, 1546, K_DEEP2, "seg_rows=16 last=10 edge_seg_rows=16 edge_last=10 extra=0 items=37+64k wgs=37+64k strips=5 segs=97 row_begin=0"),  # the split's onset
    ("cavity", 964, 1553, K_DEEP2, "seg_rows=16 last=1 edge_seg_rows=16 edge_last=1 extra=0 items=42+64k wgs=42+64k strips=5 segs=98 row_begin=0"),  # ... with one-row tails
    ("periodic", 964, 129, K_STEP2, "seg_rows=4 last=1 edge_seg_rows=0 edge_last=0 extra=0 items=4+64k wgs=33+0 strips=4 segs=33 row_begin=0"),  # a tail of 1
    ("periodic", 964, 130, K_STEP2, "seg_rows=4 last=2 edge_seg_rows=0 edge_last=0 extra=0 items=4+64k wgs=33+0 strips=4 segs=33 row_begin=0"),  # a tail of 2
    ("periodic", 964, 131, K_STEP2, "seg_rows=4 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=4+64k wgs=33+0 strips=4 segs=33 row_begin=0"),  # a tail of 3
    ("periodic", 964, 129, K_STEP3, "seg_rows=4 last=1 edge_seg_rows=0 edge_last=0 extra=0 items=4+64k wgs=33+0 strips=4 segs=33 row_begin=0"),  # a tail of 1
    ("periodic", 964, 130, K_STEP3, "seg_rows=4 last=2 edge_seg_rows=0 edge_last=0 extra=0 items=4+64k wgs=33+0 strips=4 segs=33 row_begin=0"),  # a tail of 2
    ("periodic", 964, 131, K_STEP3, "seg_rows=4 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=4+64k wgs=33+0 strips=4 segs=33 row_begin=0"),  # a tail of 3
    ("periodic", 964, 129, K_STEP4, "seg_rows=8 last=1 edge_seg_rows=0 edge_last=0 extra=0 items=4+64 wgs=4+64 strips=4 segs=17 row_begin=0"),  # a tail of 1
    ("periodic", 964, 130, K_STEP4, "seg_rows=8 last=2 edge_seg_rows=0 edge_last=0 extra=0 items=4+64 wgs=4+64 strips=4 segs=17 row_begin=0"),  # a tail of 2
    ("periodic", 964, 131, K_STEP4, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=4+64 wgs=4+64 strips=4 segs=17 row_begin=0"),  # a tail of 3
    ("periodic", 964, 129, K_STEP5, "seg_rows=8 last=1 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 1
    ("periodic", 964, 130, K_STEP5, "seg_rows=8 last=2 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 2
    ("periodic", 964, 131, K_STEP5, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 3
    ("periodic", 964, 129, K_DEEP6, "seg_rows=8 last=1 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 1
    ("periodic", 964, 130, K_DEEP6, "seg_rows=8 last=2 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 2
    ("periodic", 964, 131, K_DEEP6, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 3
    ("periodic", 964, 129, K_DEEP7, "seg_rows=8 last=1 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 1
    ("periodic", 964, 130, K_DEEP7, "seg_rows=8 last=2 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 2
    ("periodic", 964, 131, K_DEEP7, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 3
    ("periodic", 964, 129, K_DEEP2, "seg_rows=8 last=1 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 1
    ("periodic", 964, 130, K_DEEP2, "seg_rows=8 last=2 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 2
    ("periodic", 964, 131, K_DEEP2, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=21+64 wgs=21+64 strips=5 segs=17 row_begin=0"),  # a tail of 3
    ("periodic", 512, 128, K_DEEP6, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=48+0 wgs=48+0 strips=3 segs=16 row_begin=0"),  # 48 items
    ("periodic", 724, 128, K_DEEP6, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=0+64 wgs=0+64 strips=4 segs=16 row_begin=0"),  # 64 items
    ("periodic", 964, 211, K_DEEP6, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=7+64k wgs=7+64k strips=5 segs=27 row_begin=0"),  # 135 items
    ("periodic", 512, 128, K_DEEP7, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=48+0 wgs=48+0 strips=3 segs=16 row_begin=0"),  # 48 items
    ("periodic", 724, 128, K_DEEP7, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=0+64 wgs=0+64 strips=4 segs=16 row_begin=0"),  # 64 items
    ("periodic", 964, 211, K_DEEP7, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=7+64k wgs=7+64k strips=5 segs=27 row_begin=0"),  # 135 items
    ("periodic", 512, 128, K_DEEP2, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=48+0 wgs=48+0 strips=3 segs=16 row_begin=0"),  # 48 items
    ("periodic", 724, 128, K_DEEP2, "seg_rows=8 last=8 edge_seg_rows=0 edge_last=0 extra=0 items=0+64 wgs=0+64 strips=4 segs=16 row_begin=0"),  # 64 items
    ("periodic", 964, 211, K_DEEP2, "seg_rows=8 last=3 edge_seg_rows=0 edge_last=0 extra=0 items=7+64k wgs=7+64k strips=5 segs=27 row_begin=0"),  # 135 items
]


def class_fields(text):
    """The class line as a dict: numbers where they are numbers."""
    out = {}
    for part in text.split():
        k, v = part.split("=")
        out[k] = int(v) if v.lstrip("-").isdigit() else v
    return out


def classify_args(row):
    """What `plan_props --classify` takes for a row."""
    bc, nx, ny, word, _ = row
    return [str(nx), str(ny), str(BC_CODES[bc]), str(depth_of(word))]


def row_id(row):
    bc, nx, ny, word, _ = row
    return "%s-%dx%d-%d" % (bc, nx, ny, word)
