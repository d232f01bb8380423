"""Names for the kernel variant word of ``Simulation.set_variant`` (``lb_set_variant``): the ``LB_VAR_*`` enumerators of
include/lb_hip.h without their prefix, as plain ints (tests/test_host_logic.py holds the two lists to each other).  What each bit
means, where it applies and what the automatic choice takes is told beside the enumerators in the header.  Results never
depend on the word (bitwise); it decides which fused kernel computes them."""

AUTO = -1                       # the library's own choice (the default)

NT_STORES = 1 << 0
NT_LOADS = 1 << 1
ROWS = 3 << 2                   # a field: 0, ROWS_1 or ROWS_2 (scalar lattices with TILES: shape << 2, shape 1 ... 3)
ROWS_1 = 1 << 2
ROWS_2 = 2 << 2
XCD_ORDER = 1 << 4
STEP2 = 1 << 5
STEP3 = 1 << 6
NO_CYCLE = 1 << 7
STEP4 = 1 << 8
TILES = 1 << 9
STEP4_NO_AHEAD = 1 << 10
NO_PRIO_TURNS = 1 << 11
STEP5 = 1 << 12
TILE_LAUNCH_ORDER = 1 << 13
STEP6 = 1 << 14
STEP7 = 1 << 15
DEEP2 = 1 << 16

_STEPS = (STEP2, STEP3, STEP4, STEP5, STEP6, STEP7)


def marching(depth, deep2=False, nt_stores=True):
    """The word that lets the marching kernels fuse up to `depth` (2 ... 7) time steps per launch.  The planner takes a depth only
    with every shallower one (cycle_depth, whole_grid_depths in plan.cpp), so STEP2 ... STEP<depth> are all set; deep2: the
    seven steps by k_deep2<7> instead of k_deep<7>."""
    if not 2 <= depth <= 7 or (deep2 and depth != 7):
        raise ValueError("marching(%r, deep2=%r)" % (depth, deep2))
    word = NT_STORES if nt_stores else 0
    for bit in _STEPS[:depth - 1]:
        word |= bit
    return word | (DEEP2 if deep2 else 0)


def depth_of(word):
    """Steps per launch the marching bits of a word allow: k with STEP2 ... STEPk all set (1: none)."""
    depth = 1
    for bit in _STEPS:
        if not word & bit:
            break
        depth += 1
    return depth


# the kernels the tests and tools select by name
K_STEP = 0
K_STEP2 = marching(2)           # 33
K_STEP3 = marching(3)           # 97
K_STEP4 = marching(4)           # 353
K_STEP5 = marching(5)           # 4449
K_DEEP6 = marching(6)           # 20833: k_deep<6>
K_DEEP7 = marching(7)           # 53601: k_deep<7>
K_DEEP2 = marching(7, deep2=True)   # 119137: k_deep2<7>
K_TILE4 = TILES                 # 512

_FLAGS = (("NT_STORES", NT_STORES), ("NT_LOADS", NT_LOADS), ("XCD_ORDER", XCD_ORDER), ("NO_CYCLE", NO_CYCLE), ("TILES", TILES),
          ("STEP4_NO_AHEAD", STEP4_NO_AHEAD), ("NO_PRIO_TURNS", NO_PRIO_TURNS), ("TILE_LAUNCH_ORDER", TILE_LAUNCH_ORDER),
          ("DEEP2", DEEP2))


def describe(word):
    """A word in names, for a log line: describe(119137) == 'STEP2..7 | NT_STORES | DEEP2'."""
    word = int(word)
    if word < 0:
        return "AUTO"
    parts = []
    depth = depth_of(word)
    if depth > 1:
        parts.append("STEP2" if depth == 2 else "STEP2..%d" % depth)
    parts += ["STEP%d" % k for k, bit in enumerate(_STEPS[depth - 1:], depth + 1) if word & bit]      # (bits above a gap)
    if word & ROWS:
        parts.append("ROWS_%d" % ((word & ROWS) >> 2))
    parts += [name for name, bit in _FLAGS if word & bit]
    if word >> 17:
        parts.append("0x%x" % (word >> 17 << 17))
    return " | ".join(parts) or "K_STEP"
