"""Which kernel a forced variant word runs, written once for the GPU tests (the names of the words: LB_D2Q9/variants.py).

The expectations below hold where every kernel the word names applies to the handle (a whole grid of nx >= 512 columns and
>= 128 rows -- tiles: >= 64 x 64 cells --, or slabs high enough for the cycle: include/lb_hip.h, lb_variant_bits); the tests
call them under those conditions.  `max_depth`: the deepest marching kernel the handle's family has (the velocity-inlet
family stops at five steps)."""
import numpy as np

from LB_D2Q9.variants import DEEP2, TILES, depth_of


def steps_per_launch(word, max_depth=7):
    """lb_steps_per_launch under a forced word."""
    return 4 if word & TILES else min(depth_of(word), max_depth)


def kernel_fragment(word, max_depth=7):
    """What lb_hot_kernel's name starts with under a forced word."""
    spl = steps_per_launch(word, max_depth)
    if word & TILES:
        return "k_tile4"
    if spl == 7 and word & DEEP2:
        return "k_deep2<7>"
    if spl >= 6:
        return "k_deep<%d>" % spl
    return "k_step%d" % spl if spl >= 2 else "k_step ("


def assert_forced_kernel(sim, word, max_depth=7):
    assert word >= 0, word                      # (the automatic choice depends on the size: the caller's to state)
    name = sim.hot_kernel()
    assert sim.steps_per_launch() == steps_per_launch(word, max_depth), (word, sim.steps_per_launch(), name)
    assert kernel_fragment(word, max_depth) in name, (word, name)


def same_bits(got, want, what, fields=("f", "rho", "u", "v")):
    for k in fields:
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()), "cells differ")
