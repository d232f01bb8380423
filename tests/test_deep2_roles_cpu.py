"""k_deep2's role table (csrc/deep2_roles.h: deep2_assign_roles) on every input, without a GPU.

The header is plain C++: a small driver is compiled here with the host compiler, the way tests/test_scalar_cpu.py compiles plan.cpp,
and prints the roles of all 4^4 x 2 inputs (four SIMD ids of 0..3, flip 0 / 1) and of a few out-of-range ones.  Two waves of a
workgroup in one body would race on the LDS windows, so what counts first is that EVERY result is a permutation of 0..3."""
import itertools
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

DRIVER = r"""
#include <cstdio>
#include "deep2_roles.h"
static void line(const int *s, int flip)
{
    int role[4] = {-1, -1, -1, -1};
    deep2_assign_roles(s, flip, role);
    std::printf("%d %d %d %d %d %d %d %d %d\n", s[0], s[1], s[2], s[3], flip, role[0], role[1], role[2], role[3]);
}
int main()
{
    for (int n = 0; n < 256; ++n)
        for (int flip = 0; flip < 2; ++flip) {
            const int s[4] = {n & 3, (n >> 2) & 3, (n >> 4) & 3, (n >> 6) & 3};
            line(s, flip);
        }
    // what no SIMD reports: numbers out of range must not index anything
    const int odd[4][4] = {{0, 1, 2, 4}, {-1, 0, 1, 2}, {7, 7, 7, 7}, {0, 1, 2, 1 << 30}};
    for (int k = 0; k < 4; ++k)
        for (int flip = 0; flip < 2; ++flip) line(odd[k], flip);
    return 0;
}
"""

FRONT_DOWN, FRONT_UP, BACK_DOWN, BACK_UP = range(4)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """{(simd tuple, flip): role tuple} of every input the driver ran."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("deep2_roles")
    (tmp / "drv.cpp").write_text(DRIVER)
    exe = str(tmp / "drv")
    subprocess.check_call([cxx, "-std=c++17", "-O0", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "2d-lb_amd", "csrc"), str(tmp / "drv.cpp"), "-o", exe])
    out = {}
    for ln in subprocess.check_output([exe]).decode().splitlines():
        v = [int(x) for x in ln.split()]
        out[(tuple(v[0:4]), v[4])] = tuple(v[5:9])
    return out


def static_rule(flip):
    return tuple((w + 2 * flip) & 3 for w in range(4))


def in_range(key):
    return all(0 <= s < 4 for s in key[0])


def test_every_input_was_run(table):
    assert sum(1 for k in table if in_range(k)) == 4 ** 4 * 2
    assert {k for k in table if in_range(k)} == {(s, f) for s in itertools.product(range(4), repeat=4) for f in (0, 1)}
    assert sum(1 for k in table if not in_range(k)) == 8


def test_every_result_is_a_permutation(table):
    for key, role in table.items():
        assert sorted(role) == [0, 1, 2, 3], (key, role)


def test_on_a_permutation_the_role_follows_the_simd(table):
    perms = list(itertools.permutations(range(4)))
    assert len(perms) == 24
    for simd in perms:
        on = {flip: {simd[w]: table[(simd, flip)][w] for w in range(4)} for flip in (0, 1)}       # SIMD -> role
        # flip 0: SIMDs 0, 1 hold the front pair (down, up), 2, 3 the back pair; flip 1: the other way round
        assert on[0] == {0: FRONT_DOWN, 1: FRONT_UP, 2: BACK_DOWN, 3: BACK_UP}, (simd, on[0])
        assert on[1] == {0: BACK_DOWN, 1: BACK_UP, 2: FRONT_DOWN, 3: FRONT_UP}, (simd, on[1])
        for flip in (0, 1):
            kinds = {sd: r >> 1 for sd, r in on[flip].items()}                                   # 0 front, 1 back
            assert {kinds[0], kinds[1]} == {flip} and {kinds[2], kinds[3]} == {1 - flip}
            # each direction once per kind
            assert sorted(r & 1 for r in on[flip].values() if r >> 1 == 0) == [0, 1]
            assert sorted(r & 1 for r in on[flip].values() if r >> 1 == 1) == [0, 1]
        # two workgroups of opposite flip: a front and a back wave on every SIMD
        for sd in range(4):
            assert (on[0][sd] >> 1) != (on[1][sd] >> 1), (simd, sd)


def test_anything_else_is_the_static_rule(table):
    n = 0
    for (simd, flip), role in table.items():
        if sorted(simd) == [0, 1, 2, 3]:
            continue
        n += 1
        assert role == static_rule(flip), (simd, flip, role)
    assert n == (4 ** 4 - 24) * 2 + 8
