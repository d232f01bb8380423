"""The host side hands the kernels the arguments it handed them one commit earlier: SHA-256 digests of every array, bit for bit.

The kernels are deterministic and were not touched when each handle kind's host code moved into the kind's own translation unit
(csrc/host.h, KindOps), so a library whose host code fills one kernel argument differently -- a stride, a derived float32 scalar, which
lattice of the pair is current, a store flag on the wrong launch -- leaves other bits behind.  gpu_parent_digests.json holds what the
commit before that move left behind:

  every committed sequence of tests/sequence_scenarios.py (every kind, family and seed, at its shapes), played as the subject of
  tests/test_gpu_sequences.py plays it (effective and transparent ops): the digests of snapshot() behind the last op -- f, rho, u, v,
  feq and the kind's own planes and state words;
  a surfactant-propelled colony, which that module does not cover, at 37 x 23 in both modes: three fused steps under variant 0, three
  under variant 1, then one step by the stage calls, the digests of every array behind each of the three.

record() wrote the table; the tests replay each case and compare.  A mismatch names the arrays that differ.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import sequence_scenarios as S

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_parent_digests.json")
KINDS = ("flow", "scalar", "multifield", "poisson", "porous", "multifluid")      # (the kinds that module had when the table was recorded:
SEQUENCES = [(k, f, s) for k in KINDS for f in S.FAMILIES[k] for s in S.SEEDS]  #  the later ones have no parent in this sense)
ROCKET_SHAPE, ROCKET_MODES, ROCKET_SEED = (37, 23), ("flow", "forces"), 11


def digests(arrays):
    return {name: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest() for name, a in sorted(arrays.items())}


def play_sequence(kind, family, seed, tmpdir):
    subject = S.GpuPlayer(S.case_of(kind, family, seed), tmpdir=tmpdir)
    try:
        S.play(subject, S.generate(kind, family, seed), transparent=True)
        return digests(subject.snapshot())
    finally:
        subject.close()


def play_rocket(mode):
    from test_gpu_rocket import all_keys, colony_of, got_of, smooth_case
    colony = colony_of(smooth_case(ROCKET_SHAPE[0], ROCKET_SHAPE[1], mode, ROCKET_SEED))
    try:
        out = {}
        for stage in ("variant0", "variant1", "stages"):
            if stage == "stages":
                colony.step_phases()
            else:
                colony.set_variant(int(stage[-1]))
                colony.run(3)
            out.update({"%s.%s" % (stage, k): d for k, d in digests(got_of(colony, all_keys(mode) + ("feq",))).items()})
        return out
    finally:
        colony.close()


def table():
    with open(TABLE) as fh:
        return json.load(fh)


def differing(got, want):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    return [k for k in sorted(want) if got[k] != want[k]]


@pytest.mark.parametrize("kind,family,seed", SEQUENCES, ids=["%s-%s-%d" % c for c in SEQUENCES])
def test_sequence_leaves_the_parents_bits(lbhip, tmp_path, kind, family, seed):
    assert differing(play_sequence(kind, family, seed, tmp_path), table()["%s-%s-%d" % (kind, family, seed)]) == []


@pytest.mark.parametrize("mode", ROCKET_MODES)
def test_colony_leaves_the_parents_bits(lbhip, mode):
    assert differing(play_rocket(mode), table()["rocket-%s" % mode]) == []


def record(tmpdir):
    """Writes gpu_parent_digests.json.  Run by hand on an MI355X with LB_LIB=<the parent commit's liblbhip.so>:
        LB_LIB=... python tests/test_gpu_parent_digests.py
    The committed table was recorded at 59adc56 ("Test the launch planner's invariants on a host; march its odd shapes"), the commit
    before each kind's host code moved into its unit."""
    out = {}
    for kind, family, seed in SEQUENCES:
        out["%s-%s-%d" % (kind, family, seed)] = play_sequence(kind, family, seed, tmpdir)
    for mode in ROCKET_MODES:
        out["rocket-%s" % mode] = play_rocket(mode)
    with open(TABLE, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    return out


if __name__ == "__main__":
    import tempfile

    import conftest  # noqa: F401  (puts the package on the path)
    with tempfile.TemporaryDirectory() as tmp:
        print("%d cases recorded" % len(record(tmp)))
