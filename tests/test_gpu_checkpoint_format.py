"""A checkpoint holds the entries it held one commit earlier: every key, its dtype, its shape and its bits.

Round-trip tests cannot see the file format: a key renamed on both sides, a float64 that became a float32, an array that changed its
memory order all survive save -> load.  When the Python package was folded (one row per handle kind in LB_D2Q9/kinds.py, one base
class for the lattice sets) the library stayed the parent's bit for bit, so what a handle writes after three steps must be the
parent's bits too.  checkpoint_format.json holds, for every entry, [dtype string, shape, SHA-256 of the bytes in memory order]:

  every kind and family of tests/sequence_scenarios.py at seed 0 and that module's shapes, the subject built as GpuPlayer builds it,
  after run(3): the file save_checkpoint writes (Simulation, Shan_Chen_Fluids), each member's checkpoint_arrays() for
  Coupled_Scalars (it has no file of its own), entries named 'member<i>.<key>';
  a Surfactant_Colony in both modes at 37 x 23, built as test_gpu_parent_digests.play_rocket builds it, after run(3): its file.

The second test loads each file with from_checkpoint, saves again and compares the second file with the first.  MAY_DIFFER lists what
the docstring of Simulation.from_checkpoint lets differ: rho, u, v of a flow handle that rebuilds them on demand.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import sequence_scenarios as S
from test_gpu_parent_digests import KINDS, ROCKET_MODES, ROCKET_SEED, ROCKET_SHAPE

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "checkpoint_format.json")
SEED, STEPS = 0, 3
# (KINDS: the kinds of tests/sequence_scenarios.py that existed when the table was recorded)
CASES = ["%s-%s" % (k, f) for k in KINDS for f in S.FAMILIES[k]] + ["rocket-%s" % m for m in ROCKET_MODES]
RELOADED = [c for c in CASES if not c.startswith("multifield-")]           # (Coupled_Scalars has no from_checkpoint)


def may_differ(case):
    """Entries of the second file that need not equal the first's: only those three, only on a flow handle that is not eager."""
    kind, family = case.split("-", 1)
    return ("rho", "u", "v") if kind == "flow" and not family.endswith("-eager") else ()


def describe(arrays):
    out = {}
    for name, a in sorted(arrays.items()):
        a = np.asarray(a)
        out[name] = [a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes(order="A")).hexdigest()]
    return out


def subject_of(case):
    kind, family = case.split("-", 1)
    if kind == "rocket":
        from test_gpu_rocket import colony_of, smooth_case
        h = colony_of(smooth_case(ROCKET_SHAPE[0], ROCKET_SHAPE[1], family, ROCKET_SEED))
    else:
        h = S.GpuPlayer(S.case_of(kind, family, SEED)).h
    h.run(STEPS)
    return h


def entries_of(h, path):
    """What h writes (to `path`, where its class has a file format), as {entry: array}."""
    from LB_D2Q9.coupled import Coupled_Scalars
    from LB_D2Q9.simulation import Simulation
    if isinstance(h, Coupled_Scalars):
        return {"member%d.%s" % (i, k): a for i, m in enumerate(h.members) for k, a in m.checkpoint_arrays().items()}
    h.save_checkpoint(path)
    with np.load(Simulation._ckpt_path(path)) as d:
        return {k: d[k] for k in d.files}


def reloaded(case, path):
    from LB_D2Q9.coupled import Shan_Chen_Fluids, Surfactant_Colony
    from LB_D2Q9.simulation import Simulation
    kind, family = case.split("-", 1)
    if kind == "flow":
        return Simulation.from_checkpoint(path, eager_macro=family.endswith("-eager"))
    return dict(multifluid=Shan_Chen_Fluids, rocket=Surfactant_Colony).get(kind, Simulation).from_checkpoint(path)


def first_and_second(case, tmpdir):
    """(the entries of the subject's checkpoint, those of the checkpoint of what from_checkpoint builds from it -- None without one)"""
    path = os.path.join(str(tmpdir), case)
    h = subject_of(case)
    try:
        first = describe(entries_of(h, path))
    finally:
        h.close()
    if case not in RELOADED:
        return first, None
    h = reloaded(case, path)
    try:
        return first, describe(entries_of(h, path + "-again"))
    finally:
        h.close()


def table():
    with open(TABLE) as fh:
        return json.load(fh)


def differing(got, want, skip=()):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    return [(k, got[k][:2], want[k][:2]) for k in sorted(want) if k not in skip and got[k] != want[k]]


@pytest.fixture(scope="module")
def saved(lbhip, tmp_path_factory):
    """case -> first_and_second(case), each made once for both tests"""
    root, made = tmp_path_factory.mktemp("checkpoints"), {}

    def get(case):
        if case not in made:
            made[case] = first_and_second(case, root)
        return made[case]
    return get


@pytest.mark.parametrize("case", CASES)
def test_checkpoint_holds_the_parents_entries(saved, case):
    assert differing(saved(case)[0], table()[case]) == []


@pytest.mark.parametrize("case", RELOADED)
def test_checkpoint_of_a_restored_handle_is_the_same_file(saved, case):
    first, second = saved(case)
    assert differing(second, first, skip=may_differ(case)) == []


def record(tmpdir, path=TABLE):
    """Writes checkpoint_format.json.  Run by hand on an MI355X from a checkout of the parent commit with this file copied into tests/:
        python tests/test_gpu_checkpoint_format.py [where to write the table]
    The committed table was recorded at 39558e5 ("One row per handle kind: fold each physics' host code into its unit"), the commit
    before the package was folded."""
    out = {case: first_and_second(case, tmpdir)[0] for case in CASES}
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
        fh.write("\n")
    return out


if __name__ == "__main__":
    import sys
    import tempfile

    import conftest  # noqa: F401  (puts the package on the path)
    with tempfile.TemporaryDirectory() as tmp:
        print("%d cases recorded" % len(record(tmp, *sys.argv[1:2])))
