"""lb_create's refusals, swept: which message wins for every combination of semantics, boundary family, slab, flags, device and grid.

lb_create refuses a handle kind's impossible requests from the kind's row of the table in csrc/host.h (KindOps) -- the accepted
families, the minimum grid, no slabs, no halo interface, no CPU backend -- and where a row's checks stand relative to the others
decides which sentence a caller reads.  create_refusals.json holds, for every combination of the sweep below, the message the
library gave before the rows existed, each distinct message once and the combinations as indices into that list (-1: the
parameters pass validation).  The test holds the library to the code and the message, byte for byte, of every refused combination,
and to not refusing the others as bad arguments (without a GPU they end in LB_ERR_HIP; whatever gets created is destroyed).
"""
import ctypes as ct
import itertools
import json
import os

from conftest import ROOT
from LB_D2Q9 import _native

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "create_refusals.json")
LB_ERR_ARG = -1

SEMANTICS = tuple(range(-1, 13))
BC_MODES = tuple(range(-1, 10))
SLABS = ("whole", "lower half", "offset")
FLAGS = (0, _native.LB_FLAG_HALO, _native.LB_FLAG_PLANAR)
DEVICES = (0, _native.LB_DEVICE_CPU)
GRIDS = ((2, 2), (3, 2), (16, 12))
OMEGA = 0.8


def sweep():
    return itertools.product(SEMANTICS, BC_MODES, SLABS, FLAGS, DEVICES, GRIDS)


def params(semantics, bc_mode, slab, flags, device, grid):
    nx, ny = grid
    y0, local_ny = dict([("whole", (0, ny)), ("lower half", (0, ny // 2)), ("offset", (1, ny - 1))])[slab]
    return _native.LbParams(nx=nx, ny=ny, y0=y0, local_ny=local_ny, bc_mode=bc_mode, device=device, omega=OMEGA, inlet_rho=1., outlet_rho=1.,
                            lid_u=0., rho0=1., flags=flags, semantics=semantics, inlet_u=0., outlet_u=0.)


def create(L, combination):
    """(status code, message) of lb_create on the combination; a handle that got created is destroyed."""
    p, h = params(*combination), ct.c_void_p()
    rc = L.lb_create(ct.byref(p), ct.byref(h))
    if h.value:
        L.lb_destroy(h)
    return rc, L.lb_last_error().decode() if rc else ""


def test_abi_agrees_on_the_status_code():
    with open(os.path.join(ROOT, "include", "lb_hip.h")) as fh:
        assert "LB_ERR_ARG = %d" % LB_ERR_ARG in fh.read()


def test_every_refusal_keeps_its_message(lbhip):
    with open(TABLE) as fh:
        table = json.load(fh)
    combinations = list(sweep())
    assert len(table["index"]) == len(combinations)
    wrong = []
    for combination, i in zip(combinations, table["index"]):
        rc, message = create(lbhip, combination)
        if i < 0:
            if rc == LB_ERR_ARG:
                wrong.append((combination, "passed validation", message))
        elif (rc, message) != (LB_ERR_ARG, table["messages"][i]):
            wrong.append((combination, table["messages"][i], (rc, message)))
    assert not wrong, "%d of %d combinations (semantics, bc_mode, slab, flags, device, grid), the first: %r" % (len(wrong), len(combinations), wrong[:5])
    assert sum(i >= 0 for i in table["index"]) > len(combinations) // 2 and any(i < 0 for i in table["index"])


def record():
    """Writes create_refusals.json.  Run by hand with LB_LIB=<the parent commit's liblbhip.so>, no GPU needed:
        LB_LIB=... python tests/test_create_refusals_cpu.py
    The committed table was recorded at 59adc56 ("Test the launch planner's invariants on a host; march its odd shapes"), the commit
    before lb_create's six per-kind refusal blocks became rows of one table."""
    L = _native.lib()
    messages, index = [], []
    for combination in sweep():
        rc, message = create(L, combination)
        if rc == LB_ERR_ARG and message not in messages:
            messages.append(message)
        index.append(messages.index(message) if rc == LB_ERR_ARG else -1)
    with open(TABLE, "w") as fh:
        json.dump(dict(messages=messages, index=index), fh, separators=(",", ":"), indent=None)
        fh.write("\n")
    return len(messages), sum(i >= 0 for i in index), len(index)


if __name__ == "__main__":
    print("%d distinct messages, %d of %d combinations refused" % record())
