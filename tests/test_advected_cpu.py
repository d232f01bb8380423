"""A flow and the scalars it carries, without a GPU: the two ABI symbols, the refusals that need no device, the unit in the build, the
Python class's surface and the mismatches it refuses before the library is called."""
import ctypes as ct
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT


def header():
    return open(os.path.join(ROOT, "include", "lb_hip.h")).read()


def test_entry_points_exported_bound_and_declared(lbhip):
    from LB_D2Q9 import _native
    text = header()
    for name in ("lb_run_advected", "lb_advected_kernel"):
        fn = getattr(lbhip, name)
        assert name in _native.EXPORTS and name in _native.SIGNATURES and fn.argtypes is not None, name
    assert re.search(r"\bint lb_run_advected\(lb_sim \*flow, lb_sim \*\*scalars, int count, int n_steps, int form\);", text)
    assert re.search(r"\bint lb_advected_kernel\(int count, int form, int64_t cells, char \*buf, int buflen\);", text)
    assert len(_native.SIGNATURES["lb_run_advected"][0]) == 5 and len(_native.SIGNATURES["lb_advected_kernel"][0]) == 5
    assert int(re.search(r"#define LB_ABI_VERSION (\d+)", text).group(1)) == 11 == _native.ABI_VERSION == lbhip.lb_abi_version()


def test_null_arguments_are_refused(lbhip):
    assert lbhip.lb_run_advected(None, None, 0, 0, 0) == -1 and b"null" in lbhip.lb_last_error()
    assert lbhip.lb_advected_kernel(1, -1, 0, None, 0) == -1 and b"null" in lbhip.lb_last_error()


def test_refusals_that_need_no_device(lbhip):
    """LB_ERR_ARG (-1) with the reason before any device is touched: a null array, a handle of the CPU backend as the flow."""
    from LB_D2Q9 import _native
    from LB_D2Q9.simulation import Simulation
    host = Simulation(8, 6, 1.0, semantics="cython", device=_native.LB_DEVICE_CPU)
    try:
        one = (ct.c_void_p * 2)(host._h, None)
        assert lbhip.lb_run_advected(host._h, None, 1, 1, -1) == -1 and b"null handle array" in lbhip.lb_last_error()
        for count in (-1, 0, 3):
            assert lbhip.lb_run_advected(host._h, one, count, 1, -1) == -1 and b"takes 1..2 scalar lattices" in lbhip.lb_last_error(), count
        assert lbhip.lb_run_advected(host._h, one, 1, 1, -1) == -1 and b"the flow is not a GPU flow handle" in lbhip.lb_last_error()
    finally:
        host.close()


def test_kernel_names(lbhip):
    buf = ct.create_string_buffer(512)
    for count in (1, 2):
        assert lbhip.lb_advected_kernel(count, 1, 1 << 20, buf, len(buf)) == 0
        assert buf.value.startswith(b"k_fa_step") and b"NS = %d" % count in buf.value
        assert lbhip.lb_advected_kernel(count, 0, 1 << 20, buf, len(buf)) == 0
        assert buf.value.startswith(b"k_step<MACRO> + %d x k_ad_step" % count)
        for cells in (256 * 256, 2048 * 2048, 8192 * 8192):        # the planner's choice is one of the two
            assert lbhip.lb_advected_kernel(count, -1, cells, buf, len(buf)) == 0 and buf.value.startswith((b"k_fa_step", b"k_step<MACRO> + "))
    assert lbhip.lb_advected_kernel(3, 1, 100, buf, len(buf)) == -1 and b"takes 1..2" in lbhip.lb_last_error()
    assert lbhip.lb_advected_kernel(1, 2, 100, buf, len(buf)) == -1 and b"form must be -1" in lbhip.lb_last_error()


def test_the_growth_rate_matrix_reaches_every_instantiation():
    """What lb_run_advected launches for every case of tests/test_gpu_advected.py's growth-rate matrix, by the rule of advected.cpp --
    react = some scalar has G != 0, LAST = the call's last launch, inside <NS, true> member i takes the growth cell where G[i] != 0; form 0:
    one k_ad_step<PERIODIC, REACT = G[i] != 0, RHO = the last step> per scalar --: all eight k_fa_step<NS, REACT, LAST>, all four orders of
    the per-member branch with two scalars, and in form 0 either cell for the scalar in either place.  A case taken out of the matrix's
    lists fails here."""
    import test_gpu_advected as T
    source = open(os.path.join(ROOT, "2d-lb_amd", "csrc", "advected.cpp")).read()
    assert "react = react || scalars[i]->ad_G != 0.f;" in source and "fa_step(count, react, it == n_steps - 1, flow->stream, m);" in source
    assert "scalar_step_carried(scalars[i], flow, it == n_steps - 1)" in source
    triples, orders, carried = set(), set(), set()
    for gs, form, n in T.MATRIX:
        ns, react = len(gs), any(np.float32(g) != 0 for g in gs)
        for it in range(n):
            last = it == n - 1
            if form == 1:
                triples.add((ns, react, last))
                if ns == 2:
                    orders.add(tuple("react" if react and np.float32(g) != 0 else "plain" for g in gs))
            else:
                carried |= {(ns, i, np.float32(g) != 0, last) for i, g in enumerate(gs)}
    assert triples == {(ns, react, last) for ns in (1, 2) for react in (False, True) for last in (False, True)}, triples
    assert orders == {("plain", "plain"), ("react", "plain"), ("plain", "react"), ("react", "react")}, orders
    assert carried == {(ns, i, react, last) for ns in (1, 2) for i in range(ns) for react in (False, True) for last in (False, True)}, carried
    assert set(T.MATRIX_SHAPES) == {(37, 23), (260, 6)} and set(T.MATRIX_FORMS) == {0, 1}
    assert len(T.MATRIX) == len(set(T.MATRIX)) == 24
    # the variant-word cases: two scalars, the FIRST with the growth cell while it reads the flow handle's planes
    assert len(T.WORD_GS) == 2 and T.WORD_GS[0] != 0. and T.WORD_GS[1] == 0. and T.WORD_STEPS in T.SNAPS and T.WORD_STEPS % 2 == 1
    assert set(T.MATRIX_STEPS) | set(T.STEPS) <= set(T.SNAPS)


def test_build_lists_the_unit():
    build = open(os.path.join(ROOT, "2d-lb_amd", "build.py")).read()
    assert '"advected.cpp"' in build
    for name in ("advected.cpp", "advected_launch.h", "kernels_advected.h"):
        assert os.path.exists(os.path.join(ROOT, "2d-lb_amd", "csrc", name)), name


def test_class_surface():
    from LB_D2Q9 import coupled
    cls = coupled.Advected_Scalars
    assert issubclass(cls, coupled._Lattice_Set) and issubclass(cls, coupled._Shared_Velocity)
    for name in ("run", "step", "sync", "hot_kernel", "get_fields", "check", "save_checkpoint", "from_checkpoint", "use_stream", "close"):
        assert callable(getattr(cls, name)), name
    import inspect
    assert list(inspect.signature(cls.__init__).parameters) == ["self", "flow", "scalars"]
    run = inspect.signature(cls.run).parameters
    assert list(run) == ["self", "num_iterations", "wait", "form"] and run["wait"].default is True and run["form"].default == -1
    assert inspect.signature(cls.hot_kernel).parameters["form"].default == -1
    assert inspect.signature(cls.from_checkpoint).parameters["device"].default == 0


def _stub(semantics, bc, nx=16, ny=12, device=0):
    from LB_D2Q9 import _native
    return types.SimpleNamespace(semantics=semantics, bc_mode=_native.BC_NAMES[bc], nx=nx, ny=ny, local_ny=ny, device=device, _h=None)


@pytest.mark.parametrize("flow, scalars, text", (
    (("opencl", "periodic"), [("diffusion", "periodic", 17, 12)], "grid"),
    (("opencl", "periodic"), [("diffusion", "periodic"), ("diffusion", "periodic", 16, 13)], "grid"),
    (("opencl", "pipe"), [("diffusion", "periodic")], "the flow must have bc='periodic'"),
    (("opencl", "periodic"), [("diffusion", "open")], "scalar 0 must have bc='periodic'"),
    (("d2q9i", "periodic"), [("diffusion", "periodic")], "the flow must have semantics='opencl'"),
    (("opencl", "periodic"), [("multifield", "periodic")], "scalar 0 must have semantics='diffusion'"),
    (("opencl", "periodic"), [("diffusion", "periodic"), ("opencl", "periodic")], "scalar 1 must have semantics='diffusion'"),
    (("opencl", "periodic"), [], "1..2 scalars"),
    (("opencl", "periodic"), [("diffusion", "periodic")] * 3, "1..2 scalars"),
))
def test_mismatches_raise_before_the_library_is_called(monkeypatch, flow, scalars, text):
    """Grid, boundary family and semantics are checked in Python: ValueError without a device (the library is never reached)."""
    from LB_D2Q9 import _native, coupled

    def unreachable():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_native, "lib", unreachable)
    with pytest.raises(ValueError, match=re.escape(text)):
        coupled.Advected_Scalars(_stub(*flow), [_stub(*s) for s in scalars])


def test_the_same_scalar_twice_raises(monkeypatch):
    from LB_D2Q9 import coupled
    s = _stub("diffusion", "periodic")
    with pytest.raises(ValueError, match="appears twice"):
        coupled.Advected_Scalars(_stub("opencl", "periodic"), [s, s])
