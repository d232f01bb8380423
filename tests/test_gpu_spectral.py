"""The spectral screened-Poisson solver and the Fisher lattice coupled to it on the MI355X, against the numpy model
(tests/spectral_model.py) and the fixtures recorded from it (tests/golden/sp_*.npz).

Shapes -- the smallest at which each thing can go wrong: (2, 3), (5, 3) one pass per radix; (4, 4), (8, 6) mixed radices; (30, 18)
mixed, not square, a lattice pitch above nx; (50, 50) the reference's default; (64, 48) a row of exactly one wave; (256, 5), (5, 256) a
long row over a short column and the other way round; (96, 250) mixed radices, both axes longer than a wave; (4096, 4), (4, 4096)
the limit on each axis.  Of these only the last two have a batch (cols = 16, rows = 16), and their batched axis is one radix-4 pass
whose every twiddle is tw[0].

Batched shapes (BATCHED) -- a workgroup takes `rows` whole rows or `cols` adjacent columns where an axis has 512 points or more
(spectral_plan.cpp); each is the smallest that reaches its case; rows (ny % rows), cols (nx % cols), x passes, y passes, as
tests/test_spectral_cpu.py asks sp_plan itself:
    1 x 1, 1 x 6, 6 x 1   1, 1             an axis of one point: no pass at all
    625 x 48     1, 2 (1)   [5,5,5,5] [3,4,4]           the smallest ragged column batch; x = 5^4
    1000 x 30    1, 3 (1)   [5,5,5,4,2] [5,3,2]         an everyday width, ragged
    800 x 640    1, 3 (2)   [5,5,4,4,2] [5,4,4,4,2]     two columns missing from the last block; an odd number of batched passes
    48 x 1000    3 (1), 1   [3,4,4] [5,5,5,4,2]         a ragged row batch
    250 x 625    2 (1), 1   [5,5,5,2] [5,5,5,5]         a row batch of four passes; y = 5^4
    64 x 3750    14 (12), 1 [4,4,4] [5,5,5,5,3,2]       a large ragged row batch; 60000 B of column LDS
    6 x 2187     8 (3), 1   [3,2] [3 x 7]               y = 3^7
    3125 x 6     1, 12 (5)  [5 x 5] [3,2]               x = 5^5; a wide ragged column batch
    3600 x 3     1, 14 (2)  [5,5,3,3,4,4] [3]           every radix but 2 in one axis
    4096 x 250   1, 16 (0)  [4 x 6] [5,5,5,2]           the widest batch there is: 64000 B of column LDS, 65536 B of row LDS
    512 x 2048   2 (0), 2 (0) [4,4,4,4,2] [4,4,4,4,4,2] both passes batched; column LDS exactly 65536 B with two columns
The ragged ones also: a charge that lives in the last column or row only, and transforms of one array beside sentinels in the two others.
The coupled calls (the real plane in, u and v out: k_sp_rows_fwd<true>, k_sp_rows_inv<true>) at 48 x 1000, 1000 x 30 and 250 x 625,
bitwise where the small shapes are and against the float64 model within the contract.

Accuracy: E = max |got - m64| / max |m64| against the float64 model, for the screened spectrum, for the gradient (both components
over max |grad phi|: it is one vector field, and one component of a single mode is exactly zero) and for a forward / inverse round
trip; E_gpu <= 4 max(E_numpy32, 2^-23), E_numpy32 the complex64 numpy model's error on the same input: two bits for a radix order
other than pocketfft's, both being O(eps log n).  Every figure is printed before it is asserted (`pytest -s`).

Bitwise: the fused solve = the phases; lb_spectral_velocity(..., 0) = float32(scale Re grad) of the solve; lb_run_screened(n) = n x
(lb_spectral_velocity(..., 1), lb_run(1)).  Contract (scalar_model.contract_tol): lb_run_screened, the phase sequence and the
Screened_Fisher_Wave class against the fixtures at steps 1, 10, 50, both families.  On an external stream the coupled calls equal
their waiting twin (a child process in the style of tests/stream_scenarios.py, whose prelude it borrows).
"""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

import spectral_model as M
import stream_scenarios as S
from conftest import ROOT, golden
from scalar_model import contract_tol

pytestmark = pytest.mark.gpu

PLAIN = [(2, 3), (5, 3), (4, 4), (8, 6), (30, 18), (50, 50), (64, 48), (256, 5), (5, 256), (96, 250), (4096, 4), (4, 4096)]
BATCHED = [(1, 1), (1, 6), (6, 1), (625, 48), (1000, 30), (800, 640), (48, 1000), (250, 625), (64, 3750), (6, 2187), (3125, 6), (3600, 3),
           (4096, 250), (512, 2048)]
SHAPES = PLAIN + BATCHED
RAGGED = [(625, 48), (48, 1000), (64, 3750), (3125, 6)]          # a last column block / row block with padding, narrow and wide
EPS = 2. ** -23
LAM = 1.0


class Solver(object):
    """An lb_spectral through ctypes; arrays are (nx, ny) complex64, Fortran order = the device's [ny][nx]."""

    def __init__(self, lib, nx, ny, lam=LAM):
        from LB_D2Q9 import _native
        self.L, self.check, self.nx, self.ny = lib, _native.check, nx, ny
        self.h = ct.c_void_p()
        self.check(lib.lb_spectral_create(nx, ny, 0, float(lam), ct.byref(self.h)))

    def put(self, which, a):
        a = np.asfortranarray(np.asarray(a).astype(np.complex64))
        assert a.shape == (self.nx, self.ny)
        self.check(self.L.lb_spectral_set(self.h, which, a.ctypes.data, 0))

    def get(self, which):
        out = np.zeros((self.nx, self.ny), np.complex64, order='F')
        self.check(self.L.lb_spectral_get(self.h, which, out.ctypes.data))
        return out

    def all(self):
        return [self.get(w) for w in range(3)]

    def solve(self, charge):
        self.put(0, charge)
        self.check(self.L.lb_spectral_solve(self.h))
        return self.all()

    def phases(self, charge):
        self.put(0, charge)
        for call in ((self.L.lb_spectral_transform, 0, 1), (self.L.lb_spectral_screen,), (self.L.lb_spectral_grad_multiply,),
                     (self.L.lb_spectral_transform, 1, 0), (self.L.lb_spectral_transform, 2, 0)):
            self.check(call[0](self.h, *call[1:]))
        return self.all()

    def round_trip(self, charge):
        self.put(0, charge)
        self.check(self.L.lb_spectral_transform(self.h, 0, 1))
        self.check(self.L.lb_spectral_transform(self.h, 0, 0))
        return self.get(0)

    def close(self):
        if self.h.value:
            self.L.lb_spectral_destroy(self.h)
            self.h = ct.c_void_p()


@pytest.fixture(scope="module")
def solvers(lbhip):
    made = {}

    def get(nx, ny):
        if (nx, ny) not in made:
            made[(nx, ny)] = Solver(lbhip, nx, ny)
        return made[(nx, ny)]
    yield get
    for s in made.values():
        s.close()


def inputs(nx, ny):
    """name -> (nx, ny) float32 charge: a seeded noisy droplet, a delta, one low mode, the highest mode of the longer even axis."""
    X, Y = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    delta = np.zeros((nx, ny), np.float32)
    delta[nx // 3, ny // 2] = 1.
    low = np.cos(2 * np.pi * (X / float(nx) + Y / float(ny))).astype(np.float32)
    if nx % 2 == 0 and (ny % 2 or nx >= ny):
        nyq = np.cos(np.pi * X)
    elif ny % 2 == 0:
        nyq = np.cos(np.pi * Y)
    else:                                       # (no even axis: the highest mode there is)
        nyq = np.cos(2 * np.pi * (nx // 2) * X / float(nx))
    return dict(droplet=M.noisy_droplet(nx, ny, max(nx, ny) / 3., 0.5, 1000 * nx + ny), delta=delta, low=low,
                nyquist=nyq.astype(np.float32))


def over(err, top):
    """err / top; a field the model has identically zero (the gradient on a 1 x 1 box: its only wave index is 0) is held to err itself, the
    charges being of order one."""
    return err / top if top > 0 else err


def rel(got, want):
    return over(np.abs(np.asarray(got, np.complex128) - want).max(), np.abs(want).max())


def grad_rel(gx, gy, wx, wy):
    top = max(np.abs(wx).max(), np.abs(wy).max())
    return over(max(np.abs(np.asarray(gx, np.complex128) - wx).max(), np.abs(np.asarray(gy, np.complex128) - wy).max()), top)


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_accuracy_of_the_solve_and_of_a_round_trip(solvers, nx, ny):
    sp = solvers(nx, ny)
    bad = []
    for name, charge in sorted(inputs(nx, ny).items()):
        w = M.solve(charge, LAM)
        n32 = M.solve(charge, LAM, np.complex64)
        g = sp.solve(charge)
        figures = [("spectrum", rel(g[0], w[0]), rel(n32[0], w[0])),
                   ("gradient", grad_rel(g[1], g[2], w[1], w[2]), grad_rel(n32[1], n32[2], w[1], w[2])),
                   ("round trip", rel(sp.round_trip(charge), M.round_trip(charge)), rel(M.round_trip(charge, np.complex64), M.round_trip(charge)))]
        for what, e_gpu, e_np in figures:
            print("ACCURACY %4d x %-4d %-8s %-10s E_gpu %.3e E_numpy32 %.3e ratio %.2f bound %.3e"
                  % (nx, ny, name, what, e_gpu, e_np, e_gpu / max(e_np, 1e-30), 4 * max(e_np, EPS)))
            if not e_gpu <= 4 * max(e_np, EPS):
                bad.append((name, what, e_gpu, e_np))
    assert bad == []


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_the_fused_solve_equals_the_phases_bitwise(solvers, nx, ny):
    sp = solvers(nx, ny)
    for name, charge in sorted(inputs(nx, ny).items()):
        fused, phased = sp.solve(charge), sp.phases(charge)
        for which, a, b in zip(("charge", "xgrad", "ygrad"), fused, phased):
            assert a.tobytes() == b.tobytes(), (name, which, int((a != b).sum()))
        assert np.isfinite(fused[1].real).all() and np.isfinite(fused[1].imag).all()


def test_the_nyquist_gradient_keeps_its_imaginary_part(solvers):
    """Re xgrad of the Nyquist mode is zero, its imaginary part is not (the reference's -n/2 convention)."""
    nx, ny = 30, 18
    X, _ = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    _, xg, _ = solvers(nx, ny).solve(np.cos(np.pi * X))
    want = 2 * np.pi * 15 / (1. + 15 ** 2)
    assert np.abs(xg.real).max() <= 8 * EPS * want and abs(np.abs(xg.imag).max() - want) <= 8 * EPS * want


def sentinel(nx, ny, k):
    """(nx, ny) complex64 without a NaN, no two elements alike, none like another k's."""
    a = (np.arange(2 * nx * ny, dtype=np.float64) + 1.) * (k + 2) + 0.25 * (k + 1)
    a = np.where(np.arange(2 * nx * ny) % 2, -a, a).astype(np.float32)
    return np.asfortranarray(a.view(np.complex64).reshape((nx, ny), order='F'))


@pytest.mark.parametrize("nx,ny", RAGGED)
def test_a_ragged_last_batch_neither_leaks_its_padding_nor_leaves_the_array(solvers, nx, ny):
    """The last block of the batched axis is zero-filled past the array and guarded on the way out.  A charge that lives in the last
    column only, and one in the last row only -- the padding's neighbours in LDS --, solve to the float64 model within the accuracy
    test's bound; a transform of one array, forward or inverse, leaves the two other arrays' bits alone and changes its own."""
    sp = solvers(nx, ny)
    rng = np.random.RandomState(nx + ny)
    bad = []
    for name, sel in (("last column", (nx - 1, slice(None))), ("last row", (slice(None), ny - 1))):
        charge = np.zeros((nx, ny), np.float32)
        charge[sel] = 1. + 0.5 * rng.standard_normal(charge[sel].shape)
        w, n32, g = M.solve(charge, LAM), M.solve(charge, LAM, np.complex64), sp.solve(charge)
        for what, e_gpu, e_np in (("spectrum", rel(g[0], w[0]), rel(n32[0], w[0])),
                                  ("gradient", grad_rel(g[1], g[2], w[1], w[2]), grad_rel(n32[1], n32[2], w[1], w[2]))):
            print("ACCURACY %4d x %-4d %-11s %-10s E_gpu %.3e E_numpy32 %.3e ratio %.2f bound %.3e"
                  % (nx, ny, name, what, e_gpu, e_np, e_gpu / max(e_np, 1e-30), 4 * max(e_np, EPS)))
            if not e_gpu <= 4 * max(e_np, EPS):
                bad.append((name, what, e_gpu, e_np))
    assert bad == []
    marks = [sentinel(nx, ny, k) for k in range(3)]
    for which in range(3):
        for forward in (1, 0):
            for k in range(3):
                sp.put(k, marks[k])
            sp.check(sp.L.lb_spectral_transform(sp.h, which, forward))
            after = sp.all()
            for k in range(3):
                same = after[k].tobytes() == marks[k].tobytes()
                assert same == (k != which), (which, forward, k)


# ---- the coupling to a scalar lattice ---------------------------------------------------------------------------------------
FIELDS = ("f", "rho", "u", "v")


def lattice(nx, ny, omega, G, bc, rho0, sp, scale):
    """A diffusion handle set up as Screened_Fisher_Wave.redo_initial_condition does: rho, the velocity it gives itself, feq, f = feq."""
    from LB_D2Q9 import _native
    from LB_D2Q9.simulation import Simulation
    sim = Simulation(nx, ny, omega, bc=bc, semantics="diffusion")
    sim.set_reaction(float(G))
    zero = np.zeros((nx, ny), np.float32)
    sim.set_fields(rho0, zero, zero)
    _native.check(sp.L.lb_spectral_velocity(sp.h, sim._h, float(scale), 0))
    sim.update_feq()
    sim.init_pop()
    return sim


def case(nx, ny):
    """(omega, G, scale, rho0): the fixtures' parameters on any box."""
    p = M.fisher_lattice_parameters(1., 1., 1., 1., 10)
    return p["omega"], p["lb_G"], p["scale"], M.noisy_droplet(nx, ny, max(nx, ny) / 3., 0.5, 7 * nx + ny)


@pytest.mark.parametrize("nx,ny", [(30, 18), (5, 3), (64, 48), (48, 1000), (1000, 30)])
def test_the_velocity_is_the_float32_product_with_the_solves_gradient(solvers, nx, ny):
    from LB_D2Q9 import _native
    sp = solvers(nx, ny)
    omega, G, scale, rho0 = case(nx, ny)
    sim = lattice(nx, ny, omega, G, "open", rho0, sp, scale)
    got = sim.get_fields(("rho", "u", "v"))
    _, xg, yg = sp.solve(rho0)
    assert np.array_equal(got["rho"], rho0)
    assert np.array_equal(got["u"], np.float32(scale) * xg.real) and np.array_equal(got["v"], np.float32(scale) * yg.real)
    assert np.abs(got["u"]).max() > 0
    # streamed = 1: the density after streaming, stored in rho; nothing moves
    f_before = sim.get_fields(("f",))["f"]
    _native.check(sp.L.lb_spectral_velocity(sp.h, sim._h, float(scale), 1))
    after = sim.get_fields(FIELDS)
    twin = lattice(nx, ny, omega, G, "open", rho0, sp, scale)
    twin.move()
    twin.update_hydro()
    rho_s = twin.get_fields(("rho",))["rho"]
    assert np.array_equal(after["f"], f_before) and np.array_equal(after["rho"], rho_s)
    _, xg, yg = sp.solve(rho_s)
    assert np.array_equal(after["u"], np.float32(scale) * xg.real) and np.array_equal(after["v"], np.float32(scale) * yg.real)
    sim.close()
    twin.close()


@pytest.mark.parametrize("bc", ["open", "periodic"])
@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("nx,ny", [(30, 18), (5, 3), (48, 1000), (1000, 30)])
def test_run_screened_equals_the_pairs_of_calls_bitwise(solvers, nx, ny, n, bc):
    from LB_D2Q9 import _native
    sp = solvers(nx, ny)
    omega, G, scale, rho0 = case(nx, ny)
    a = lattice(nx, ny, omega, G, bc, rho0, sp, scale)
    b = lattice(nx, ny, omega, G, bc, rho0, sp, scale)
    _native.check(sp.L.lb_run_screened(sp.h, a._h, float(scale), n))
    for _ in range(n):
        _native.check(sp.L.lb_spectral_velocity(sp.h, b._h, float(scale), 1))
        _native.check(sp.L.lb_run(b._h, 1))
    fa, fb = a.get_fields(FIELDS), b.get_fields(FIELDS)
    for k in FIELDS:
        assert np.array_equal(fa[k].view(np.uint32), fb[k].view(np.uint32)), (k, int((fa[k] != fb[k]).sum()))
    assert not np.array_equal(fa["rho"], rho0)
    a.close()
    b.close()


def within_contract(got, g, bc, n, what):
    tol = contract_tol(n)
    bad = []
    for k in FIELDS:
        d = np.abs(got[k].astype(np.float64) - g["%s_%s_%d" % (bc, k, n)]).max()
        print("CONTRACT %-22s %-8s step %2d %-3s %.3e (tolerance %.3e)" % (what, bc, n, k, d, tol[k]))
        if not d <= tol[k]:
            bad.append((k, n, d, tol[k]))
    return bad


@pytest.mark.parametrize("bc", ["open", "periodic"])
def test_run_screened_follows_the_fixture(solvers, bc):
    from LB_D2Q9 import _native
    g = golden("sp_fisher_30x18")
    sp = solvers(30, 18)
    sim = lattice(30, 18, g["omega"], g["G"], bc, g["rho0"], sp, g["scale"])
    bad, done = [], 0
    for n in (int(s) for s in g["steps"]):
        _native.check(sp.L.lb_run_screened(sp.h, sim._h, float(g["scale"]), n - done))
        done = n
        bad += within_contract(sim.get_fields(FIELDS), g, bc, n, "lb_run_screened")
    assert bad == []
    if bc == "periodic":
        # total mass under growth: one more step adds G sum rho (1 - rho); each sum is off by at most a cell's single-step tolerance a cell
        rho50 = sim.get_fields(("rho",))["rho"].astype(np.float64)
        _native.check(sp.L.lb_run_screened(sp.h, sim._h, float(g["scale"]), 1))
        rho51 = sim.get_fields(("rho",))["rho"].astype(np.float64)
        grown, law = rho51.sum() - rho50.sum(), float(g["G"]) * (rho50 * (1. - rho50)).sum()
        print("MASS grown %.6e law %.6e" % (grown, law))
        assert law > 0.05 and abs(grown - law) <= 2 * rho50.size * contract_tol(1)["rho"]
        # (lb_check sums the populations the step left: its growth term is in them)
        after = rho51.sum() + float(g["G"]) * (rho51 * (1. - rho51)).sum()
        assert abs(sim.check()["sum_rho"] - after) <= 2 * rho50.size * contract_tol(1)["rho"]
    sim.close()


@pytest.mark.parametrize("bc", ["open", "periodic"])
@pytest.mark.parametrize("nx,ny", [(1000, 30), (48, 1000), (250, 625)])
def test_run_screened_follows_the_model_through_the_batched_kernels(solvers, nx, ny, bc):
    """No fixture at these sizes: the float64 model from the same float32 droplet, started as lattice() starts, after 1 and 5 steps
    within the contract.  The real plane in and u, v out go through row batches of 3 (ragged) and 2 (ragged), the columns through a
    ragged batch of 3."""
    from LB_D2Q9 import _native
    sp = solvers(nx, ny)
    omega, G, scale, rho0 = case(nx, ny)
    m = M.ScreenedFisherModel(nx, ny, omega, G, LAM, scale, bc=bc, dtype=np.float64)
    m.redo_initial_condition(rho0)
    sim = lattice(nx, ny, omega, G, bc, rho0, sp, scale)
    bad, done = [], 0
    for n in (1, 5):
        _native.check(sp.L.lb_run_screened(sp.h, sim._h, float(scale), n - done))
        m.run(n - done)
        done = n
        top = float(np.sqrt(m.u ** 2 + m.v ** 2).max())
        print("MODEL %d x %d %s step %d max |u| %.3f" % (nx, ny, bc, n, top))
        assert top < 0.2
        want = {"%s_%s_%d" % (bc, k, n): getattr(m, k) for k in FIELDS}
        bad += within_contract(sim.get_fields(FIELDS), want, bc, n, "run_screened %dx%d" % (nx, ny))
    assert bad == []
    sim.close()


@pytest.mark.parametrize("bc", ["open", "periodic"])
def test_the_phase_sequence_follows_the_fixture(solvers, bc):
    from LB_D2Q9 import _native
    g = golden("sp_fisher_30x18")
    sp = solvers(30, 18)
    sim = lattice(30, 18, g["omega"], g["G"], bc, g["rho0"], sp, g["scale"])
    bad = []
    for n in range(1, 51):
        sim.move()
        sim.update_hydro()
        _native.check(sp.L.lb_spectral_velocity(sp.h, sim._h, float(g["scale"]), 0))
        sim.update_feq()
        sim.collide_particles()
        if n in (1, 10, 50):
            bad += within_contract(sim.get_fields(FIELDS), g, bc, n, "the phases")
    assert bad == []
    sim.close()


def test_the_class_end_to_end(lbhip):
    from LB_D2Q9.reaction_diffusion.screened_poisson_waves import Screened_Fisher_Wave
    g = golden("sp_fisher_30x18")
    kw = dict(Lx=3., Ly=1.8, vc=1., lam=1., R0=0.5, time_prefactor=1., N=10)
    w = Screened_Fisher_Wave(check_max_ulb=True, **kw)
    assert (w.nx, w.ny) == (30, 18) and w.omega == g["omega"] and w.lb_G == g["G"]
    # its own droplet against the model, fused and by the phase methods
    m = M.ScreenedFisherModel(30, 18, w.omega, w.lb_G, 1., w.velocity_scale, dtype=np.float64)
    m.redo_initial_condition(np.asarray(w.rho))
    start = w.get_fields()
    assert np.abs(start["u"] - m.u).max() <= contract_tol(1)["u"] and np.abs(start["f"] - m.f).max() <= contract_tol(1)["f"]
    w.run(5)
    for _ in range(5):
        w.move(); w.move_bcs(); w.update_hydro(); w.update_feq(); w.collide_particles()
    m.run(10)
    got, tol = w.get_fields(), contract_tol(10)
    for k in FIELDS:
        assert np.abs(got[k] - getattr(m, k)).max() <= tol[k], k
    nd = w.get_nondim_fields()
    assert np.allclose(nd["u"], got["u"] * (w.delta_x / w.delta_t), rtol=1e-6, atol=0)
    # the fixture's noisy droplet through redo_initial_condition
    w.redo_initial_condition(g["rho0"])
    w.run(10)
    assert within_contract(w.get_fields(), g, "open", 10, "Screened_Fisher_Wave") == []
    # the solver class on its own: the reference's methods against the fixture of the solve
    from LB_D2Q9.spectral_poisson import Screened_Poisson
    s = golden("sp_solve_30x18")
    ps = Screened_Poisson(s["charge"], lam=float(s["lam"]), dx=0.1)
    ps.create_grad_fields()
    ps.solve_and_update_grad_fields()
    fused = [np.asarray(a) for a in (ps.charge, ps.xgrad, ps.ygrad)]
    assert fused[0].dtype == np.complex64 and fused[0].shape == (30, 18) and fused[0].flags.f_contiguous
    ps.charge.set(s["charge"])
    ps.fft_and_screen()
    ps.update_grad_fields()
    for a, b in zip(fused, (ps.charge, ps.xgrad, ps.ygrad)):
        assert np.array_equal(a, np.asarray(b))
    n32 = M.solve(s["charge"], float(s["lam"]), np.complex64)
    assert grad_rel(fused[1], fused[2], s["xgrad"], s["ygrad"]) <= 4 * max(grad_rel(n32[1], n32[2], s["xgrad"], s["ygrad"]), EPS)
    assert np.abs(ps.rescaling - M.rescaling(30, 18, 1.)).max() <= 1e-12 and np.abs(ps.freq_X - M.wave_grids(30, 18)[0]).max() <= 1e-10
    ps.inverse_fft()
    want = np.fft.ifft2(s["spec"])
    assert rel(np.asarray(ps.charge), want) <= 4 * max(rel(np.fft.ifft2(n32[0]), want), EPS)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_mismatched_handles_are_refused(lbhip, solvers):
    from LB_D2Q9.simulation import Simulation
    sp = solvers(30, 18)
    flow = Simulation(30, 18, 1.0, bc="periodic")
    other = Simulation(18, 30, 1.0, bc="open", semantics="diffusion")
    coupled = Simulation(30, 18, 1.0, bc="periodic", semantics="multifield")
    host = Simulation(30, 18, 1.0, bc="pipe", semantics="cython", device=-1)
    for sim, code, word in ((flow, -3, "scalar lattices (LB_SEM_DIFFUSION)"), (coupled, -3, "scalar lattices (LB_SEM_DIFFUSION)"),
                            (other, -1, "30 x 18"), (host, -3, "CPU backend")):
        for call in (lambda: lbhip.lb_spectral_velocity(sp.h, sim._h, 1.0, 0), lambda: lbhip.lb_run_screened(sp.h, sim._h, 1.0, 1)):
            assert call() == code and word in lbhip.lb_last_error().decode(), (code, word, lbhip.lb_last_error())
    good = Simulation(30, 18, 1.0, bc="open", semantics="diffusion")
    assert lbhip.lb_run_screened(sp.h, good._h, 1.0, -1) == -1 and lbhip.lb_run_screened(sp.h, good._h, float("nan"), 1) == -1
    assert lbhip.lb_spectral_set(sp.h, 3, None, 0) == -1 and lbhip.lb_spectral_transform(sp.h, -1, 1) == -1
    for s in (flow, other, coupled, host, good):
        s.close()


# ---- on an external stream --------------------------------------------------------------------------------------------------
CHILD = r'''
CHILD = "SPECTRAL"
import spectral_model as M
NX, NY = 96, 250


def screened_case(bc, sp, scale, stream):
    p = M.fisher_lattice_parameters(1., 1., 1., 1., 10)
    rho0 = M.noisy_droplet(NX, NY, 40., 0.5, 5)
    sim = Simulation(NX, NY, p["omega"], bc=bc, semantics="diffusion")
    sim.set_reaction(float(p["lb_G"]))
    zero = np.zeros((NX, NY), np.float32)
    sim.set_fields(rho0, zero, zero)
    _native.check(L.lb_spectral_velocity(sp, sim._h, scale, 0))
    sim.update_feq()
    sim.init_pop()
    if stream is not None:
        sim.use_stream(stream)
    return sim


def chain(sim, sp, scale, wait):
    for _ in range(3):
        _native.check(L.lb_spectral_velocity(sp, sim._h, scale, 1))
        if wait: sim.sync()
        _native.check(L.lb_run(sim._h, 1))
        if wait: sim.sync()
    _native.check(L.lb_run_screened(sp, sim._h, scale, 5))
    if wait: sim.sync()
    _native.check(L.lb_spectral_velocity(sp, sim._h, scale, 0))
    if wait: sim.sync()


def spectrum(sp):
    out = np.zeros((NX, NY), np.complex64, order='F')
    _native.check(L.lb_spectral_get(sp, 0, out.ctypes.data))
    return out


@scenario
def screened_calls_on_an_external_stream():
    scale = -0.1
    for bc in ("open", "periodic"):
        sp_t, sp_s = ct.c_void_p(), ct.c_void_p()
        _native.check(L.lb_spectral_create(NX, NY, 0, 1.0, ct.byref(sp_t)))
        _native.check(L.lb_spectral_create(NX, NY, 0, 1.0, ct.byref(sp_s)))
        twin = screened_case(bc, sp_t, scale, None)
        chain(twin, sp_t, scale, True)
        want = twin.get_fields(("f", "rho", "u", "v"))
        want["spectrum"] = spectrum(sp_t)
        S_ = SIDE[0]
        sim = screened_case(bc, sp_s, scale, S_.cuda_stream)
        torch.cuda.synchronize()
        d = Delay(S_)
        chain(sim, sp_s, scale, False)
        d.done()
        spec = spectrum(sp_s)            # (before any wait of ours: the solver's own stream must be behind the lattice's work)
        torch.cuda.synchronize()
        d.check("screened chain on S, %s" % bc)
        got = sim.get_fields(("f", "rho", "u", "v"))
        got["spectrum"] = spec
        assert_same(got, want, "screened chain on S, %s" % bc)
        assert np.isfinite(got["f"]).all() and np.abs(got["u"]).max() > 0
        sim.use_stream(None)
        for s_ in (sim, twin):
            s_.close()
        for h in (sp_t, sp_s):
            _native.check(L.lb_spectral_destroy(h))
'''


def test_the_coupled_calls_on_an_external_stream_equal_their_waiting_twin(lbhip, tmp_path):
    script = tmp_path / "child_spectral.py"
    script.write_text(S.PRELUDE + CHILD + S.EPILOGUE)
    p = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "tests"), os.path.join(ROOT, "2d-lb_amd")],
                       capture_output=True, text=True, timeout=300)
    print("\n".join(l for l in p.stdout.splitlines() if l.startswith(("RATIO", "SCENARIO"))))
    assert p.returncode == 0 and "SPECTRAL_OK" in p.stdout and "SCENARIO screened_calls_on_an_external_stream OK" in p.stdout, \
        p.stdout[-2000:] + p.stderr[-4000:]
