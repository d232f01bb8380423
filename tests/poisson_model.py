"""A numpy float32 model of the LB Poisson solver in pull form (test infrastructure; not a test module).

What LB_D2Q9/D2Q9_poisson.cl computes per iteration of poisson/solver.py's run loop, written for whole arrays: stream
(pull), the prescribed-value rule on the four walls and in the corners, rho = (9/5)(f1 + ... + f8), feq_0 = (w0 - 1) rho,
feq_k = w_k rho, f = f (1 - omega) + omega feq + w_k source react_factor; then the reference's convergence ratio
mean |rho - rho_before| / mean rho_before, in float64.
  the box   a link whose source cell lies outside keeps what the streaming buffer held (move + copy_buffer); on a wall the
            three links pointing into the box, and in a corner three of the five, are then replaced by w_k R with
            R = -(sum of the cell's five other non-rest links + (w0 - 1) rho_on_boundary) / (sum of the three weights).
            Two links per corner are neither streamed nor written, and the corner's rule reads them: the corner state,
            eight floats in the ABI's order (include/lb_hip.h; LB_BC_BOX's links).
Against the fixtures recorded from the reference's C (tests/golden/ps_*.npz) and against a literal push + copy +
cell-by-cell restatement it is checked by tests/test_poisson_cpu.py.

Arrays: (nx, ny) / (nx, ny, 9) of `dtype` (float32; float64 for judging the reference's own rounding).  Every scalar has
that type and every operation is one operation of that type.
"""
import numpy as np

from multifield_model import CORNER_LINKS
from scalar_model import CX, CY, F, W, contract_tol  # noqa: F401


class PoissonModel(object):
    def __init__(self, nx, ny, omega, rho_on_boundary=0., react_factor=1., dtype=F):
        T = self.T = dtype
        self.nx, self.ny = int(nx), int(ny)
        self.omega, self.rho_on_boundary, self.react_factor = T(F(omega)), T(F(rho_on_boundary)), T(F(react_factor))
        self.w = W.astype(T) if T is F else np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
        self.f = np.zeros((nx, ny, 9), T)
        self.stale = np.zeros((nx, ny, 9), T)          # the populations as last set; only never-streamed links are read
        self.feq = np.zeros((nx, ny, 9), T)
        self.rho = np.zeros((nx, ny), T)
        self.rho_before = np.zeros((nx, ny), T)
        self.source = np.zeros((nx, ny), T)
        self.iterations = 0                            # since the last solve_reset
        self.ratio = float("nan")
        x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
        self.wall = dict(w=x == 0, e=x == nx - 1, s=y == 0, n=y == ny - 1)

    def set_f(self, f):
        self.f = np.array(f, dtype=self.T)
        self.stale = self.f.copy()

    def set_source(self, source):
        self.source = np.array(source, dtype=self.T)

    def solve_reset(self):
        self.iterations = 0

    def get_corner_state(self):
        return np.array([self.stale[x, y, k] for k, x, y in CORNER_LINKS], self.T)

    def set_corner_state(self, values):
        for j, (k, x, y) in enumerate(CORNER_LINKS):
            self.stale[x, y, k] = self.T(values[j])

    # -- the phases -------------------------------------------------------------------------------------------------------
    def outside(self, k):
        """cells whose link k would be pulled from outside the box"""
        o = np.zeros((self.nx, self.ny), bool)
        if CX[k] == 1: o[0, :] = True
        if CX[k] == -1: o[-1, :] = True
        if CY[k] == 1: o[:, 0] = True
        if CY[k] == -1: o[:, -1] = True
        return o

    def move(self):
        new = np.empty_like(self.f)
        for k in range(9):
            pulled = np.roll(self.f[:, :, k], (CX[k], CY[k]), axis=(0, 1))      # new[x, y] = f[x - cx, y - cy]
            new[:, :, k] = np.where(self.outside(k), self.stale[:, :, k], pulled)
        self.f = new

    def written(self):
        """[k] -> the cells whose link k move_bcs writes: it enters from outside, and in a corner it is not one of the two
        diagonals that run along the corner's other wall"""
        w, e, s, n = (self.wall[c] for c in "wesn")
        return [None, w, s, e, n, (w | s) & ~(e | n), (e | s) & ~(w | n), (e | n) & ~(w | s), (w | n) & ~(e | s)]

    def move_bcs(self):
        T, wr = self.T, self.written()
        w, e, s, n = (self.wall[c] for c in "wesn")
        total = np.zeros((self.nx, self.ny), T)
        for k in range(1, 9):                           # the five links read, in ascending order (a written one adds an exact 0)
            total = total + np.where(wr[k], T(0), self.f[:, :, k])
        w1, w2 = self.w[1], self.w[5]
        den = np.where((w | e) & (s | n), (w1 + w1) + w2, (w1 + w2) + w2).astype(T)
        R = -(total + (T(-1) + self.w[0]) * self.rho_on_boundary) / den
        for k in range(1, 9):
            self.f[:, :, k] = np.where(wr[k], self.w[k] * R, self.f[:, :, k])

    def update_hydro(self):
        total = self.f[:, :, 1].copy()
        for k in range(2, 9):
            total = total + self.f[:, :, k]
        self.rho = (self.T(9.) / self.T(5.)) * total

    def update_feq(self):
        self.feq[:, :, 0] = (self.w[0] - self.T(1)) * self.rho
        for k in range(1, 9):
            self.feq[:, :, k] = self.w[k] * self.rho

    def collide_particles(self):
        keep = self.T(1) - self.omega
        react = self.source * self.react_factor
        for k in range(9):
            self.f[:, :, k] = (self.f[:, :, k] * keep + self.omega * self.feq[:, :, k]) + self.w[k] * react

    def step(self):
        self.rho_before = self.rho.copy()
        self.move()
        self.move_bcs()
        self.update_hydro()
        self.update_feq()
        self.collide_particles()
        self.iterations += 1
        with np.errstate(all="ignore"):
            self.ratio = float(np.abs(self.rho_before.astype(np.float64) - self.rho).sum() / self.rho_before.astype(np.float64).sum())

    def run(self, n):
        for _ in range(int(n)):
            self.step()

    def solve(self, max_iterations, tolerance):
        """solver.py:333-358: (iterations made, converged, last ratio)"""
        for i in range(int(max_iterations)):
            self.step()
            if self.iterations != 1 and self.ratio < tolerance:
                return i + 1, True, self.ratio
        return int(max_iterations), False, self.ratio

    def gradient(self, dx=1.):
        """(d rho / dx, d rho / dy): central differences over 2 dx, 0 for a neighbour outside"""
        p = np.pad(self.rho, 1)
        inv = self.T(1) / (self.T(2) * self.T(dx))
        return (p[2:, 1:-1] - p[:-2, 1:-1]) * inv, (p[1:-1, 2:] - p[1:-1, :-2]) * inv

    def get_fields(self):
        return dict(f=self.f, feq=self.feq, rho=self.rho)
