"""A numpy model of a scalar lattice in pull form, float32 or float64 (test infrastructure; not a test module).

What LB_D2Q9/D2Q9_diffusion.cl computes per iteration of reaction_diffusion/diffusion.py's run loop, written for whole
arrays: stream (pull), rho = sum f, feq_k = w_k rho (1 + 3 c_k.u) with the imposed u, v, f = f (1 - omega) + omega feq
[+ w_k G rho (1 - rho)].  Two families:
  'periodic'  the box wraps in x and y;
  'open'      the reference's box: a link whose source cell lies outside keeps the value it had when the populations were
              last set (set_f) -- the reference's push `move` never writes it and copy_buffer restores it from f_streamed.
It is the yardstick where no fixture reaches (the periodic family, larger boxes, the coupling).  Against the fixtures
recorded from the reference's C (tests/golden/ad_*.npz) it is checked by tests/test_scalar_cpu.py.

Arrays: (nx, ny) / (nx, ny, 9) of `dtype` (float32 unless asked otherwise).  Every scalar is a `dtype` and every operation one
operation in it; 1/cs^2 is the constant 3 (the reference divides by cs*cs of its float32 cs).
"""
import numpy as np

F = np.float32
W = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4, dtype=np.float32)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])


def contract_tol(n_steps):
    """The project's parity contract, restated from tests/test_gpu_parity.py (n x the single-step bounds, capped at the
    envelope for <= 1000 steps)."""
    n = max(1, int(n_steps))
    return dict(f=min(2.5e-7 * n, 5e-6), rho=min(5e-7 * n, 1e-5), u=min(1e-6 * n, 5e-6), v=min(1e-6 * n, 5e-6))


def edge_index(nx, ny):
    """(k, x-indices, y-indices) of the twelve segments of the edge state, in the ABI's order (include/lb_hip.h)."""
    xs, ys = np.arange(nx), np.arange(ny)
    z = lambda n, val: np.full(n, val)
    west = [(k, z(ny, 0), ys) for k in (1, 5, 8)]
    east = [(k, z(ny, nx - 1), ys) for k in (3, 6, 7)]
    south = [(k, xs, z(nx, 0)) for k in (2, 5, 6)]
    north = [(k, xs, z(nx, ny - 1)) for k in (4, 7, 8)]
    return west, east, south, north


class ScalarModel(object):
    def __init__(self, nx, ny, omega, G=0., bc="open", dtype=F):
        assert bc in ("open", "periodic")
        T = self.T = np.dtype(dtype).type                 # (a scalar type: T(x) makes one value, whatever names the dtype)
        self.nx, self.ny, self.bc = int(nx), int(ny), bc
        self.omega, self.G = T(F(omega)), T(F(G))        # (the handle's parameters are float32)
        self.w = W if T == F else np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4, dtype=T)
        self.f = np.zeros((nx, ny, 9), T)
        self.frozen = np.zeros((nx, ny, 9), T)        # open: the populations as last set; only its edge links are ever read
        self.feq = np.zeros((nx, ny, 9), T)
        self.rho = np.zeros((nx, ny), T)
        self.u = np.zeros((nx, ny), T)
        self.v = np.zeros((nx, ny), T)

    def set_reaction(self, G):
        self.G = self.T(F(G))

    def set_fields(self, rho, u, v):
        self.rho, self.u, self.v = (np.array(a, dtype=self.T) for a in (rho, u, v))

    def set_f(self, f):
        self.f = np.array(f, dtype=self.T)
        self.frozen = self.f.copy()

    # -- edge state in the ABI's order ---------------------------------------------------------------------------------
    def get_edge_state(self):
        if self.bc != "open":
            return np.zeros(0, self.T)
        west, east, south, north = edge_index(self.nx, self.ny)
        return np.concatenate([self.frozen[x, y, k] for k, x, y in west + east + south + north]).astype(self.T)

    def set_edge_state(self, e):
        if self.bc != "open":
            return
        e = np.asarray(e, self.T)
        west, east, south, north = edge_index(self.nx, self.ny)
        cols, rows = west + east, south + north
        o = sum(len(x) for _, x, _ in cols)
        for k, x, y in rows:                           # rows first: where a corner link has two entries the column's counts
            self.frozen[x, y, k] = e[o:o + len(x)]
            o += len(x)
        o = 0
        for k, x, y in cols:
            self.frozen[x, y, k] = e[o:o + len(x)]
            o += len(x)

    # -- the phases -------------------------------------------------------------------------------------------------------
    def move(self):
        new = np.empty_like(self.f)
        for k in range(9):
            pulled = np.roll(self.f[:, :, k], (CX[k], CY[k]), axis=(0, 1))      # new[x, y] = f[x - cx, y - cy]
            if self.bc == "open":
                outside = np.zeros((self.nx, self.ny), bool)
                if CX[k] == 1: outside[0, :] = True
                if CX[k] == -1: outside[-1, :] = True
                if CY[k] == 1: outside[:, 0] = True
                if CY[k] == -1: outside[:, -1] = True
                pulled = np.where(outside, self.frozen[:, :, k], pulled)
            new[:, :, k] = pulled
        self.f = new

    def update_hydro(self):
        rho = self.f[:, :, 0].copy()
        for k in range(1, 9):
            rho = rho + self.f[:, :, k]
        self.rho = rho

    def update_feq(self):
        T = self.T
        for k in range(9):
            cu = T(CX[k]) * self.u + T(CY[k]) * self.v
            self.feq[:, :, k] = self.w[k] * self.rho * (T(1.) + cu * T(3.))

    def collide_particles(self):
        T = self.T
        keep = T(1.) - self.omega
        react = self.G * self.rho * (T(1.) - self.rho)
        for k in range(9):
            new = self.f[:, :, k] * keep + self.omega * self.feq[:, :, k]
            if self.G != 0:
                new = new + self.w[k] * react
            self.f[:, :, k] = new

    def step(self):
        self.move()
        self.update_hydro()
        self.update_feq()
        self.collide_particles()

    def run(self, n):
        for _ in range(int(n)):
            self.step()

    def get_fields(self):
        return dict(f=self.f, feq=self.feq, rho=self.rho, u=self.u, v=self.v)
