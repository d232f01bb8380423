"""A numpy model of coupled scalar lattices in pull form, float32 or float64 (test infrastructure; not a test module).

What LB_D2Q9/D2Q9_multifield_fisher.cl computes per iteration of advecting_range_expansion/deterministic_fisher_waves.py's run
loop, written for whole arrays: stream (pull), the box's bounce-back, rho_i = sum f, feq_k = w_k rho_i (1 + 3 c_k.u) with the
imposed u, v, f = f (1 - omega_i) + omega_i feq + w_k G_i rho_i (1 - rho_tot), rho_tot = rho_0 + rho_1 + ...  Two families:
  'periodic'  the box wraps in x and y;
  'box'       the reference's closed box: every link whose source cell lies outside is replaced by move_bcs's rule from
              post-stream links of the SAME cell (f1 := f3 at x = 0, ...); two links per corner are neither streamed nor
              bounced and keep the value they had when the populations were last set: the corner state, eight floats per
              field in the ABI's order (include/lb_hip.h).
Against the fixtures recorded from the reference's C (tests/golden/mf_*.npz) it is checked by tests/test_multifield_cpu.py.

Arrays: (nx, ny) / (nx, ny, nf) / (nx, ny, nf, 9) of `dtype` (float32 unless asked otherwise).  Every scalar is a `dtype` and every
operation one operation in it; 1/cs^2 is the constant 3, as in tests/scalar_model.py.
"""
import numpy as np

from scalar_model import CX, CY, F, W, contract_tol  # noqa: F401

# (k, x, y) of the corner state's eight links; x, y = 0 or -1 (the last column / row)
CORNER_LINKS = ((6, 0, 0), (8, 0, 0), (5, -1, 0), (7, -1, 0), (5, 0, -1), (7, 0, -1), (6, -1, -1), (8, -1, -1))
OPPOSITE = (0, 3, 4, 1, 2, 7, 8, 5, 6)


class MultifieldModel(object):
    def __init__(self, nx, ny, omegas, Gs, bc="box", dtype=F):
        assert bc in ("box", "periodic")
        T = self.T = np.dtype(dtype).type                 # (a scalar type: T(x) makes one value, whatever names the dtype)
        self.nx, self.ny, self.bc = int(nx), int(ny), bc
        self.omega, self.G = np.array(omegas, F).reshape(-1).astype(T), np.array(Gs, F).reshape(-1).astype(T)      # (the handles' parameters are float32)
        self.nf = len(self.omega)
        assert len(self.G) == self.nf
        self.w = W if T == F else np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4, dtype=T)
        self.f = np.zeros((nx, ny, self.nf, 9), T)
        self.stale = np.zeros((nx, ny, self.nf, 9), T)      # box: the populations as last set; only never-streamed links are read
        self.feq = np.zeros((nx, ny, self.nf, 9), T)
        self.rho = np.zeros((nx, ny, self.nf), T)
        self.u = np.zeros((nx, ny), T)
        self.v = np.zeros((nx, ny), T)

    def set_fields(self, rho, u, v):
        self.rho, self.u, self.v = (np.array(a, dtype=self.T) for a in (rho, u, v))

    def set_f(self, f):
        self.f = np.array(f, dtype=self.T)
        self.stale = self.f.copy()

    def get_corner_state(self):
        return np.stack([self.stale[x, y, :, k] for k, x, y in CORNER_LINKS], axis=1).astype(self.T)      # (nf, 8)

    def set_corner_state(self, values):
        values = np.asarray(values, self.T)
        for j, (k, x, y) in enumerate(CORNER_LINKS):
            self.stale[x, y, :, k] = values[:, j]

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
        """new[x, y] = f[x - cx, y - cy]; box: a link from outside keeps what the streaming buffer held (move + copy_buffer)"""
        new = np.empty_like(self.f)
        for k in range(9):
            pulled = np.roll(self.f[..., k], (CX[k], CY[k]), axis=(0, 1))
            if self.bc == "box":
                pulled = np.where(self.outside(k)[:, :, None], self.stale[..., k], pulled)
            new[..., k] = pulled
        self.f = new

    def move_bcs(self):
        """box: every link from outside := the opposite link of the same cell, post-stream -- except the two per corner that
        run along the corner's other wall (their opposite came from outside too): the rule skips them"""
        if self.bc != "box":
            return
        post = self.f.copy()
        for k in range(1, 9):
            o = self.outside(k)
            o &= ~self.outside(OPPOSITE[k])
            self.f[..., k] = np.where(o[:, :, None], post[..., OPPOSITE[k]], self.f[..., k])

    def update_hydro(self):
        rho = self.f[..., 0].copy()
        for k in range(1, 9):
            rho = rho + self.f[..., k]
        self.rho = rho

    def update_feq(self):
        T = self.T
        for k in range(9):
            cu = (T(CX[k]) * self.u + T(CY[k]) * self.v)[:, :, None]
            self.feq[..., k] = self.w[k] * self.rho * (T(1.) + cu * T(3.))

    def collide_particles(self):
        rho_tot = self.rho[..., 0].copy()
        for i in range(1, self.nf):
            rho_tot = rho_tot + self.rho[..., i]
        room = self.T(1.) - rho_tot
        for i in range(self.nf):
            keep = self.T(1.) - self.omega[i]
            react = (self.G[i] * self.rho[..., i]) * room
            for k in range(9):
                new = self.f[:, :, i, k] * keep + self.omega[i] * self.feq[:, :, i, k]
                if self.G[i] != 0:
                    new = new + self.w[k] * react
                self.f[:, :, i, k] = new

    def step(self):
        self.move()
        self.move_bcs()
        self.update_hydro()
        self.update_feq()
        self.collide_particles()

    def run(self, n):
        for _ in range(int(n)):
            self.step()

    def get_fields(self):
        return dict(f=self.f, feq=self.feq, rho=self.rho, u=self.u, v=self.v)
