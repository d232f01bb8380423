"""A numpy model of a set of Shan-Chen fluids in pull form, float32 or float64 (test infrastructure; not a test module).

What LB_D2Q9/multicomponent_multiphase/multi.cl computes per iteration of multi.py's Simulation_Runner.run, written for whole
arrays, one method per stage:
  move              per fluid, pull-stream; 'periodic' wraps, 'zero_gradient' is the reference's push `move`, which leaves the
                    links that would enter from outside as the streaming buffer last held them (all overwritten by move_bcs)
  move_bcs          'zero_gradient': every boundary cell := the interior cell (clamp(x, 1, nx-2), clamp(y, 1, ny-2))
  update_hydro      rho_i = sum f; u, v = sum f c / rho where rho > 1e-12, else 0
  forces            G_i := (g_i [+ field_i]) rho_i, then per table entry (i, j, G_int, potential, parameter), with
                    S_j = sum_k w_k c_k psi(rho_j(x + c_k)) (neighbour wrapped, or clamped to [0, n-1]):
                    G_i -= G_int psi(rho_i) S_j and G_j -= G_int psi(rho_j) S_i
  update_bary       u_b = sum_i (sum_k f_ik c_k + G_i / 2) / sum_i rho_i          (total density 0: NaN, as the reference)
  update_feq        feq_k = w_k rho_i (1 + 3 c.u_b + 4.5 (c.u_b)^2 - 1.5 u_b^2)
  collide           f_k (1 - omega_i) + omega_i feq_k + (1 - omega_i / 2) w_k (3 c.G_i + 9 (c.G_i)(c.u_b) - 3 u_b.G_i)
  react             per table entry, on the rho of update_hydro: ('eat', a, b, rate, cutoff): growth = rate rho_a rho_b where
                    |rho_a - rho_b| / (rho_a + rho_b) < cutoff; f_a += w growth, f_b -= w growth;
                    ('grow', a, lo, hi, rate): f_a += w rate where lo < rho_a < hi.  w is rounded to float32 there, as the
                    reference's kernels do even in float64.
It is the yardstick where no fixture reaches; against the fixtures recorded from the reference's C (tests/golden/mc_*.npz) it
is checked by tests/test_multifluid_cpu.py.

Arrays: (nx, ny, NP) / (nx, ny, NP, 9) of `dtype`; u_b, v_b (nx, ny).  1/cs^2 is the constant 3.
"""
import numpy as np

W64 = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
ZERO_DENSITY = 1e-12
POTENTIALS = ("linear", "shan_chen", "pow")


def psi(potential, par, rho):
    r = np.where(rho < 0, rho.dtype.type(0.), rho)
    T = rho.dtype.type
    if potential == "linear":
        return r
    if potential == "shan_chen":
        return (T(par) * (T(1.) - np.exp(-(r / T(par))))).astype(rho.dtype)
    if potential == "pow":
        return np.power(r, T(par)).astype(rho.dtype)
    raise ValueError(potential)


def psi_bounds(potential, par, rho_max):
    """(max psi, max |dpsi / drho|) for 0 <= rho <= rho_max."""
    if potential == "linear":
        return rho_max, 1.
    if potential == "shan_chen":
        return min(abs(par), rho_max), 1.
    a = float(par)
    return rho_max ** a, a * max(rho_max ** (a - 1.), 1.)


def force_bound(interactions, g, num_fluids, rho_max, tol_rho, eps=2. ** -24):
    """The bound on |G_i - G_i,ref| that follows from densities known to tol_rho, per fluid.  An increment is
    -G_int psi(rho_i) S_j with |S| <= (sum_k w_k |c_kx|) max psi = max psi / 3, so its error is at most
    |G_int| (dpsi |S| + psi dS) <= (2 / 3) |G_int| L max psi tol_rho, L = max |dpsi / drho|; the body force g_i rho_i adds
    |g_i| tol_rho; plus the float32 rounding of the terms themselves (a few eps of their size)."""
    out = np.zeros(num_fluids)
    for i in range(num_fluids):
        gi = float(np.abs(np.asarray(g[i], np.float64)).max()) if g is not None else 0.
        out[i] = gi * tol_rho + 4. * eps * gi * rho_max
    for (i, j, G_int, potential, par) in interactions:
        pmax, lip = psi_bounds(potential, float(par), rho_max)
        inc = (2. / 3.) * abs(float(G_int)) * lip * pmax * tol_rho + 8. * eps * abs(float(G_int)) * pmax * pmax / 3.
        out[int(i)] += inc
        out[int(j)] += inc
    return out


class MultifluidModel(object):
    def __init__(self, nx, ny, omegas, bc="periodic", dtype=np.float32):
        assert bc in ("periodic", "zero_gradient")
        T = self.T = dtype
        self.nx, self.ny, self.bc = int(nx), int(ny), bc
        self.omegas = [T(o) for o in np.atleast_1d(omegas)]
        self.np_ = n = len(self.omegas)
        self.w = W64.astype(T)
        self.g = [(T(0.), T(0.)) for _ in range(n)]
        self.field = [None] * n
        self.interactions, self.reactions = [], []
        z2, z3, z4 = (lambda: np.zeros((nx, ny), T)), (lambda: np.zeros((nx, ny, n), T)), (lambda: np.zeros((nx, ny, n, 9), T))
        self.f, self.fs, self.feq = z4(), z4(), z4()
        self.rho, self.u, self.v, self.Gx, self.Gy = z3(), z3(), z3(), z3(), z3()
        self.ub, self.vb = z2(), z2()

    def set_f(self, f):
        self.f = np.array(f, dtype=self.T).reshape(self.nx, self.ny, self.np_, 9)
        self.fs = self.f.copy()

    def set_body_force(self, i, gx, gy):
        self.g[i] = (self.T(gx), self.T(gy))

    def set_force_field(self, i, fx, fy):
        self.field[i] = None if fx is None else (np.array(fx, dtype=self.T), np.array(fy, dtype=self.T))

    # -- the stages ---------------------------------------------------------------------------------------------------------
    def move(self):
        new = self.fs.copy()
        for k in range(9):
            pulled = np.roll(self.f[:, :, :, k], (CX[k], CY[k]), axis=(0, 1))      # pulled[x, y] = f[x - cx, y - cy]
            if self.bc == "periodic":
                new[:, :, :, k] = pulled
            else:
                inside = np.ones((self.nx, self.ny), bool)
                if CX[k] == 1: inside[0, :] = False
                if CX[k] == -1: inside[-1, :] = False
                if CY[k] == 1: inside[:, 0] = False
                if CY[k] == -1: inside[:, -1] = False
                new[:, :, :, k] = np.where(inside[:, :, None], pulled, new[:, :, :, k])
        self.f, self.fs = new, new.copy()

    def move_bcs(self):
        if self.bc == "periodic":
            return
        xs = np.clip(np.arange(self.nx), 1, self.nx - 2)
        ys = np.clip(np.arange(self.ny), 1, self.ny - 2)
        self.f = self.f[xs][:, ys].copy()

    def moments(self):
        f = self.f
        rho = f[..., 0].copy()
        for k in range(1, 9):
            rho = rho + f[..., k]
        mx = f[..., 1] - f[..., 3] + f[..., 5] - f[..., 6] - f[..., 7] + f[..., 8]
        my = f[..., 2] - f[..., 4] + f[..., 5] + f[..., 6] - f[..., 7] - f[..., 8]
        return rho, mx, my

    def update_hydro(self):
        T = self.T
        rho, mx, my = self.moments()
        dense = rho > T(ZERO_DENSITY)
        with np.errstate(all="ignore"):
            self.u = np.where(dense, mx / rho, T(0.)).astype(T)
            self.v = np.where(dense, my / rho, T(0.)).astype(T)
        self.rho = rho

    def _shift(self, a, cx, cy):
        """a(x + cx, y + cy), wrapped or clamped to the box."""
        if self.bc == "periodic":
            return np.roll(a, (-cx, -cy), axis=(0, 1))
        xs = np.clip(np.arange(self.nx) + cx, 0, self.nx - 1)
        ys = np.clip(np.arange(self.ny) + cy, 0, self.ny - 1)
        return a[xs][:, ys]

    def stencil(self, p):
        sx, sy = np.zeros_like(p), np.zeros_like(p)
        for k in range(1, 9):
            q = self._shift(p, int(CX[k]), int(CY[k]))
            sx = sx + (self.w[k] * self.T(CX[k])) * q
            sy = sy + (self.w[k] * self.T(CY[k])) * q
        return sx, sy

    def forces(self):
        T = self.T
        Gx, Gy = np.zeros_like(self.rho), np.zeros_like(self.rho)
        for i in range(self.np_):
            gx = np.full((self.nx, self.ny), self.g[i][0], T)
            gy = np.full((self.nx, self.ny), self.g[i][1], T)
            if self.field[i] is not None:
                gx, gy = gx + self.field[i][0], gy + self.field[i][1]
            Gx[:, :, i], Gy[:, :, i] = gx * self.rho[:, :, i], gy * self.rho[:, :, i]
        for (i, j, G_int, potential, par) in self.interactions:
            i, j = int(i), int(j)
            p1, p2 = psi(potential, par, self.rho[:, :, i]), psi(potential, par, self.rho[:, :, j])
            s1x, s1y = self.stencil(p1)
            s2x, s2y = self.stencil(p2)
            Gx[:, :, i] = Gx[:, :, i] + s2x * (-(T(G_int) * p1))
            Gy[:, :, i] = Gy[:, :, i] + s2y * (-(T(G_int) * p1))
            Gx[:, :, j] = Gx[:, :, j] + s1x * (-(T(G_int) * p2))
            Gy[:, :, j] = Gy[:, :, j] + s1y * (-(T(G_int) * p2))
        self.Gx, self.Gy = Gx.astype(T), Gy.astype(T)

    def update_bary(self):
        T = self.T
        _, mx, my = self.moments()
        sx, sy, rs = (np.zeros((self.nx, self.ny), T) for _ in range(3))
        for i in range(self.np_):
            rs = rs + self.rho[:, :, i]
            sx = sx + mx[:, :, i] + T(0.5) * self.Gx[:, :, i]
            sy = sy + my[:, :, i] + T(0.5) * self.Gy[:, :, i]
        with np.errstate(all="ignore"):
            self.ub, self.vb = (sx / rs).astype(T), (sy / rs).astype(T)

    def update_feq(self):
        T = self.T
        usq = self.ub * self.ub + self.vb * self.vb
        for k in range(9):
            cu = T(CX[k]) * self.ub + T(CY[k]) * self.vb
            inner = T(1.) + T(3.) * cu + T(4.5) * cu * cu - T(1.5) * usq
            self.feq[:, :, :, k] = (self.w[k] * self.rho) * inner[:, :, None]

    def collide(self):
        T = self.T
        uG = self.Gx * self.ub[:, :, None] + self.Gy * self.vb[:, :, None]
        for i in range(self.np_):
            om = self.omegas[i]
            keep, hw = T(1.) - om, T(1.) - T(0.5) * om
            for k in range(9):
                cG = T(CX[k]) * self.Gx[:, :, i] + T(CY[k]) * self.Gy[:, :, i]
                cu = T(CX[k]) * self.ub + T(CY[k]) * self.vb
                inner = T(3.) * cG + T(9.) * cG * cu - T(3.) * uG[:, :, i]
                self.f[:, :, i, k] = self.f[:, :, i, k] * keep + om * self.feq[:, :, i, k] + (self.w[k] * hw) * inner

    def react(self):
        T = self.T
        w = W64.astype(np.float32).astype(T)
        for r in self.reactions:
            if r[0] == "eat":
                a, b, rate, cutoff = int(r[1]), int(r[2]), T(r[3]), T(r[4])
                ra, rb = self.rho[:, :, a], self.rho[:, :, b]
                with np.errstate(all="ignore"):
                    phi = np.abs((ra - rb) / (ra + rb))
                growth = np.where(phi < cutoff, rate * ra * rb, T(0.)).astype(T)
                self.f[:, :, a, :] = self.f[:, :, a, :] + w * growth[:, :, None]
                self.f[:, :, b, :] = self.f[:, :, b, :] - w * growth[:, :, None]
            else:
                a, lo, hi, rate = int(r[1]), T(r[2]), T(r[3]), T(r[4])
                ra = self.rho[:, :, a]
                growth = np.where((ra > lo) & (ra < hi), rate, T(0.)).astype(T)
                self.f[:, :, a, :] = self.f[:, :, a, :] + w * growth[:, :, None]

    STAGES = ("move", "move_bcs", "update_hydro", "forces", "update_bary", "update_feq", "collide", "react")

    def step(self):
        with np.errstate(invalid="ignore"):
            for name in self.STAGES:
                getattr(self, name)()

    def run(self, n):
        for _ in range(int(n)):
            self.step()

    def get_fields(self):
        return dict(f=self.f, feq=self.feq, rho=self.rho, u=self.u, v=self.v, u_bary=self.ub, v_bary=self.vb, Gx=self.Gx, Gy=self.Gy)


def from_fixture(g, dtype):
    """The model set up as a run fixture's header says, holding its f0."""
    m = MultifluidModel(int(g["nx"]), int(g["ny"]), g["omega"], bc=str(g["bc"]), dtype=dtype)
    for i, (gx, gy) in enumerate(g["g"]):
        m.set_body_force(i, gx, gy)
    m.interactions = [(int(r[0]), int(r[1]), r[2], POTENTIALS[int(r[3])], r[4]) for r in g["interactions"]]
    m.reactions = [("eat", int(r[1]), int(r[2]), r[3], r[4]) if int(r[0]) == 0 else ("grow", int(r[1]), r[3], r[4], r[5]) for r in g["reactions"]]
    if "f0" in g:
        m.set_f(g["f0"])
    return m
