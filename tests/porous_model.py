"""A numpy model of forced flow in a porous medium in pull form, float32 or float64 (test infrastructure; not a test module).

What LB_D2Q9/porous_media/single_component.cl computes per iteration of single_component.py's Simulation_Runner.run with one
fluid, written for whole arrays, one method per stage:
  move              pull-stream; 'periodic' wraps, 'zero_gradient' is the reference's push `move`, which leaves the links that
                    would enter from outside as the streaming buffer last held them (all of them overwritten by move_bcs)
  move_bcs          'zero_gradient': every boundary cell := the interior cell (clamp(x, 1, nx-2), clamp(y, 1, ny-2))
  update_hydro      rho = sum f; u, v = sum f c / rho where rho > 1e-6, else 0
  body_force        G := the constant force [+ the field]
  update_forces     G := eps G - eps nu u / K - eps Fe |u| u / sqrt(K) where rho > 1e-6, else 0
  update_bary       u_b = (sum f c + rho G / 2) / rho          (rho = 0: NaN, as the reference)
  update_feq        feq_k = w_k rho (1 + 3 c.u_b + 4.5 (c.u_b)^2 / eps - 1.5 u_b^2 / eps)
  collide           f_k (1 - omega) + omega feq_k + w_k rho (1 - omega / 2)(3 c.G + 9 (c.G)(c.u_b) / eps - 3 u_b.G / eps)
It is the yardstick where no fixture reaches; against the fixtures recorded from the reference's C (tests/golden/pm_*.npz)
it is checked by tests/test_porous_cpu.py.

Arrays: (nx, ny) / (nx, ny, 9) of `dtype`.  Every scalar is a `dtype` and every operation one operation in it; 1/cs^2 is
the constant 3 (the reference divides by cs*cs).
"""
import numpy as np

W64 = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
ZERO_DENSITY = 1e-6


def force_bound(header, max_speed, tol_u):
    """The bound on |G - G_ref| that follows from a velocity known to tol_u: G is eps (g - nu u / K - Fe |u| u / sqrt(K)), whose
    derivative with respect to u is at most eps (nu / K + 2 Fe max|u| / sqrt(K)); plus float32 rounding of G itself."""
    eps, nu, K, Fe = (float(header[k]) for k in ("epsilon", "nu_fluid", "K", "Fe"))
    return eps * (nu / K + 2. * Fe * max_speed / np.sqrt(K)) * tol_u


class PorousModel(object):
    def __init__(self, nx, ny, omega, epsilon=1., nu_fluid=0., K=1., Fe=0., bc="periodic", dtype=np.float32):
        assert bc in ("periodic", "zero_gradient")
        T = self.T = dtype
        self.nx, self.ny, self.bc = int(nx), int(ny), bc
        self.omega, self.eps, self.nu, self.K, self.Fe = T(omega), T(epsilon), T(nu_fluid), T(K), T(Fe)
        self.w = W64.astype(T)
        self.g = (T(0.), T(0.))
        self.field = None
        z2, z3 = (lambda: np.zeros((nx, ny), T)), (lambda: np.zeros((nx, ny, 9), T))
        self.f, self.fs, self.feq = z3(), z3(), z3()
        self.rho, self.u, self.v, self.Gx, self.Gy, self.ub, self.vb = z2(), z2(), z2(), z2(), z2(), z2(), z2()

    def set_f(self, f):
        self.f = np.array(f, dtype=self.T)
        self.fs = self.f.copy()

    def set_body_force(self, gx, gy):
        self.g = (self.T(gx), self.T(gy))

    def set_force_field(self, fx, fy):
        self.field = None if fx is None else (np.array(fx, dtype=self.T), np.array(fy, dtype=self.T))

    # -- the stages ---------------------------------------------------------------------------------------------------------
    def move(self):
        new = self.fs.copy()
        for k in range(9):
            pulled = np.roll(self.f[:, :, k], (CX[k], CY[k]), axis=(0, 1))      # pulled[x, y] = f[x - cx, y - cy]
            if self.bc == "periodic":
                new[:, :, k] = pulled
            else:
                inside = np.ones((self.nx, self.ny), bool)
                if CX[k] == 1: inside[0, :] = False
                if CX[k] == -1: inside[-1, :] = False
                if CY[k] == 1: inside[:, 0] = False
                if CY[k] == -1: inside[:, -1] = False
                new[:, :, k] = np.where(inside, pulled, new[:, :, k])
        self.f, self.fs = new, new.copy()

    def move_bcs(self):
        if self.bc == "periodic":
            return
        xs = np.clip(np.arange(self.nx), 1, self.nx - 2)
        ys = np.clip(np.arange(self.ny), 1, self.ny - 2)
        self.f = self.f[xs][:, ys].copy()

    def moments(self):
        f = self.f
        rho = f[:, :, 0].copy()
        for k in range(1, 9):
            rho = rho + f[:, :, k]
        mx = f[:, :, 1] - f[:, :, 3] + f[:, :, 5] - f[:, :, 6] - f[:, :, 7] + f[:, :, 8]
        my = f[:, :, 2] - f[:, :, 4] + f[:, :, 5] + f[:, :, 6] - f[:, :, 7] - f[:, :, 8]
        return rho, mx, my

    def update_hydro(self):
        T = self.T
        rho, mx, my = self.moments()
        dense = rho > T(ZERO_DENSITY)
        with np.errstate(all="ignore"):
            self.u = np.where(dense, mx / rho, T(0.)).astype(T)
            self.v = np.where(dense, my / rho, T(0.)).astype(T)
        self.rho = rho

    def body_force(self):
        self.Gx = np.full((self.nx, self.ny), self.g[0], self.T)
        self.Gy = np.full((self.nx, self.ny), self.g[1], self.T)
        if self.field is not None:
            self.Gx = self.Gx + self.field[0]
            self.Gy = self.Gy + self.field[1]

    def update_forces(self):
        T = self.T
        dense = self.rho > T(ZERO_DENSITY)
        mag = np.sqrt(self.u * self.u + self.v * self.v)
        sqrtK = np.sqrt(self.K)
        out = []
        for G, w in ((self.Gx, self.u), (self.Gy, self.v)):
            g = self.eps * G - ((self.eps * self.nu) * w) / self.K - (((self.eps * self.Fe) * mag) * w) / sqrtK
            out.append(np.where(dense, g, T(0.)).astype(T))
        self.Gx, self.Gy = out

    def update_bary(self):
        T = self.T
        _, mx, my = self.moments()
        with np.errstate(all="ignore"):
            self.ub = ((mx + T(0.5) * (self.rho * self.Gx)) / self.rho).astype(T)
            self.vb = ((my + T(0.5) * (self.rho * self.Gy)) / self.rho).astype(T)

    def update_feq(self):
        T = self.T
        usq = self.ub * self.ub + self.vb * self.vb
        for k in range(9):
            cu = T(CX[k]) * self.ub + T(CY[k]) * self.vb
            inner = T(1.) + T(3.) * cu + (T(4.5) * cu * cu) / self.eps - (T(1.5) * usq) / self.eps
            self.feq[:, :, k] = (self.w[k] * self.rho) * inner

    def collide(self):
        T = self.T
        keep = T(1.) - self.omega
        s = self.rho * (T(1.) - T(0.5) * self.omega)
        uG = self.Gx * self.ub + self.Gy * self.vb
        for k in range(9):
            cG = T(CX[k]) * self.Gx + T(CY[k]) * self.Gy
            cu = T(CX[k]) * self.ub + T(CY[k]) * self.vb
            inner = T(3.) * cG + (T(9.) * cG * cu) / self.eps - (T(3.) * uG) / self.eps
            self.f[:, :, k] = self.f[:, :, k] * keep + self.omega * self.feq[:, :, k] + (self.w[k] * s) * inner

    STAGES = ("move", "move_bcs", "update_hydro", "body_force", "update_forces", "update_bary", "update_feq", "collide")

    def step(self):
        with np.errstate(invalid="ignore"):
            for name in self.STAGES:
                getattr(self, name)()

    def run(self, n):
        for _ in range(int(n)):
            self.step()

    def get_fields(self):
        return dict(f=self.f, feq=self.feq, rho=self.rho, u=self.u, v=self.v, u_bary=self.ub, v_bary=self.vb, Gx=self.Gx, Gy=self.Gy)
