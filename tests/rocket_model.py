"""A numpy model of a surfactant-propelled colony in pull form, float32 or float64 (test infrastructure; not a test module).

What LB_D2Q9/rocket_yeast/rocket_yeast.cl (mode 'flow') and rocket_yeast_forces_only.cl (mode 'forces') compute per iteration of
Rocket_Yeast.run (rocket_yeast.py:469-483), written for whole arrays, one method per stage.  Two scalar lattices in a periodic
box: index 0 the population p, index 1 the surfactant c.  With grad_w a (x) = sum_k w_k c_k a(x + c_k), the D2Q9 stencil with
periodic wrap, cs = float32(1 / sqrt(3)) and 1 / cs^2 = 1. / (cs cs) as the kernels form it:
  move              both lattices, pull-stream with wrap
  update_hydro      rho_i = sum_k f_ik, k = 0 ... 8
  'flow':
    update_velocity (u, v) = -epsilon (1 / cs^2) grad_w rho_c
    update_forces   psi = rho_o (1 - exp(-max(rho_p, 0) / rho_o)); F = -G_chen sum_k w_k c_k psi(x) psi(x + c_k)
  'forces' (forces first):
    update_forces   S = pow(1 - exp(-max(rho_c, 0) / c_o), alpha); F_s = -epsilon (1 / cs^2) grad_w S;
                    F_p = -G_chen ((1 / cs^2) grad_w rho_p) (rho_p - rho_o)
    update_velocity (u, v) = F_p + F_s
  update_feq        feq_ik = w_k rho_i (1 + c_k.u / cs^2)
  collide           population: max(0, f_k (1 - omega) + omega feq_k + w_k G rho_p (1 - rho_p) ['flow': + (w_k c_k.F) / cs^2]);
                    'forces': no growth where rho_p > 1.  Surfactant: f_k (1 - omega_c) + omega_c feq_k + w_k G_c rho_p.
It is the yardstick where no fixture reaches; against the fixtures recorded from the reference's C (tests/golden/ry_*.npz) it is
checked by tests/test_rocket_cpu.py.

Arrays: (nx, ny, 2) / (nx, ny, 2, 9) of `dtype`; u, v, psi / S and the forces (nx, ny).  F is `Fx, Fy`: the pseudo-force ('flow')
or the pressure force ('forces'); the surface force is `Sx, Sy`.
"""
import numpy as np

W64 = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CX = np.array([0, 1, 0, -1, 0, 1, -1, -1, 1])
CY = np.array([0, 0, 1, 0, -1, 1, 1, -1, -1])
CS32 = np.float32(1. / np.sqrt(3))
PARAMS = ("G", "G_c", "epsilon", "rho_o", "G_chen", "c_o", "alpha")
EPS32 = 2. ** -24


def rocket_bounds(mode, params, rho_max, tol_rho, eps=EPS32):
    """The bounds on psi / S and the forces that follow from densities known to tol_rho (each density; rho_max bounds both).

    A stencil over a quantity known to d is known to (sum_k w_k |c_kx|) d = d / 3, and is at most a third of the quantity's
    maximum.  1 / cs^2 = 3.
      psi   |dpsi / drho| <= 1: tol_rho.                  S   |dS / dc| <= alpha / c_o (alpha >= 1): (alpha / c_o) tol_rho.
      'flow'    F   = -G_chen psi grad_w psi: |G_chen| (d psi |grad psi| + psi d grad psi) <= (2 / 3) |G_chen| psi_max tol_rho,
                psi_max = min(|rho_o|, rho_max)
      'forces'  F_s = -epsilon 3 grad_w S: |epsilon| dS
                F_p = -G_chen 3 grad_w rho (rho - rho_o): |G_chen| (tol_rho D + rho_max tol_rho), D = max |rho - rho_o|
                      <= max(rho_max, |rho_o|)
    plus the float32 rounding of the terms themselves (a few eps of their size; expf and powf: a few ulp of a value <= 1 or rho_o)."""
    p = {k: abs(float(params[k])) for k in PARAMS}
    if mode == "flow":
        psi_max = min(p["rho_o"], rho_max)
        return dict(op=tol_rho + 8. * eps * max(p["rho_o"], 1.),
                    F=(2. / 3.) * p["G_chen"] * psi_max * tol_rho + 16. * eps * p["G_chen"] * psi_max * psi_max / 3., S=0.)
    dS = (p["alpha"] / p["c_o"]) * tol_rho + 16. * eps * max(p["alpha"], 1.)
    D = max(rho_max, p["rho_o"])
    return dict(op=dS, S=p["epsilon"] * dS + 8. * eps * p["epsilon"],
                F=p["G_chen"] * (D + rho_max) * tol_rho + 16. * eps * p["G_chen"] * rho_max * D)


class RocketModel(object):
    def __init__(self, nx, ny, omega, omega_c, mode="flow", dtype=np.float32, **params):
        assert mode in ("flow", "forces")
        T = self.T = np.dtype(dtype).type
        self.nx, self.ny, self.mode = int(nx), int(ny), mode
        self.omegas = [T(np.float32(omega)), T(np.float32(omega_c))]      # (the handles' parameters are float32)
        self.w = W64.astype(T)
        self.cs = T(CS32)
        self.cs2 = self.cs * self.cs
        # `1. / (cs * cs)`: a double quotient, rounded once to the kernels' float
        self.inv_cs2 = T(1.) / self.cs2 if T is np.float64 else np.float32(1. / np.float64(self.cs2))
        self.params = dict(G=0., G_c=0., epsilon=0., rho_o=1., G_chen=0., c_o=1., alpha=1.)
        self.set_params(**params)
        z2, z3, z4 = (lambda: np.zeros((nx, ny), T)), (lambda: np.zeros((nx, ny, 2), T)), (lambda: np.zeros((nx, ny, 2, 9), T))
        self.f, self.feq, self.rho = z4(), z4(), z3()
        self.u, self.v, self.op, self.Fx, self.Fy, self.Sx, self.Sy = z2(), z2(), z2(), z2(), z2(), z2(), z2()
        self.clamped = np.zeros((nx, ny, 9), bool)      # the population links the last collision floored at 0

    def set_params(self, **kw):
        for k, v in kw.items():
            assert k in PARAMS, k
            self.params[k] = float(np.float32(v))

    def _p(self, k):
        return self.T(self.params[k])

    def set_f(self, f):
        self.f = np.array(f, dtype=self.T).reshape(self.nx, self.ny, 2, 9)

    # -- the stages ---------------------------------------------------------------------------------------------------------
    def move(self):
        new = np.empty_like(self.f)
        for k in range(9):
            new[:, :, :, k] = np.roll(self.f[:, :, :, k], (CX[k], CY[k]), axis=(0, 1))      # new[x, y] = f[x - cx, y - cy]
        self.f = new

    def update_hydro(self):
        rho = self.f[..., 0].copy()
        for k in range(1, 9):
            rho = rho + self.f[..., k]
        self.rho = rho

    @staticmethod
    def _at(a, cx, cy):
        return np.roll(a, (-cx, -cy), axis=(0, 1))          # a(x + cx, y + cy)

    def stencil(self, a, times=None):
        """sum_k (w_k c_k) a(x + c_k) [times(x)], in the order of the links"""
        sx, sy = np.zeros_like(a), np.zeros_like(a)
        for k in range(9):
            q = self._at(a, int(CX[k]), int(CY[k]))
            if times is not None:
                q = times * q
            sx = sx + (self.w[k] * self.T(CX[k])) * q
            sy = sy + (self.w[k] * self.T(CY[k])) * q
        return sx, sy

    def psi(self):
        r = np.maximum(self.rho[:, :, 0], self.T(0.))
        return (self._p("rho_o") * (self.T(1.) - np.exp(-r / self._p("rho_o")))).astype(self.T)

    def surf(self):
        r = np.maximum(self.rho[:, :, 1], self.T(0.))
        return np.power(self.T(1.) - np.exp(-r / self._p("c_o")), self._p("alpha")).astype(self.T)

    def update_velocity(self):
        if self.mode == "flow":
            gx, gy = self.stencil(self.rho[:, :, 1])
            self.u, self.v = -self._p("epsilon") * self.inv_cs2 * gx, -self._p("epsilon") * self.inv_cs2 * gy
        else:
            self.u, self.v = self.Fx + self.Sx, self.Fy + self.Sy

    def update_forces(self):
        if self.mode == "flow":
            self.op = self.psi()
            sx, sy = self.stencil(self.op, times=self.op)
            self.Fx, self.Fy = -self._p("G_chen") * sx, -self._p("G_chen") * sy
        else:
            self.op = self.surf()
            gx, gy = self.stencil(self.op)
            self.Sx, self.Sy = -self._p("epsilon") * self.inv_cs2 * gx, -self._p("epsilon") * self.inv_cs2 * gy
            rp = self.rho[:, :, 0]
            px, py = self.stencil(rp)
            px, py = px * self.inv_cs2, py * self.inv_cs2
            self.Fx, self.Fy = -self._p("G_chen") * px * (rp - self._p("rho_o")), -self._p("G_chen") * py * (rp - self._p("rho_o"))

    def update_feq(self):
        T = self.T
        for k in range(9):
            cu = T(CX[k]) * self.u + T(CY[k]) * self.v
            inner = T(1.) + cu / self.cs2
            self.feq[:, :, :, k] = (self.w[k] * self.rho) * inner[:, :, None]

    def collide(self):
        T = self.T
        rp = self.rho[:, :, 0]
        growth = self._p("G") * rp * (T(1.) - rp)
        if self.mode == "forces":
            growth = np.where(rp > T(1.), T(0.), growth)
        om, omc = self.omegas
        for k in range(9):
            new = self.f[:, :, 0, k] * (T(1.) - om) + om * self.feq[:, :, 0, k] + self.w[k] * growth
            if self.mode == "flow":
                new = new + (self.w[k] * (T(CX[k]) * self.Fx + T(CY[k]) * self.Fy)) / self.cs2
            self.clamped[:, :, k] = new < 0
            self.f[:, :, 0, k] = np.where(new < 0, T(0.), new)
            self.f[:, :, 1, k] = self.f[:, :, 1, k] * (T(1.) - omc) + omc * self.feq[:, :, 1, k] + self.w[k] * (self._p("G_c") * rp)

    @property
    def STAGES(self):
        third = ("update_velocity", "update_forces") if self.mode == "flow" else ("update_forces", "update_velocity")
        return ("move", "update_hydro") + third + ("update_feq", "collide")

    def step(self):
        for name in self.STAGES:
            getattr(self, name)()

    def run(self, n):
        for _ in range(int(n)):
            self.step()

    def get_fields(self):
        return dict(f=self.f, feq=self.feq, rho=self.rho, u=self.u, v=self.v, op=self.op, Fx=self.Fx, Fy=self.Fy, Sx=self.Sx, Sy=self.Sy)


def from_fixture(g, dtype):
    """The model set up as a fixture's header says, holding its f0."""
    m = RocketModel(int(g["nx"]), int(g["ny"]), float(g["omega"][0]), float(g["omega"][1]), mode=str(g["mode"]), dtype=dtype,
                    **dict(zip(PARAMS, [float(x) for x in g["params"]])))
    m.set_f(g["f0"])
    return m
