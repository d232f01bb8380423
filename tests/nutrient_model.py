"""A numpy model of a population and its nutrient under a spectral velocity, in pull form, float32 or float64 (test infrastructure;
not a test module).

What LB_D2Q9/reaction_diffusion/surfactant_nutrient_waves.cl computes per iteration of Surfactant_Nutrient_Wave.run /
Clumpy_Surfactant_Nutrient_Wave.run, written for whole arrays, one method per stage.  Two scalar lattices in a periodic box: index 0
the population p (omega), index 1 the nutrient n (omega_n).  With cs = float32(1 / sqrt(3)) and cs^2 = cs cs as the kernels form it:
  move              both lattices, pull-stream with wrap
  update_hydro      rho_i = sum_k f_ik, k = 0 ... 8
  update_velocity   (u, v) = scale Re grad phi, (1 - lam^2 laplace) phi = rho_p           (spectral_model.solve, complex64 / complex128)
  update_forces     clumpy: psi = rho_o (1 - exp(-max(rho_p, 0) / rho_o)); F = -cs cs G_chen sum_k w_k c_k psi(x) psi(x + c_k)
  update_feq        feq_ik = w_k rho_i (1 + c_k.u / cs^2)
  collide           population: f_k (1 - omega) + omega feq_k + w_k G rho_p rho_n [clumpy: + (w_k c_k.F) / cs^2];
                    nutrient: f_k (1 - omega_n) + omega_n feq_k - w_k G rho_p rho_n.  No floor at zero.
It is the yardstick where no fixture reaches; against the fixtures recorded from the reference's C (tests/golden/sn_*.npz) it is
checked by tests/test_nutrient_cpu.py.  The stream and the contract are scalar_model's, the solve is spectral_model's.

Arrays: (nx, ny, 2) / (nx, ny, 2, 9) of `dtype`; u, v, psi, Fx, Fy (nx, ny).  Every scalar is a `dtype` and every operation one
operation in it.
"""
import numpy as np

from scalar_model import CX, CY, contract_tol  # noqa: F401  (contract_tol: for the users of this module)
from spectral_model import solve

F32 = np.float32
W64 = np.array([4. / 9.] + [1. / 9.] * 4 + [1. / 36.] * 4)
CS32 = np.float32(1. / np.sqrt(3))
PARAMS = ("G", "scale", "rho_o", "G_chen", "lam")
EPS32 = 2. ** -24


def nutrient_bounds(params, rho_max, tol_rho, eps=EPS32):
    """The bounds on psi and F that follow from a population density known to tol_rho (rho_max bounds it), rho_o > 0.

      psi = rho_o (1 - exp(-max(rho, 0) / rho_o)):  d psi / d rho = exp(-rho / rho_o) in (0, 1], so psi is known to tol_rho, and
            0 <= psi <= psi_max = min(rho_o, rho_max) (1 - exp(-x) <= min(1, x)); its own float32 rounding -- a quotient, expf, a
            difference and a product, a few ulp of a value <= max(rho_o, 1) -- is 8 eps max(rho_o, 1).
      F = -cs^2 G_chen psi(x) sum_k w_k c_k psi(x + c_k), cs^2 = 1/3: the nine-point sum over a quantity known to d is known to
            (sum_k w_k |c_kx|) d = d / 3 and is at most psi_max / 3, so
            dF <= (1/3) |G_chen| (d psi  psi_max / 3 + psi_max  d psi / 3) = (2 / 9) |G_chen| psi_max tol_psi,
            plus the float32 rounding of the terms themselves: some ten operations on a value <= |G_chen| psi_max^2 / 9, 16 eps of it."""
    rho_o, G_chen = abs(float(params["rho_o"])), abs(float(params["G_chen"]))
    psi_max = min(rho_o, rho_max)
    tol_psi = tol_rho + 8. * eps * max(rho_o, 1.)
    return dict(psi=tol_psi, F=(2. / 9.) * G_chen * psi_max * tol_psi + 16. * eps * G_chen * psi_max * psi_max / 9.)


class NutrientModel(object):
    def __init__(self, nx, ny, omega, omega_n, clumpy=False, dtype=np.float32, **params):
        T = self.T = np.dtype(dtype).type
        self.nx, self.ny, self.clumpy = int(nx), int(ny), bool(clumpy)
        self.omegas = [T(F32(omega)), T(F32(omega_n))]      # (the handles' parameters are float32)
        self.ctype = np.complex64 if T is np.float32 else np.complex128
        self.w = W64.astype(T)
        self.cs = T(CS32)
        self.cs2 = self.cs * self.cs
        self.params = dict(G=0., scale=0., rho_o=1., G_chen=0., lam=1.)
        self.set_params(**params)
        z2, z3, z4 = (lambda: np.zeros((nx, ny), T)), (lambda: np.zeros((nx, ny, 2), T)), (lambda: np.zeros((nx, ny, 2, 9), T))
        self.f, self.feq, self.rho = z4(), z4(), z3()
        self.u, self.v, self.psi, self.Fx, self.Fy = z2(), z2(), z2(), z2(), z2()

    def set_params(self, **kw):
        for k, v in kw.items():
            assert k in PARAMS, k
            self.params[k] = float(v) if k == "lam" else float(np.float32(v))

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

    def update_velocity(self):
        _, xg, yg = solve(self.rho[:, :, 0], self.params["lam"], self.ctype)
        self.u = (self._p("scale") * xg.real).astype(self.T)
        self.v = (self._p("scale") * yg.real).astype(self.T)

    def update_forces(self):
        if not self.clumpy:
            return
        T = self.T
        r = np.maximum(self.rho[:, :, 0], T(0.))
        self.psi = (self._p("rho_o") * (T(1.) - np.exp(-r / self._p("rho_o")))).astype(T)
        sx, sy = np.zeros_like(self.psi), np.zeros_like(self.psi)
        for k in range(9):
            mult = self.psi * np.roll(self.psi, (-int(CX[k]), -int(CY[k])), axis=(0, 1))    # psi(x) psi(x + c_k)
            sx = sx + (self.w[k] * T(CX[k])) * mult
            sy = sy + (self.w[k] * T(CY[k])) * mult
        k = -self.cs * self.cs * self._p("G_chen")
        self.Fx, self.Fy = k * sx, k * sy

    def update_feq(self):
        T = self.T
        for k in range(9):
            cu = T(CX[k]) * self.u + T(CY[k]) * self.v
            inner = T(1.) + cu / self.cs2
            self.feq[:, :, :, k] = (self.w[k] * self.rho) * inner[:, :, None]

    def collide(self):
        T = self.T
        growth = self._p("G") * self.rho[:, :, 0] * self.rho[:, :, 1]
        om, omn = self.omegas
        for k in range(9):
            new = self.f[:, :, 0, k] * (T(1.) - om) + om * self.feq[:, :, 0, k] + self.w[k] * growth
            if self.clumpy:
                new = new + (self.w[k] * (T(CX[k]) * self.Fx + T(CY[k]) * self.Fy)) / self.cs2
            self.f[:, :, 0, k] = new
            self.f[:, :, 1, k] = self.f[:, :, 1, k] * (T(1.) - omn) + omn * self.feq[:, :, 1, k] + (-self.w[k]) * growth

    STAGES = ("move", "update_hydro", "update_velocity", "update_forces", "update_feq", "collide")

    def step(self):
        for name in self.STAGES:
            getattr(self, name)()

    def run(self, n):
        for _ in range(int(n)):
            self.step()

    def redo_initial_condition(self, rho):
        """The drop-in's: the velocity (and the force) of rho, feq, f = feq."""
        self.rho = np.array(rho, dtype=self.T).reshape(self.nx, self.ny, 2)
        self.update_velocity()
        self.update_forces()
        self.update_feq()
        self.f = self.feq.copy()

    def state(self):
        d = dict(f=self.f, rho=self.rho, u=self.u, v=self.v)
        if self.clumpy:
            d.update(psi=self.psi, Fx=self.Fx, Fy=self.Fy)
        return d


def lattice_parameters(Lx, Ly, N, vc=1., Dn=1. / 4., time_prefactor=1.):
    """What the fixtures' header records: the arithmetic of surfactant_nutrient_parameters, restated (the package's is tested against
    hand values and against this)."""
    f64 = np.float64
    cs2 = f64(CS32) ** 2
    delta_x = 1. / N
    delta_t = time_prefactor * delta_x ** 2
    ratio = delta_t / delta_x ** 2
    omega = F32((.5 + f64(F32(.25 * ratio)) / cs2) ** -1.)
    omega_n = F32((.5 + f64(F32(Dn * ratio)) / cs2) ** -1.)
    return dict(nx=int(np.round(N * Lx)), ny=int(np.round(N * Ly)), omega=omega, omega_n=omega_n, lb_G=F32(1. * delta_t),
                scale=F32(-vc * (delta_t / delta_x)), delta_x=delta_x, delta_t=delta_t)


def from_fixture(g, dtype, tag=""):
    """The model set up as a fixture's header says, holding its f0 (tag: 'plain_' / 'clumpy_' in the phase file)."""
    m = NutrientModel(int(g["nx"]), int(g["ny"]), float(g["omega"][0]), float(g["omega"][1]), clumpy=bool(g[tag + "clumpy"]), dtype=dtype,
                      **dict(zip(PARAMS, [float(x) for x in g[tag + "params"]])))
    m.set_f(g["f0"])
    return m
