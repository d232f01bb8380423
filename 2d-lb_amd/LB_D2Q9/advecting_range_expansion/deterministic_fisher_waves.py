"""Deterministic range expansions: the surface of the reference's
``LB_D2Q9.advecting_range_expansion.deterministic_fisher_waves.Fisher_Expansion`` on coupled scalar lattices
(``LB_D2Q9.coupled.Coupled_Scalars``, bc='box').

``num_populations`` strains, inoculated side by side in a strip along the wall y = 0, diffuse (each with its own
diffusivity, hence its own omega), are advected by a uniform imposed velocity and grow logistically into the room all of
them together leave: field i gains ``w_k G_i rho_i (1 - sum_j rho_j)``.  The box is closed: on-node bounce-back on four
walls.  ``run(n)`` is fused HIP, one launch per step for all strains; the phase methods run one kernel each.

The parameter arithmetic lives in a plain function (``fisher_expansion_parameters``) that needs no handle.  Two repairs
against the reference: ``np.float`` no longer exists; the velocity ratio vc / vf is taken as 0 when
vc = 0 (the reference divides 0 by 0 there and carries NaN into u, v).
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, DropIn, cs, get_divisible_global, lattice_arrays  # noqa: F401
from ..coupled import Coupled_Scalars

w, cx, cy = lattice_arrays(np.float32, np.int32)


def fisher_expansion_parameters(Lx=1.0, Ly=1.0, vx=0., vy=0., vc=0., mu_standard=1.0, mu_list=None, D_standard=1.0,
                                D_list=None, time_prefactor=1., N=50):
    """L = 2 sqrt(D_standard / mu_standard), T = 1 / mu_standard, vf = L / T; delta_x = 1 / N, delta_t = time_prefactor
    delta_x^2; per strain G = (mu / mu_standard) delta_t, lattice diffusivity D / (4 D_standard) delta_t / delta_x^2, omega
    = 1 / (1/2 + 3 lb_D); the uniform velocity in lattice units is (delta_t / delta_x) (vc / vf) (vx, vy) / vc."""
    mu, D = np.array(mu_list, dtype=np.float64), np.array(D_list, dtype=np.float64)
    p = dict(L=2 * np.sqrt(D_standard / mu_standard), T=1. / mu_standard)
    p["vf"] = p["L"] / p["T"]
    p["N"], p["delta_x"] = N, 1. / N
    p["delta_t"] = time_prefactor * p["delta_x"] ** 2
    p["ulb"] = p["delta_t"] / p["delta_x"]
    p["dim_vel_ratio"] = vc / p["vf"]
    p["dim_G"] = mu / mu_standard
    p["lb_G"] = (p["dim_G"] * p["delta_t"]).astype(np.float32)
    p["dim_D_population"] = (1. / (4. * D_standard)) * D
    p["lb_D_population"] = (p["dim_D_population"] * (p["delta_t"] / p["delta_x"] ** 2)).astype(np.float32)
    p["omega"] = ((.5 + p["lb_D_population"] / cs ** 2) ** -1.).astype(np.float32)
    p["lx"], p["ly"] = N * int(Lx / p["L"]), N * int(Ly / p["L"])
    p["nx"], p["ny"] = p["lx"] + 2, p["ly"] + 2
    scale = p["ulb"] * (p["dim_vel_ratio"] / vc if vc != 0 else 0.)
    p["lb_vx"], p["lb_vy"] = scale * vx, scale * vy
    return p


def inoculation_stripes(nx, ny, num_populations, widths, indices, depth):
    """rho (nx, ny, num_populations): strain indices[j] at density 1 over the next int(widths[j] nx) columns of the strip
    0 <= y < depth; the last stripe takes whatever columns are left."""
    rho = np.zeros((nx, ny, num_populations), dtype=np.float32, order='F')
    occupied = 0
    for j, (width, strain) in enumerate(zip(widths, indices)):
        n = nx - occupied if j == len(widths) - 1 else int(width * nx)
        rho[occupied:occupied + n, 0:depth, strain] = 1.0
        occupied += n
    return rho


class Fisher_Expansion(DropIn):
    verbose = True
    _sim = property(lambda self: self.sim)      # the engine under the name the shared methods use

    def __init__(self, Lx=1.0, Ly=1.0, vx=0., vy=0., vc=0., mu_standard=1.0, mu_list=None, D_standard=1.0, D_list=None,
                 initial_frac_widths=None, initial_frac_indices=None, time_prefactor=1., N=50, rho_amp=1.0,
                 concentration_amp=1.0, two_d_local_size=(32, 32), three_d_local_size=(32, 32, 1), use_interop=False,
                 device=0):
        self.phys_Lx, self.phys_Ly = Lx, Ly
        self.phys_D_list, self.D_standard = np.array(D_list, dtype=np.float64), D_standard
        self.phys_vx, self.phys_vy, self.phys_vc = vx, vy, vc
        self.phys_mu_standard, self.phys_mu_list = mu_standard, np.array(mu_list, dtype=np.float64)
        self.num_populations = np.int32(len(self.phys_mu_list))
        self.rho_amp, self.concentration_amp = rho_amp, concentration_amp
        self.initial_frac_widths, self.initial_frac_indices = initial_frac_widths, initial_frac_indices
        self.use_interop = use_interop              # (OpenCL-only arguments: accepted, unused)
        self.time_prefactor = time_prefactor

        p = fisher_expansion_parameters(Lx, Ly, vx, vy, vc, mu_standard, mu_list, D_standard, D_list, time_prefactor, N)
        self._lb_v = (p["lb_vx"], p["lb_vy"])
        for k in ("L", "T", "vf", "N", "delta_x", "delta_t", "ulb", "dim_vel_ratio", "dim_G", "lb_G", "dim_D_population",
                  "lb_D_population", "omega", "lx", "ly", "nx", "ny"):
            setattr(self, k, p[k])
        self._say('Characteristic L:', self.L)
        self._say('Characteristic T:', self.T)
        self._say('Fisher wave velocity:', self.vf)
        self._say('u_lb:', self.ulb)
        self._say('lb_G:', self.lb_G)
        self._say('omega populations:', self.omega)

        self.two_d_local_size, self.three_d_local_size = two_d_local_size, three_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.three_d_global_size = get_divisible_global((self.nx, self.ny, 9), three_d_local_size)

        self.sim = Coupled_Scalars(self.nx, self.ny, self.omega, self.lb_G, bc="box", device=device)
        self.rho, self.u, self.v = DeviceField(self, "rho"), DeviceField(self, "u"), DeviceField(self, "v")
        self.f, self.feq = DeviceField(self, "f"), DeviceField(self, "feq")

        self.x_center = self.y_center = self.X_dim = self.Y_dim = None
        self.init_hydro()
        self.update_feq()
        self.init_f()

    def init_hydro(self, initial_fisher_widths=2):
        nx, ny = self.nx, self.ny
        self.x_center, self.y_center = nx // 2, ny // 2
        X, Y = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
        self.X_dim = (X.astype(np.float64) - self.x_center) / self.N
        self.Y_dim = (Y.astype(np.float64) - self.y_center) / self.N
        rho = inoculation_stripes(nx, ny, int(self.num_populations), self.initial_frac_widths, self.initial_frac_indices,
                                  int(self.N * initial_fisher_widths))
        u = np.asfortranarray((self._lb_v[0] * np.ones((nx, ny))).astype(np.float32))
        v = np.asfortranarray((self._lb_v[1] * np.ones((nx, ny))).astype(np.float32))
        self.sim.set_fields(rho, u, v)

    def init_f(self, amplitude=0.00, seed=None):
        """f = feq (1 + amplitude randn) on every strain.  (The reference draws the noise unseeded.)"""
        perturb = None
        if amplitude != 0:
            rng = np.random.default_rng(seed)
            perturb = 1. + amplitude * rng.standard_normal((self.nx, self.ny, int(self.num_populations), NUM_JUMPERS))
        self.sim.init_pop(perturb)
        # The engine starts the never-streamed corner links from f itself (f_streamed = f, the other classes' convention); the
        # reference's f_temporary starts as zeros and nothing ever writes those eight links of it, so its corners read zeros.
        self.sim.set_corner_state(np.zeros((int(self.num_populations), 8), np.float32))
