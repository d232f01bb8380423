"""Stochastic range expansions on a nutrient: the surface of the reference's
``LB_D2Q9.advecting_range_expansion.stochastic_nutrients.Expansion`` on noisy strains that share a nutrient lattice
(``LB_D2Q9.expansion_set.Expansion_Set``).

``num_populations`` strains (one to three), inoculated well mixed in a strip along the edge y = 0, diffuse (each with its own
diffusivity, hence its own omega), are advected by a uniform imposed velocity, grow on the nutrient ahead of them and deplete it, and
fluctuate: strain i gains ``w_k (G_i rho_i c + sqrt(Dg_i rho_i c) z + (Dg_i c / 4)(z^2 - 1))`` per step, with ``c`` the nutrient and ``z``
a standard normal per cell, strain and step; densities below ``zero_cutoff`` count as 0.  The box is the reference's open one (``bc=
'open'``: nothing enters from outside) or periodic.  ``run(n)`` is fused HIP, one launch per step for all strains and the nutrient, the
normals drawn inside the kernel; the phase methods run one kernel each.

The parameter arithmetic lives in a plain function (``expansion_parameters``) that needs no handle.  Repairs against the reference
(INTEGRATION.md): ``np.float`` no longer exists; ``nx / 2`` is an integer division; the velocity ratio vc / vf gives velocity zero when
vc = 0 (the reference divides 0 by 0 there); ``D_list=None`` raises a clear error; the prints are dropped; the reference's unseeded
generator is the engine's seeded stream (``seed``; strain i draws under ``seed + i``), whose first collision draws at noise counter 0 as
the reference's first fill.
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, DropIn, get_divisible_global, lattice_arrays  # noqa: F401
from ..expansion_set import Expansion_Set

w, cx, cy = lattice_arrays(np.float32, np.int32)
cs = np.float32(1. / np.sqrt(3))        # stochastic_nutrients.py:27

MAX_STRAINS = Expansion_Set.MAX_STRAINS


def expansion_parameters(Lx=1.0, Ly=1.0, vx=0., vy=0., vc=0., mu_standard=1.0, mu_list=None, D_standard=1.0, D_list=None, Nb=10.,
                         Dc=1.0, time_prefactor=1., N=50):
    """set_characteristic_length_time, set_field_constants and initialize_grid_dims of the reference: L = 2 sqrt(D_standard /
    mu_standard), T = 1 / mu_standard, vf = L / T; delta_x = 1 / N, delta_t = time_prefactor delta_x^2; per strain G = (mu /
    mu_standard) delta_t, Dg = (mu / Nb) / (4 D_standard) delta_t, lattice diffusivity D / (4 D_standard) delta_t / delta_x^2 and omega =
    1 / (1/2 + lb_D / cs^2) in float32 with the float32 cs; the nutrient's omega from Dc likewise, in float64 over the float32 cs^2 and
    rounded once; the uniform velocity in lattice units is (delta_t / delta_x) (vc / vf) (vx, vy) / vc."""
    if mu_list is None:
        raise ValueError("mu_list is required: one growth rate per strain")
    if D_list is None:
        raise ValueError("D_list is required: one diffusivity per strain (the reference fails later, on None arithmetic)")
    mu, D = np.atleast_1d(np.array(mu_list, dtype=np.float64)), np.atleast_1d(np.array(D_list, dtype=np.float64))
    if len(mu) != len(D):
        raise ValueError("mu_list and D_list must have one entry per strain each")
    if len(mu) > MAX_STRAINS:
        raise ValueError("%d strains: at most %d strains on one nutrient are built" % (len(mu), MAX_STRAINS))
    p = dict(L=2 * np.sqrt(D_standard / mu_standard), T=1. / mu_standard)
    p["vf"] = p["L"] / p["T"]
    p["N"], p["delta_x"] = N, 1. / N
    p["delta_t"] = time_prefactor * p["delta_x"] ** 2
    p["ulb"] = p["delta_t"] / p["delta_x"]
    p["dim_vel_ratio"] = vc / p["vf"]
    p["dim_G"] = mu / mu_standard
    p["lb_G"] = (p["dim_G"] * p["delta_t"]).astype(np.float32)
    p["dim_Dg"] = (mu / Nb) * (1. / (4 * D_standard))
    p["lb_Dg"] = (p["dim_Dg"] * p["delta_t"]).astype(np.float32)
    p["dim_D_population"] = (1. / (4. * D_standard)) * D
    p["lb_D_population"] = (p["dim_D_population"] * (p["delta_t"] / p["delta_x"] ** 2)).astype(np.float32)
    p["omega"] = ((.5 + p["lb_D_population"] / cs ** 2) ** -1.).astype(np.float32)        # float32 throughout: cs ** 2 is one
    p["dim_D_nutrient"] = Dc / (4 * D_standard)
    p["lb_D_nutrient"] = p["dim_D_nutrient"] * (p["delta_t"] / p["delta_x"] ** 2)
    p["omega_nutrient"] = np.float32((.5 + p["lb_D_nutrient"] / float(cs ** 2)) ** -1.)
    p["lx"], p["ly"] = np.int32(N * int(Lx / p["L"])), np.int32(N * int(Ly / p["L"]))
    p["nx"], p["ny"] = np.int32(p["lx"] + 2), np.int32(p["ly"] + 2)
    scale = p["ulb"] * (p["dim_vel_ratio"] / vc if vc != 0 else 0.)
    p["lb_vx"], p["lb_vy"] = scale * vx, scale * vy
    return p


def inoculum(nx, ny, num_populations, depth, rho_amp, concentration_amp):
    """rho (nx, ny, num_populations + 1) of init_hydro: every strain at rho_amp / num_populations in the rows y < depth and 0 ahead, the
    nutrient (last) at concentration_amp everywhere."""
    rho = np.zeros((nx, ny, num_populations + 1), dtype=np.float32, order='F')
    rho[:, :, 0:num_populations] = rho_amp / num_populations
    rho[:, depth:, 0:num_populations] = 0
    rho[:, :, num_populations] = concentration_amp
    return rho


class Expansion(DropIn):
    verbose = False                     # (the reference's prints are dropped)
    _sim = property(lambda self: self.sim)      # the engine under the name the shared methods use

    def __init__(self, Lx=1.0, Ly=1.0, z=0.1, vx=0., vy=0., vc=0., mu_standard=1.0, mu_list=None, D_standard=1.0, D_list=None,
                 Nb=10., Dc=1.0, time_prefactor=1., N=50, rho_amp=1.0, concentration_amp=1.0, zero_cutoff=0.01,
                 two_d_local_size=(32, 32), three_d_local_size=(32, 32, 1), use_interop=False, seed=0, bc="open", device=0):
        p = expansion_parameters(Lx, Ly, vx, vy, vc, mu_standard, mu_list, D_standard, D_list, Nb, Dc, time_prefactor, N)
        self.phys_Lx, self.phys_Ly, self.phys_z = Lx, Ly, z
        self.phys_D_list, self.D_standard = np.array(D_list, dtype=np.float64), D_standard
        self.phys_vx, self.phys_vy, self.phys_vc = vx, vy, vc
        self.phys_Nb, self.phys_Dc = Nb, Dc
        self.phys_mu_standard, self.phys_mu_list = mu_standard, np.array(mu_list, dtype=np.float64)
        self.num_populations = np.int32(len(np.atleast_1d(self.phys_mu_list)))
        self.rho_amp, self.concentration_amp = rho_amp, concentration_amp
        self.zero_cutoff = np.float32(zero_cutoff)
        self.use_interop = use_interop              # (OpenCL-only arguments: accepted, unused)
        self.time_prefactor, self.seed, self.bc = time_prefactor, int(seed), bc
        self._lb_v = (p["lb_vx"], p["lb_vy"])
        for k in ("L", "T", "vf", "N", "delta_x", "delta_t", "ulb", "dim_vel_ratio", "dim_G", "lb_G", "dim_Dg", "lb_Dg", "dim_D_population",
                  "lb_D_population", "omega", "dim_D_nutrient", "lb_D_nutrient", "omega_nutrient", "lx", "ly", "nx", "ny"):
            setattr(self, k, p[k])

        self.two_d_local_size, self.three_d_local_size = two_d_local_size, three_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.three_d_global_size = get_divisible_global((self.nx, self.ny, 9), three_d_local_size)

        self.sim = Expansion_Set(self.nx, self.ny, self.omega, self.omega_nutrient, self.lb_G, bc=bc, zero_cutoff=self.zero_cutoff,
                                 device=device)
        self.sim.set_noise(self.lb_Dg, self.seed)
        self.rho, self.u, self.v = DeviceField(self, "rho"), DeviceField(self, "u"), DeviceField(self, "v")
        self.f, self.feq = DeviceField(self, "f"), DeviceField(self, "feq")

        self.x_center = self.y_center = self.X_dim = self.Y_dim = None
        self.init_hydro()
        self.update_feq()
        self.init_f()

    def init_hydro(self):
        nx, ny = int(self.nx), int(self.ny)
        self.x_center, self.y_center = nx // 2, ny // 2
        X, Y = np.meshgrid(np.arange(nx), np.arange(ny))
        self.X_dim = (X.astype(np.float64) - self.x_center) / self.N
        self.Y_dim = (Y.astype(np.float64) - self.y_center) / self.N
        rho = inoculum(nx, ny, int(self.num_populations), 2 * int(self.N), self.rho_amp, self.concentration_amp)
        u = np.asfortranarray((self._lb_v[0] * np.ones((nx, ny))).astype(np.float32))
        v = np.asfortranarray((self._lb_v[1] * np.ones((nx, ny))).astype(np.float32))
        self.sim.set_fields(rho, u, v)

    def init_f(self, amplitude=0.00, seed=None):
        """f = feq (1 + amplitude randn) on every strain and the nutrient.  (The reference draws this perturbation unseeded.)"""
        perturb = None
        if amplitude != 0:
            rng = np.random.default_rng(seed)
            perturb = 1. + amplitude * rng.standard_normal((int(self.nx), int(self.ny), int(self.num_populations) + 1, NUM_JUMPERS))
        self.sim.init_pop(perturb)
        # The engine starts the links that enter from outside the box from f itself (f_streamed = f, the other classes' convention);
        # the reference's f_temporary starts as zeros and its push `move` never writes those links: they read zeros.
        self.sim.set_edge_state(np.zeros_like(self.sim.get_edge_state()))

    def noise(self):
        """[(Dg, seed, t)] per strain: t = the noise counter, the number of noisy collisions since the start."""
        return self.sim.noise()
