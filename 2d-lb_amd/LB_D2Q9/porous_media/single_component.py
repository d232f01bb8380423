"""Forced flow of one fluid in a porous medium: the surface of the reference's ``LB_D2Q9.porous_media.single_component``
(``Simulation_Runner``, ``Pourous_Media`` -- the reference's spelling) on a porous handle of liblbhip
(``Simulation(..., semantics='porous', bc='periodic' | 'zero_gradient')``).

A D2Q9 BGK fluid with Guo forcing, a porosity ``epsilon`` in the equilibrium and in the forcing term, a linear drag
``-epsilon nu_fluid u / K``, a quadratic one ``-epsilon Fe |u| u / sqrt(K)``, and constant or radial body forces, in a
periodic or a zero-gradient box.  ``run(n)`` is the reference's loop -- move, move_bcs, update_hydro, G = 0, the additional
forces, update_forces, update_bary_velocity, update_feq, collide_particles -- but where the reference makes eleven launches
and eleven host waits per step, here a step is one fused launch.  The phase methods run one kernel each and are bitwise
equal to it.

``num_type``: the reference computes in float64; this engine is float32 like every lattice it has, so ``num_type`` is
``np.float32`` here.  Arrays are ``(nx, ny, 1[, 9])`` F-ordered, as in the reference with one population.

Not built: several fluids (``num_populations > 1``), the Shan-Chen interaction forces (``add_interaction_force``,
``add_interaction_force_second_belt``) and ``add_eating_rate``: they raise ``NotImplementedError`` here
(``LB_D2Q9.multicomponent_multiphase.multi`` has them, without the porous medium).  Differences:
``Pourous_Media.update_forces`` is the reference's ``Gx, Gy = 0`` + additional forces + ``update_forces_pourous`` in one
kernel (the reference's kernel alone, applied twice, would scale the force by ``epsilon`` twice); ``initialize`` runs it
with no additional force, which is what the reference's buffers hold at that point; ``init_pop`` takes a ``seed``; the
OpenCL-only arguments are accepted and ignored.  A cell with ``rho = 0`` gets a NaN barycentric velocity, as in the
reference.
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, cs, get_divisible_global, lattice_arrays  # noqa: F401
from ..simulation import Simulation

num_type = np.float32
int_type = np.int32
w, cx, cy = lattice_arrays(num_type, int_type)

_UNBUILT = "only one fluid is built: several fluids and Shan-Chen interaction forces are not (LB_D2Q9.porous_media.single_component)"


class Pourous_Media(object):
    def __init__(self, sim, field_index, nu_e=1.0, epsilon=1.0, nu_fluid=1.0, K=1.0, Fe=1.0, bc='periodic', device=0, seed=None):
        if int(field_index) != 0:
            raise NotImplementedError(_UNBUILT)
        if bc not in ('periodic', 'zero_gradient'):
            raise ValueError('unknown bc...')
        self.sim = sim
        self.field_index = int_type(field_index)
        self.lb_nu_e = num_type(nu_e)
        self.epsilon, self.nu_fluid, self.K, self.Fe = num_type(epsilon), num_type(nu_fluid), num_type(K), num_type(Fe)
        self.bc = bc
        # (the reference's float64 expression, rounded once: omega is the float32 of 1 / (0.5 + nu_e / cs^2))
        self.tau = num_type(.5 + float(nu_e) / cs ** 2)
        self.omega = num_type((.5 + float(nu_e) / cs ** 2) ** -1.)
        assert self.omega < 2.
        self._seed = seed
        self._engine = Simulation(int(sim.nx), int(sim.ny), self.omega, bc=bc, semantics="porous", device=device)
        self._engine.set_porous(self.epsilon, self.nu_fluid, self.K, self.Fe)

    def initialize(self, rho_arr, f_amp=0.0):
        """ASSUMES THAT THE BARYCENTRIC VELOCITY IS ALREADY SET (Simulation_Runner.set_bary_velocity)."""
        e = self._engine
        g = e.get_fields(("u", "v"))
        e.set_fields(np.asarray(rho_arr).reshape(e.nx, e.ny), g["u"], g["v"])
        self.update_feq()
        self.init_pop(amplitude=f_amp)
        self.update_hydro()
        # the reference's force buffers hold no additional force here: they are added inside run()
        force, field = e.body_force, e._force_field
        e.set_body_force(0., 0.)
        e.set_force_field(None, None)
        self.update_forces()
        e.set_body_force(*force)
        if field is not None:
            e.set_force_field(*field)

    def init_pop(self, amplitude=0.001, seed=None):
        """f = f_streamed = feq (1 + amplitude randn), seeded; amplitude 0 = exactly feq."""
        if amplitude == 0:
            self._engine.init_pop(None)
            return
        rng = np.random.default_rng(self._seed if seed is None else seed)
        self._engine.init_pop(1. + amplitude * rng.standard_normal((int(self.sim.nx), int(self.sim.ny), NUM_JUMPERS)))

    def update_forces(self):
        self._engine.update_forces()

    def update_feq(self):
        self._engine.update_feq()

    def move_bcs(self):
        self._engine.move_bcs()

    def move(self):
        self._engine.move()

    def update_hydro(self):
        self._engine.update_hydro()

    def collide_particles(self):
        self._engine.collide_particles()


class Simulation_Runner(object):
    """Everything is in dimensionless units.  It's just easier."""

    _KEYS = {"rho": 2, "u": 2, "v": 2, "u_bary": 2, "v_bary": 2, "Gx": 2, "Gy": 2, "f": 3, "feq": 3}

    def __init__(self, nx=100, ny=100, L_lb=100, T_lb=1., num_populations=1, two_d_local_size=(32, 32), use_interop=False,
                 check_max_ulb=False, mach_tolerance=0.1):
        if int(num_populations) != 1:
            raise NotImplementedError(_UNBUILT)
        self.nx, self.ny = int_type(nx), int_type(ny)
        self.L_lb, self.T_lb = int_type(L_lb), num_type(T_lb)
        self.delta_x, self.delta_t = 1. / self.L_lb, 1. / self.T_lb
        self.num_populations = int_type(num_populations)
        self.check_max_ulb, self.mach_tolerance = check_max_ulb, mach_tolerance
        self.two_d_local_size = two_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.context = self.queue = self.kernels = None     # (OpenCL objects of the reference: kept, never used)
        self.use_interop = use_interop
        self.w, self.cx, self.cy = w, cx, cy
        self.cs = num_type(cs)
        self.num_jumpers = int_type(NUM_JUMPERS)
        self.halo = int_type(1)
        self.fluid_list, self.tau_arr = [], []
        self.additional_collisions, self.additional_forces = [], []
        self._engine = None
        self._bary = None                                   # set_bary_velocity before add_fluid: kept until there is an engine
        self._force = [num_type(0.), num_type(0.)]
        self._field64 = None
        for key in self._KEYS:
            setattr(self, key, DeviceField(self, key))

    @property
    def engine(self):
        """The ``Simulation`` underneath (set_f, checkpoints, hot_kernel ...); None before add_fluid."""
        return self._engine

    def _need_engine(self):
        if self._engine is None:
            raise RuntimeError("add_fluid() first: the fluid carries the lattice")
        return self._engine

    def _read_field(self, key):
        a = self._need_engine().get_fields((key,))[key]
        return a[:, :, None] if self._KEYS[key] == 2 else a[:, :, None, :]

    def add_fluid(self, fluid):
        if self.fluid_list:
            raise NotImplementedError(_UNBUILT)
        self.fluid_list.append(fluid)
        self._engine = fluid._engine
        if self._bary is not None:
            self._engine.set_bary_velocity(*self._bary)

    def complete_setup(self):
        self.tau_arr = np.array([f.tau for f in self.fluid_list], dtype=num_type)

    def set_bary_velocity(self, u_bary_host, v_bary_host):
        shape = (int(self.nx), int(self.ny))
        self._bary = (np.asarray(u_bary_host).reshape(shape), np.asarray(v_bary_host).reshape(shape))
        if self._engine is not None:
            self._engine.set_bary_velocity(*self._bary)

    def update_bary_velocity(self):
        self._need_engine().update_bary_velocity()

    def add_constant_body_force(self, fluid_index, force_x, force_y):
        if int(fluid_index) != 0:
            raise NotImplementedError(_UNBUILT)
        self._force = [num_type(self._force[0] + num_type(force_x)), num_type(self._force[1] + num_type(force_y))]
        self.additional_forces.append(["add_constant_body_force", [int(fluid_index), force_x, force_y]])
        self._need_engine().set_body_force(*self._force)

    def add_radial_body_force(self, fluid_index, center_x, center_y, prefactor, radial_scaling):
        """prefactor r^radial_scaling along the unit vector from (center_x, center_y): single_component.cl:571-607, formed on
        the host in float64 (it depends on position only) and cast to float32 once."""
        if int(fluid_index) != 0:
            raise NotImplementedError(_UNBUILT)
        x, y = np.meshgrid(np.arange(int(self.nx)), np.arange(int(self.ny)), indexing="ij")
        dx, dy = (x - int(center_x)).astype(np.float64), (y - int(center_y)).astype(np.float64)
        radius, theta = np.sqrt(dx * dx + dy * dy), np.arctan2(dy, dx)
        magnitude = float(prefactor) * np.power(radius, float(radial_scaling))
        if self._field64 is None:
            self._field64 = [np.zeros_like(dx), np.zeros_like(dx)]
        self._field64[0] += magnitude * np.cos(theta)
        self._field64[1] += magnitude * np.sin(theta)
        self.additional_forces.append(["add_radial_body_force", [int(fluid_index), center_x, center_y, prefactor, radial_scaling]])
        self._need_engine().set_force_field(self._field64[0].astype(num_type), self._field64[1].astype(num_type))

    def add_eating_rate(self, eater_index, eatee_index, rate):
        raise NotImplementedError(_UNBUILT)

    def add_interaction_force(self, *args, **kwargs):
        raise NotImplementedError(_UNBUILT)

    def add_interaction_force_second_belt(self, *args, **kwargs):
        raise NotImplementedError(_UNBUILT)

    def run(self, num_iterations, debug=False):
        """num_iterations time steps, one fused launch each."""
        self._need_engine().run(int(num_iterations))

    def get_fields(self):
        return {k: self._read_field(k) for k in self._KEYS}
