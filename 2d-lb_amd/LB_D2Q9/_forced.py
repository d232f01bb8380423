"""What the two families of forced-fluid drop-ins share (``porous_media.single_component`` and
``multicomponent_multiphase.multi``): a fluid that owns one engine lattice, and the runner the reference drives its fluids
through.  Internal: import the names from those modules.  What differs stays there: which fluids a family builds and the
text it refuses the others with, the engine a runner drives, the shapes of its fields (``_KEYS``), its additional forces."""
import numpy as np

from ._dropin import NUM_JUMPERS, DeviceField, Phases, cs, get_divisible_global, lattice_arrays
from .simulation import Simulation

num_type = np.float32
int_type = np.int32
w, cx, cy = lattice_arrays(num_type, int_type)


class Forced_Fluid(Phases):
    """One fluid = one lattice of the engine (``self._engine``, a ``Simulation`` of the subclass's semantics)."""

    def __init__(self, sim, field_index, nu, bc, semantics, device, seed):
        self.sim = sim
        self.field_index = int_type(field_index)
        self.lb_nu_e = num_type(nu)
        self.bc = bc
        # (the reference's float64 expression, rounded once: omega is the float32 of 1 / (0.5 + nu / cs^2))
        self.tau = num_type(.5 + float(nu) / cs ** 2)
        self.omega = num_type((.5 + float(nu) / cs ** 2) ** -1.)
        assert self.omega < 2.
        self._seed = seed
        self._sim = self._engine = Simulation(int(sim.nx), int(sim.ny), self.omega, bc=bc, semantics=semantics, device=device)

    def initialize(self, rho_arr, f_amp=0.0):
        """ASSUMES THAT THE BARYCENTRIC VELOCITY IS ALREADY SET (Simulation_Runner.set_bary_velocity)."""
        e = self._engine
        g = e.get_fields(("u", "v"))
        e.set_fields(np.asarray(rho_arr).reshape(e.nx, e.ny), g["u"], g["v"])
        self.update_feq()
        self.init_pop(amplitude=f_amp)

    def init_pop(self, amplitude=0.001, seed=None):
        """f = f_streamed = feq (1 + amplitude randn), seeded; amplitude 0 = exactly feq."""
        if amplitude == 0:
            self._engine.init_pop(None)
            return
        rng = np.random.default_rng(self._seed if seed is None else seed)
        self._engine.init_pop(1. + amplitude * rng.standard_normal((int(self.sim.nx), int(self.sim.ny), NUM_JUMPERS)))


class Forced_Runner(object):
    """Everything is in dimensionless units.  It's just easier."""

    _KEYS = {}              # field name -> rank of the array the reference's attribute of that name has

    def __init__(self, nx, ny, L_lb, T_lb, num_populations, two_d_local_size, use_interop, check_max_ulb, mach_tolerance,
                 context=None):
        self.nx, self.ny = int_type(nx), int_type(ny)
        self.L_lb, self.T_lb = int_type(L_lb), num_type(T_lb)
        self.delta_x, self.delta_t = 1. / self.L_lb, 1. / self.T_lb
        self.num_populations = int_type(num_populations)
        self.check_max_ulb, self.mach_tolerance = check_max_ulb, mach_tolerance
        self.two_d_local_size = two_d_local_size
        self.two_d_global_size = get_divisible_global((self.nx, self.ny), two_d_local_size)
        self.context, self.queue, self.kernels = context, None, None    # (OpenCL objects of the reference: kept, never used)
        self.use_interop = use_interop
        self.w, self.cx, self.cy = w, cx, cy
        self.cs = num_type(cs)
        self.num_jumpers = int_type(NUM_JUMPERS)
        self.halo = int_type(1)
        self.fluid_list, self.tau_arr = [], []
        self.additional_collisions, self.additional_forces = [], []
        self._bary = None                                   # set_bary_velocity before add_fluid: kept for the fluids to come
        self._field64 = {}                                  # fluid -> [fx, fy] float64, the sum of its radial forces
        for key in self._KEYS:
            setattr(self, key, DeviceField(self, key))

    def _adopt(self, fluid):
        self.fluid_list.append(fluid)
        if self._bary is not None:
            fluid._engine.set_bary_velocity(*self._bary)

    def complete_setup(self):
        self.tau_arr = np.array([f.tau for f in self.fluid_list], dtype=num_type)

    def set_bary_velocity(self, u_bary_host, v_bary_host):
        shape = (int(self.nx), int(self.ny))
        self._bary = (np.asarray(u_bary_host).reshape(shape), np.asarray(v_bary_host).reshape(shape))
        for f in self.fluid_list:
            f._engine.set_bary_velocity(*self._bary)

    def update_bary_velocity(self):
        self._need().update_bary_velocity()

    def _add_radial(self, fluid_index, center_x, center_y, prefactor, radial_scaling):
        """prefactor r^radial_scaling along the unit vector from (center_x, center_y), added to the fluid's radial field: formed
        and summed on the host in float64 (it depends on position only).  Returns the sum cast to float32, once."""
        x, y = np.meshgrid(np.arange(int(self.nx)), np.arange(int(self.ny)), indexing="ij")
        dx, dy = (x - int(center_x)).astype(np.float64), (y - int(center_y)).astype(np.float64)
        radius, theta = np.sqrt(dx * dx + dy * dy), np.arctan2(dy, dx)
        magnitude = float(prefactor) * np.power(radius, float(radial_scaling))
        acc = self._field64.setdefault(int(fluid_index), [np.zeros_like(dx), np.zeros_like(dx)])
        acc[0] += magnitude * np.cos(theta)
        acc[1] += magnitude * np.sin(theta)
        return acc[0].astype(num_type), acc[1].astype(num_type)

    def run(self, num_iterations, debug=False):
        """num_iterations time steps, one fused launch each."""
        self._need().run(int(num_iterations))

    def get_fields(self):
        return {k: self._read_field(k) for k in self._KEYS}
