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
from .._forced import Forced_Fluid, Forced_Runner, cx, cy, int_type, num_type, w  # noqa: F401
from ..simulation import Simulation  # noqa: F401

_UNBUILT = "only one fluid is built: several fluids and Shan-Chen interaction forces are not (LB_D2Q9.porous_media.single_component)"


class Pourous_Media(Forced_Fluid):
    def __init__(self, sim, field_index, nu_e=1.0, epsilon=1.0, nu_fluid=1.0, K=1.0, Fe=1.0, bc='periodic', device=0, seed=None):
        if int(field_index) != 0:
            raise NotImplementedError(_UNBUILT)
        if bc not in ('periodic', 'zero_gradient'):
            raise ValueError('unknown bc...')
        self.epsilon, self.nu_fluid, self.K, self.Fe = num_type(epsilon), num_type(nu_fluid), num_type(K), num_type(Fe)
        Forced_Fluid.__init__(self, sim, field_index, nu_e, bc, "porous", device, seed)
        self._engine.set_porous(self.epsilon, self.nu_fluid, self.K, self.Fe)

    def initialize(self, rho_arr, f_amp=0.0):
        """ASSUMES THAT THE BARYCENTRIC VELOCITY IS ALREADY SET (Simulation_Runner.set_bary_velocity)."""
        Forced_Fluid.initialize(self, rho_arr, f_amp)
        self.update_hydro()
        # the reference's force buffers hold no additional force here: they are added inside run()
        e = self._engine
        force, field = e.body_force, e._force_field
        e.set_body_force(0., 0.)
        e.set_force_field(None, None)
        self.update_forces()
        e.set_body_force(*force)
        if field is not None:
            e.set_force_field(*field)

    def update_forces(self):
        self._engine.update_forces()


class Simulation_Runner(Forced_Runner):
    """Everything is in dimensionless units.  It's just easier."""

    _KEYS = {"rho": 2, "u": 2, "v": 2, "u_bary": 2, "v_bary": 2, "Gx": 2, "Gy": 2, "f": 3, "feq": 3}

    def __init__(self, nx=100, ny=100, L_lb=100, T_lb=1., num_populations=1, two_d_local_size=(32, 32), use_interop=False,
                 check_max_ulb=False, mach_tolerance=0.1):
        if int(num_populations) != 1:
            raise NotImplementedError(_UNBUILT)
        Forced_Runner.__init__(self, nx, ny, L_lb, T_lb, num_populations, two_d_local_size, use_interop, check_max_ulb, mach_tolerance)
        self._engine = None
        self._force = [num_type(0.), num_type(0.)]

    @property
    def engine(self):
        """The ``Simulation`` underneath (set_f, checkpoints, hot_kernel ...); None before add_fluid."""
        return self._engine

    def _need(self):
        if self._engine is None:
            raise RuntimeError("add_fluid() first: the fluid carries the lattice")
        return self._engine

    def _read_field(self, key):
        a = self._need().get_fields((key,))[key]
        return a[:, :, None] if self._KEYS[key] == 2 else a[:, :, None, :]

    def add_fluid(self, fluid):
        if self.fluid_list:
            raise NotImplementedError(_UNBUILT)
        self._engine = fluid._engine
        self._adopt(fluid)

    def add_constant_body_force(self, fluid_index, force_x, force_y):
        if int(fluid_index) != 0:
            raise NotImplementedError(_UNBUILT)
        self._force = [num_type(self._force[0] + num_type(force_x)), num_type(self._force[1] + num_type(force_y))]
        self.additional_forces.append(["add_constant_body_force", [int(fluid_index), force_x, force_y]])
        self._need().set_body_force(*self._force)

    def add_radial_body_force(self, fluid_index, center_x, center_y, prefactor, radial_scaling):
        """prefactor r^radial_scaling along the unit vector from (center_x, center_y): single_component.cl:571-607, formed on
        the host in float64 (it depends on position only) and cast to float32 once."""
        if int(fluid_index) != 0:
            raise NotImplementedError(_UNBUILT)
        field = self._add_radial(fluid_index, center_x, center_y, prefactor, radial_scaling)
        self.additional_forces.append(["add_radial_body_force", [int(fluid_index), center_x, center_y, prefactor, radial_scaling]])
        self._need().set_force_field(*field)

    def add_eating_rate(self, eater_index, eatee_index, rate):
        raise NotImplementedError(_UNBUILT)

    def add_interaction_force(self, *args, **kwargs):
        raise NotImplementedError(_UNBUILT)

    def add_interaction_force_second_belt(self, *args, **kwargs):
        raise NotImplementedError(_UNBUILT)
