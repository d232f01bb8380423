"""Several immiscible or partly miscible fluids, liquid-vapour separation, interface-limited eating and growth: the surface of
the reference's ``LB_D2Q9.multicomponent_multiphase.multi`` (``Simulation_Runner``, ``Fluid``) on a set of liblbhip handles
(``Simulation(..., semantics='multifluid')``, advanced together by ``LB_D2Q9.coupled.Shan_Chen_Fluids``).

Every fluid is a D2Q9 BGK lattice with its own viscosity that relaxes towards an equilibrium at the barycentric velocity of
all fluids, Guo-forced by constant and radial accelerations and by the Shan-Chen interaction forces
``G_i(x) -= G_int psi(rho_i(x)) sum_k w_k c_k psi(rho_j(x + c_k))`` (and the same with i and j exchanged).  ``run(n)`` is the
reference's loop -- move, move_bcs, update_hydro, G = 0, the additional forces, update_bary_velocity, update_feq,
collide_particles, the additional collisions -- but where the reference makes about ``6 NP + 4 + entries`` launches and as
many host waits per step, here a step is one launch and no wait (two with ``sim.engine.set_variant(0)``).  The phase methods run
one kernel each and equal it bitwise.

``num_type``: the reference computes in float64; this engine is float32 like every lattice it has, so ``num_type`` is
``np.float32`` here.  Arrays are ``(nx, ny, NP[, 9])`` F-ordered; ``u_bary``, ``v_bary`` are ``(nx, ny)``.

Differences.  The additional forces act in a fixed order -- each fluid's constant accelerations (summed), its radial ones
(summed on the host in float64, cast once), then the interaction forces in the order they were added -- whatever the order
of the ``add_*`` calls; an interaction force's ``bc`` must be the fluids' own.  Strings are compared with ``==`` (the
reference's ``is 'periodic'`` only works for interned literals).  ``init_pop`` takes a ``seed``; the OpenCL-only arguments are
accepted and ignored.  A cell whose total density is 0 gets a NaN barycentric velocity, as in the reference.

NOT BUILT -- each raises ``NotImplementedError`` naming this list: ``potential='vdw'``;
``add_interaction_force_second_belt`` (halo 2); ``add_screened_poisson_force`` (FFT); ``Simulation_RunnerD2Q25``; more than
3 fluids; fluids of different families in one set.
"""
import numpy as np

from .._dropin import NUM_JUMPERS, DeviceField, cs, get_divisible_global, lattice_arrays  # noqa: F401
from .._forced import Forced_Fluid, Forced_Runner, cx, cy, int_type, num_type, w  # noqa: F401
from ..coupled import Shan_Chen_Fluids
from ..simulation import Simulation  # noqa: F401

_NOT_BUILT = ("not built in LB_D2Q9.multicomponent_multiphase.multi: potential='vdw'; add_interaction_force_second_belt "
              "(halo 2); add_screened_poisson_force (FFT); Simulation_RunnerD2Q25; more than 3 fluids; fluids of different "
              "families in one set")
MAX_FLUIDS = Shan_Chen_Fluids.MAX_POPULATIONS


class Fluid(Forced_Fluid):
    def __init__(self, sim, field_index, nu=1.0, bc='periodic', device=0, seed=None):
        if bc not in ('periodic', 'zero_gradient'):
            raise ValueError('unknown bc...')
        if not 0 <= int(field_index) < MAX_FLUIDS:
            raise NotImplementedError(_NOT_BUILT)
        Forced_Fluid.__init__(self, sim, field_index, nu, bc, "multifluid", device, seed)

    def update_forces(self):
        """For internal forces...none in this case."""


class Simulation_Runner(Forced_Runner):
    """Everything is in dimensionless units.  It's just easier."""

    _KEYS = {"rho": 3, "u": 3, "v": 3, "Gx": 3, "Gy": 3, "f": 4, "feq": 4, "u_bary": 2, "v_bary": 2}

    def __init__(self, nx=100, ny=100, L_lb=100, T_lb=1., num_populations=1, two_d_local_size=(32, 32), use_interop=False,
                 check_max_ulb=False, mach_tolerance=0.1, context=None):
        if not 1 <= int(num_populations) <= MAX_FLUIDS:
            raise NotImplementedError(_NOT_BUILT)
        Forced_Runner.__init__(self, nx, ny, L_lb, T_lb, num_populations, two_d_local_size, use_interop, check_max_ulb, mach_tolerance,
                               context)
        self._set = None
        self._g = {}                                        # fluid -> [gx, gy], the sum of its constant accelerations
        self._inter, self._react = [], []
        self._dirty = False                                 # the tables differ from what the set's first handle holds

    @property
    def engine(self):
        """The ``Shan_Chen_Fluids`` underneath (checkpoints, hot_kernel ...); None before add_fluid."""
        return self._set

    def _need(self):
        if self._set is None:
            raise RuntimeError("add_fluid() first: the fluids carry the lattices")
        if self._dirty:
            self._set.set_interactions(self._inter)
            self._set.set_reactions(self._react)
            self._dirty = False
        return self._set

    def _fluid(self, index):
        index = int(index)
        if not 0 <= index < len(self.fluid_list):
            raise IndexError("fluid %d of %d: add_fluid() it first" % (index, len(self.fluid_list)))
        return self.fluid_list[index]

    def _read_field(self, key):
        return self._need().get_fields((key,))[key]

    def add_fluid(self, fluid):
        if len(self.fluid_list) >= min(MAX_FLUIDS, int(self.num_populations)):
            raise NotImplementedError(_NOT_BUILT) if len(self.fluid_list) >= MAX_FLUIDS else ValueError("num_populations fluids are there already")
        if self.fluid_list and fluid.bc != self.fluid_list[0].bc:
            raise NotImplementedError(_NOT_BUILT)
        if int(fluid.field_index) != len(self.fluid_list):
            raise ValueError("fluids are added in the order of their field_index")
        self._adopt(fluid)
        self._set = Shan_Chen_Fluids.of([f._engine for f in self.fluid_list])
        self._dirty = True

    def update_forces(self):
        """Gx, Gy = 0 and the additional forces: one kernel."""
        self._need().update_forces()

    # -- additional forces ------------------------------------------------------------------------------------------------
    def add_constant_g_force(self, fluid_index, force_x, force_y):
        f = self._fluid(fluid_index)
        g = self._g.setdefault(int(fluid_index), [num_type(0.), num_type(0.)])
        g[0], g[1] = num_type(g[0] + num_type(force_x)), num_type(g[1] + num_type(force_y))
        self.additional_forces.append(["add_constant_g_force", [int(fluid_index), force_x, force_y]])
        f._engine.set_body_force(*g)

    def add_radial_g_force(self, fluid_index, center_x, center_y, prefactor, radial_scaling):
        """prefactor r^radial_scaling along the unit vector from (center_x, center_y): multi.cl:568-606, formed on the host in
        float64 (it depends on position only) and cast to float32 once; the kernel multiplies by rho."""
        f = self._fluid(fluid_index)
        field = self._add_radial(fluid_index, center_x, center_y, prefactor, radial_scaling)
        self.additional_forces.append(["add_radial_g_force", [int(fluid_index), center_x, center_y, prefactor, radial_scaling]])
        f._engine.set_force_field(*field)

    def add_interaction_force(self, fluid_1_index, fluid_2_index, G_int, bc='periodic', potential='linear', potential_parameters=None):
        f1, f2 = self._fluid(fluid_1_index), self._fluid(fluid_2_index)
        if bc not in ('periodic', 'zero_gradient'):
            raise ValueError('Specified boundary condition does not exist')
        if potential == 'vdw':
            raise NotImplementedError(_NOT_BUILT)
        if potential not in Shan_Chen_Fluids.POTENTIALS:
            raise ValueError('Specified pseudopotential does not exist.')
        if bc != f1.bc or bc != f2.bc:
            raise ValueError("the stencil's bc (%r) must be the fluids' (%r): the engine has one boundary rule per set" % (bc, f1.bc))
        par = 0. if potential_parameters is None else float(np.atleast_1d(potential_parameters)[0])
        if potential == 'shan_chen' and par == 0.:
            raise ValueError("potential='shan_chen' needs potential_parameters=[rho_0], rho_0 != 0")
        if len(self._inter) >= 6:
            raise ValueError("the interaction table holds 6 entries")
        self._inter.append((int(fluid_1_index), int(fluid_2_index), num_type(G_int), potential, num_type(par)))
        self.additional_forces.append(["add_interaction_force", [int(fluid_1_index), int(fluid_2_index), G_int, bc, potential, potential_parameters]])
        self._dirty = True

    def add_interaction_force_second_belt(self, *args, **kwargs):
        raise NotImplementedError(_NOT_BUILT)

    def add_screened_poisson_force(self, *args, **kwargs):
        raise NotImplementedError(_NOT_BUILT)

    # -- additional collisions --------------------------------------------------------------------------------------------
    def _add_reaction(self, row):
        if len(self._react) >= 4:
            raise ValueError("the reaction table holds 4 entries")
        self._react.append(row)
        self.additional_collisions.append(list(row))
        self._dirty = True

    def add_eating_rate(self, eater_index, eatee_index, rate, orderparameter_cutoff):
        """Eater eats eatee at a given rate, where |rho_eater - rho_eatee| / (rho_eater + rho_eatee) < orderparameter_cutoff."""
        self._fluid(eater_index), self._fluid(eatee_index)
        self._add_reaction(("eat", int(eater_index), int(eatee_index), num_type(rate), num_type(orderparameter_cutoff)))

    def add_growth(self, eater_index, min_rho_cutoff, max_rho_cutoff, eat_rate):
        """Grows uniformly wherever min_rho_cutoff < rho < max_rho_cutoff."""
        self._fluid(eater_index)
        self._add_reaction(("grow", int(eater_index), num_type(min_rho_cutoff), num_type(max_rho_cutoff), num_type(eat_rate)))

    def react(self):
        """The additional collisions, from the stored rho."""
        self._need().react()

    def check_fields(self):
        g = self.get_fields()
        for i in range(len(self.fluid_list)):
            print('Field:', i)
            for k in ("rho", "u", "v", "Gx", "Gy"):
                print(k, 'sum', np.sum(g[k][:, :, i]), 'nonfinite', int(np.sum(~np.isfinite(g[k][:, :, i]))))


class Simulation_RunnerD2Q25(Simulation_Runner):
    def __init__(self, **kwargs):
        raise NotImplementedError(_NOT_BUILT)
