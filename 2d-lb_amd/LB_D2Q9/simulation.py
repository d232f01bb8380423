"""Generic D2Q9 BGK lattice on one MI355X (or one row slab of a multi-GPU run).

``Simulation`` owns a ``liblbhip`` handle and mirrors the method surface of the reference's
``LB_D2Q9.dimensionless.opencl_dim.Pipe_Flow`` (opencl_dim.py:295-438): ``move``, ``move_bcs``,
``update_hydro``, ``update_feq``, ``collide_particles``, ``run(n)``, ``get_fields()``, plus
``step()`` == ``run(1)``.  It takes lattice parameters directly (nx, ny, omega, boundary family);
the physical-units constructors live in ``LB_D2Q9.dimensionless.hip_dim``.

Host arrays use the reference's conventions: F-ordered float32 ``(nx, ny)`` / ``(nx, ny, 9)``
(opencl_dim.py:165, 279, 390-415); for a row slab ``ny`` is the slab height.
"""
import ctypes as ct
import os

import numpy as np

from . import _native
from ._native import LbError, check
from .kinds import KINDS

NUM_JUMPERS = 9


def _f_order(a, shape, dtype=np.float32):
    a = np.asarray(a)
    if a.shape != shape:
        raise ValueError("expected shape %s, got %s" % (shape, a.shape))
    return np.asfortranarray(a.astype(dtype, copy=False))


def _address(buf):
    if isinstance(buf, np.ndarray):
        assert buf.dtype == np.float32 and buf.flags.c_contiguous
        return buf.ctypes.data
    return int(buf)


def run_group(sims, num_iterations, wait=True):
    """Advance slab handles that tile one grid on one device in lock step (lb_run_group)."""
    arr = (ct.c_void_p * len(sims))(*[s._h for s in sims])
    check(_native.lib().lb_run_group(arr, len(sims), int(num_iterations)))
    if wait:
        for s in sims:
            s.sync()


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 creates it, the caller broadcasts it)."""
    uid = (ct.c_char * 128)()
    check(_native.lib().lb_comm_unique_id(uid))
    return bytes(uid.raw)


class Simulation(object):
    def __init__(self, nx, ny, omega, bc="pipe", inlet_rho=1., outlet_rho=1., lid_u=0., rho0=1.,
                 obstacle_mask=None, device=0, y0=0, local_ny=None, halo=False, semantics="opencl",
                 inlet_u=0., outlet_u=None, planar=None, eager_macro=False):
        """
        :param nx, ny: global grid size (cells, boundary nodes included).
        :param omega: BGK relaxation rate, 0 < omega < 2.
        :param bc: 'pipe' (the reference's pressure inlet/outlet + no-slip walls, D2Q9.cl:173-261),
                   'periodic' or 'cavity' (lid-driven; build-defined, see oracle/d2q9_oracle.c).
        :param inlet_u, outlet_u: bc='velocity_inlet' (D2Q9.cl:263-374; un-fused kernels): imposed speed at
               x=0 / x=nx-1 (outlet_u defaults to inlet_u, as OLD/opencl.py:283-286 sets u_e = u_w).
        :param obstacle_mask: optional (nx, ny) array, non-zero = solid (bounce-back, D2Q9.cl:398-433).
        :param device: HIP device ordinal; -1 (LB_DEVICE_CPU) = the product's own CPU backend: semantics='cython', bc='pipe',
               whole grid, single thread, the reference's mixed float32 / float64 arithmetic (include/lb_hip.h).  Chosen by
               this value only: a GPU handle never falls back to the host.
        :param y0, local_ny: the row slab this object owns (multi-GPU); default = whole grid.
        :param halo: fill the ghost rows through the halo interface even for a whole-grid handle.
        :param semantics: 'opencl' (D2Q9.cl, fused fast path), 'cython' (cython_dim.pyx: pipe family, whole grid,
               compatibility path; the two reference paths differ at walls and inlets) or 'd2q9i' (the reference's
               D2Q9i.cl fork of the OpenCL path: pipe family, whole grid, fused).
               'diffusion': a SCALAR lattice (the reference's D2Q9_diffusion.cl / reaction_diffusion/diffusion.py): rho is a
               concentration, u, v an imposed velocity field (set_fields, set_velocity_from) that no kernel writes, the
               equilibrium is linear, set_reaction(G) adds Fisher growth; bc='periodic' or 'open' (the reference's box:
               links entering from outside keep the values of the last set_f / init_pop, get_edge_state); whole grid.
               'multifield': one field of a set of COUPLED scalar lattices (the reference's D2Q9_multifield_fisher.cl): as
               'diffusion', but the growth term is G rho (1 - sum of the set's rho) and bc is 'periodic' or 'box' (on-node
               bounce-back on four walls; get_corner_state).  LB_D2Q9.coupled.Coupled_Scalars advances a set in lock step;
               run() on one member is the set of one.
               'poisson': the LB Poisson solver (the reference's D2Q9_poisson.cl / poisson/solver.py): bc='dirichlet' (a value
               prescribed on the four walls, set_poisson), a source field (set_source), solve(max_iterations) with the
               reference's stopping rule decided on the device, gradient(); whole grid.  run(n) = n iterations, no check.
               'porous': forced flow in a porous medium (the reference's porous_media/single_component.cl / .py with one
               fluid): a Guo-forced BGK fluid with porosity, linear and quadratic drag (set_porous) and body forces
               (set_body_force, set_force_field); bc='periodic' or 'zero_gradient'; whole grid, no obstacles.  float32 like
               every lattice here (the reference's fork is float64).  get_fields adds 'u_bary', 'v_bary', 'Gx', 'Gy'.
               'multifluid': one fluid of a set of Shan-Chen fluids (the reference's multicomponent_multiphase/multi.cl /
               multi.py): a Guo-forced BGK fluid relaxing towards the barycentric velocity of the set, with body forces
               (set_body_force, set_force_field: accelerations, multiplied by rho), pseudopotential interaction forces
               (set_interactions) and reactions (set_reactions); bc='periodic' or 'zero_gradient'; whole grid, at least 3x3, no
               obstacles.  One launch per step (set_variant(0): two).  A handle on its own is a set of one; LB_D2Q9.coupled.Shan_Chen_Fluids advances several.
               get_fields keys are those of 'porous'.
               'rocket': one of the two lattices of a surfactant-propelled colony (the reference's rocket_yeast/rocket_yeast.cl and
               rocket_yeast_forces_only.cl): a scalar lattice with the linear equilibrium whose velocity the set computes from the
               surfactant; bc='periodic', whole grid, at least 3x3.  It advances only as a set of two:
               LB_D2Q9.coupled.Surfactant_Colony (run() and collide_particles() on the member itself are refused).
        :param planar: device layout of the lattices: False = the nine planes of a row stored together (default),
               True = each plane contiguous (LB_FLAG_PLANAR); results are identical.  None: environment variable
               LB_LAYOUT=planar selects True (tuning aid).
        :param eager_macro: the last launch of every run() stores rho, u, v itself (LB_FLAG_EAGER_MACRO).  Default: the
               plain families leave them to be rebuilt from the populations -- whose moments they are, BGK relaxation
               conserving both -- the first time get_fields / update_feq / ... needs them (include/lb_hip.h).
        """
        if isinstance(bc, str):
            if bc not in _native.BC_NAMES:
                raise ValueError("bc must be one of %s" % sorted(_native.BC_NAMES))
            bc = _native.BC_NAMES[bc]
        self.nx, self.ny = int(nx), int(ny)
        self.y0 = int(y0)
        self.local_ny = self.ny if local_ny is None else int(local_ny)
        self.omega = omega
        self.bc_mode = bc
        self.inlet_rho, self.outlet_rho = inlet_rho, outlet_rho
        self.lid_u, self.rho0 = lid_u, rho0
        self.device = int(device)
        self._lib = _native.lib()            # raises if liblbhip.so is missing: no CPU fallback
        p = _native.LbParams()
        p.nx, p.ny, p.y0, p.local_ny = self.nx, self.ny, self.y0, self.local_ny
        p.bc_mode, p.device = bc, self.device
        if planar is None:
            planar = os.environ.get("LB_LAYOUT", "") == "planar"
        self.planar = bool(planar)
        self.eager_macro = bool(eager_macro)
        p.flags = ((_native.LB_FLAG_HALO if halo else 0) | (_native.LB_FLAG_PLANAR if self.planar else 0) |
                   (_native.LB_FLAG_EAGER_MACRO if self.eager_macro else 0))
        if semantics not in KINDS:
            raise ValueError("semantics must be one of %s" % sorted(KINDS))
        self.semantics, self._kind = semantics, KINDS[semantics]        # (the kind's row: LB_D2Q9/kinds.py)
        p.semantics = self._kind.sem
        self._halo = bool(halo)
        p.omega = np.float32(omega)
        p.inlet_rho, p.outlet_rho = np.float32(inlet_rho), np.float32(outlet_rho)
        p.lid_u, p.rho0 = np.float32(lid_u), np.float32(rho0)
        self.inlet_u, self.outlet_u = inlet_u, (inlet_u if outlet_u is None else outlet_u)
        p.inlet_u, p.outlet_u = np.float32(self.inlet_u), np.float32(self.outlet_u)
        self._h = ct.c_void_p()
        check(self._lib.lb_create(ct.byref(p), ct.byref(self._h)))
        if self.device == _native.LB_DEVICE_CPU:
            # the CPU backend keeps the reference's float64 scalars (lb_params carries float32: include/lb_hip.h)
            check(self._lib.lb_set_params_f64(self._h, float(omega), float(inlet_rho), float(outlet_rho)))
        self._shape2 = (self.nx, self.local_ny)
        self._shape3 = (self.nx, self.local_ny, NUM_JUMPERS)
        self.G = 0.                      # scalar lattices: growth rate of the Fisher term (set_reaction)
        self.rho_on_boundary, self.react_factor, self.tolerance = 0., 1., 1e-6      # the Poisson solver's (set_poisson)
        self.epsilon, self.nu_fluid, self.K, self.Fe = 1., 0., 1., 0.               # the porous medium's (set_porous)
        self.body_force = (0., 0.)                                                  # ... and its constant force (set_body_force)
        self._force_field = None                                                    # ... and its force field, as uploaded
        self.interactions, self.reactions = [], []                                  # a set of fluids' tables, kept by its first handle (set_interactions, set_reactions)
        self._mask_host = None
        self._mask_halo_host = None      # (south_rows, north_rows) as last given to set_obstacle_mask_halo
        if obstacle_mask is not None:
            self.set_obstacle_mask(obstacle_mask)

    # -- lifetime ----------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.lb_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._lib.lb_sync(self._h))

    # -- state -------------------------------------------------------------
    def set_obstacle_mask(self, mask):
        """(nx, local_ny) array; cells equal to 1/True are solid.  None removes the obstacle."""
        if mask is None:
            check(self._lib.lb_set_mask(self._h, None))
            self._mask_host = None
            return
        m = _f_order(np.asarray(mask) != 0, self._shape2, np.int32)
        self._mask_host = m
        check(self._lib.lb_set_mask(self._h, m.ctypes.data))
        if self._halo and self.local_ny == self.ny and self.bc_mode == _native.LB_BC_PERIODIC:
            # a whole periodic grid run through the halo path is its own neighbour
            rows = np.arange(self.MASK_HALO_ROWS)
            self.set_obstacle_mask_halo(m[:, (rows - self.MASK_HALO_ROWS) % self.ny].T, m[:, rows % self.ny].T)

    def set_fields(self, rho, u, v):
        """Upload the macroscopic fields (what init_hydro does, opencl_dim.py:291-293)."""
        r, uu, vv = (_f_order(a, self._shape2) for a in (rho, u, v))
        check(self._lib.lb_set_macro(self._h, r.ctypes.data, uu.ctypes.data, vv.ctypes.data))

    def set_f(self, f):
        """Upload the populations, (nx, local_ny, 9); also fills the streaming buffer."""
        ff = _f_order(f, self._shape3)
        check(self._lib.lb_set_f(self._h, ff.ctypes.data))

    def init_pop(self, perturb=None):
        """f = f_streamed = feq * perturb (opencl_dim.py:308-327); perturb None = exactly feq."""
        if perturb is None:
            check(self._lib.lb_init_pop(self._h))
            self.sync()
        else:
            f = self.get_fields(("feq",))["feq"]
            f *= np.asarray(perturb)
            self.set_f(f)

    def init_equilibrium(self, rho, u, v, perturb=None):
        """rho,u,v -> feq -> f = feq * perturb (the construction sequence of opencl_dim.py:163-178)."""
        self.set_fields(rho, u, v)
        self.update_feq()
        self.init_pop(perturb)

    # -- the reference's phases, one kernel each (slow path, API parity) -----
    def move(self):
        check(self._lib.lb_move(self._h))
        self.sync()

    def move_bcs(self):
        check(self._lib.lb_move_bcs(self._h))
        self.sync()

    def update_hydro(self):
        check(self._lib.lb_update_hydro(self._h))
        self.sync()

    def update_feq(self):
        check(self._lib.lb_update_feq(self._h))
        self.sync()

    def collide_particles(self):
        check(self._lib.lb_collide_particles(self._h))
        self.sync()

    def zero_velocity_in_obstacle(self):
        check(self._lib.lb_zero_velocity_in_obstacle(self._h))
        self.sync()

    # -- the hot path --------------------------------------------------------
    def run(self, num_iterations, wait=True):
        """num_iterations fused time steps.  The reference returns with the work complete (it waits after
        every kernel); pass wait=False to only enqueue (never blocks the host).  A blocking run of at least four
        times the tuning pass (4 x 361 + 7 = 1451 steps; 4 x 889 + 7 on grids <= 768^2) first times the candidate kernel
        configurations on its own first steps (lb_autotune_quick: they are bitwise equivalent, the trajectory is
        unchanged; the pass advances at most (n - 7) // 4 steps, a runner-up's longer comparison included) and keeps the
        fastest for this grid; shorter runs use the size heuristic (or call autotune())."""
        n = int(num_iterations)
        if wait and n > 0 and self._kind.tunes:
            # (the pass costs 361 steps, 889 on grids <= 768^2, some of them in configurations several times slower than
            #  the best: it only pays for itself in a run several times that long)
            used = self._lib.lb_autotune_quick(self._h, (n - 7) // 4)
            if used < 0:
                check(used)
            n -= used
        check(self._lib.lb_run(self._h, n))
        if wait:
            self.sync()

    def step(self):
        self.run(1)

    # -- health -----------------------------------------------------------------
    MACH_TOLERANCE = 0.1        # the forks' default `mach_tolerance` (porous_media/single_component.py:254)

    def check(self, across_ranks=False, warn=False, raise_nonfinite=False):
        """One device pass over the populations (lb_check): {'n_nonfinite': cells whose density or velocity is not
        finite, 'max_mach': max |u| / c_s, 'sum_rho': total mass of the finite cells}.  The reference's forks have the
        two halves of this as `check_max_ulb` (a warning when max |u| > c_s * mach_tolerance,
        porous_media/single_component.py:221-225) and `check_fields()` (:753-766); `warn=True` issues that warning,
        `raise_nonfinite=True` raises FloatingPointError when the run has diverged.  across_ranks: combined over the
        ranks of the communicator (collective)."""
        n, m, r = ct.c_int64(), ct.c_float(), ct.c_double()
        check(self._lib.lb_check(self._h, int(bool(across_ranks)), ct.byref(n), ct.byref(m), ct.byref(r)))
        out = {"n_nonfinite": n.value, "max_mach": m.value, "sum_rho": r.value}
        if raise_nonfinite and n.value:
            raise FloatingPointError("lattice has %d non-finite cell(s): the run has diverged" % n.value)
        if warn and m.value > self.MACH_TOLERANCE:
            import warnings
            warnings.warn("max_ulb is greater than cs/10! Ma= %g" % m.value, RuntimeWarning, stacklevel=2)
        return out

    def timer_start(self):
        """Record the start HIP event on the engine's stream."""
        check(self._lib.lb_timer_start(self._h))

    def timer_stop(self):
        """Record the stop event, wait for it, return the milliseconds since timer_start()."""
        ms = ct.c_float()
        check(self._lib.lb_timer_stop(self._h, ct.byref(ms)))
        return ms.value

    def timed_run(self, num_iterations):
        """run() bracketed by HIP events on the engine's stream; returns milliseconds."""
        self.timer_start()
        check(self._lib.lb_run(self._h, int(num_iterations)))
        return self.timer_stop()

    # -- read-back -------------------------------------------------------------
    def get_fields(self, which=("f", "feq", "u", "v", "rho")):
        """Dictionary of host copies, same keys/shapes/orders as opencl_dim.py:390-415."""
        out = {}
        if "f" in which:
            out["f"] = np.zeros(self._shape3, np.float32, order="F")
            check(self._lib.lb_get_f(self._h, out["f"].ctypes.data))
        if "feq" in which:
            out["feq"] = np.zeros(self._shape3, np.float32, order="F")
            check(self._lib.lb_get_feq(self._h, out["feq"].ctypes.data))
        macro = [k for k in ("rho", "u", "v") if k in which]
        if macro:
            for k in macro:
                out[k] = np.zeros(self._shape2, np.float32, order="F")
            ptr = lambda k: out[k].ctypes.data if k in out else None
            check(self._lib.lb_get_macro(self._h, ptr("rho"), ptr("u"), ptr("v")))
        for a, b, get in (("u_bary", "v_bary", "lb_get_bary_velocity"), ("Gx", "Gy", "lb_get_force")):
            if a in which or b in which:            # (semantics='porous' only: the library refuses elsewhere)
                for k in (a, b):
                    if k in which:
                        out[k] = np.zeros(self._shape2, np.float32, order="F")
                ptr = lambda k: out[k].ctypes.data if k in out else None
                check(getattr(self._lib, get)(self._h, ptr(a), ptr(b)))
        return out

    # -- state I/O (the reference has none: state only leaves through get_fields) --------------
    CHECKPOINT_VERSION = 2
    _CKPT_SCALARS = ("nx", "ny", "y0", "local_ny", "bc_mode", "omega", "inlet_rho", "outlet_rho", "lid_u", "rho0",
                     "inlet_u", "outlet_u")

    @staticmethod
    def _ckpt_path(path):
        """np.savez appends '.npz' to a bare path; np.load does not: use one spelling for both."""
        path = str(path)
        return path if path.endswith(".npz") else path + ".npz"

    def checkpoint_arrays(self):
        """Everything needed to continue this run bit for bit, as a dict of arrays: populations, the macroscopic
        fields of the last step, the obstacle mask, every lattice parameter of the handle (boundary family,
        semantics, imposed speeds, halo flag) and a format version."""
        g = self.get_fields(("f", "rho", "u", "v"))
        d = dict(f=g["f"], rho=g["rho"], u=g["u"], v=g["v"],
                 mask=(self._mask_host if self._mask_host is not None else np.zeros((0, 0), np.int32)),
                 version=self.CHECKPOINT_VERSION, semantics=np.array(self.semantics), halo=int(self._halo))
        for k in self._CKPT_SCALARS:
            d[k] = getattr(self, k)
        if self.bc_mode == _native.LB_BC_VELOCITY_INLET:
            d["corner_state"] = self.get_corner_state()
        self._kind.save(self, d)
        if self._mask_halo_host is not None:         # a slab: the neighbours' obstacle rows it was given
            empty = np.zeros((0, 0), np.int32)
            d["mask_halo_south"] = empty if self._mask_halo_host[0] is None else self._mask_halo_host[0]
            d["mask_halo_north"] = empty if self._mask_halo_host[1] is None else self._mask_halo_host[1]
        return d

    def save_checkpoint(self, path):
        """Write checkpoint_arrays() to `path` (.npz appended when missing)."""
        np.savez(self._ckpt_path(path), **self.checkpoint_arrays())

    def _check_compatible(self, d):
        if int(d["version"]) != self.CHECKPOINT_VERSION:
            raise ValueError("checkpoint format %d, this build reads %d" % (int(d["version"]), self.CHECKPOINT_VERSION))
        if (int(d["nx"]), int(d["ny"]), int(d["y0"]), int(d["local_ny"])) != (self.nx, self.ny, self.y0, self.local_ny):
            raise ValueError("checkpoint is for a %dx%d lattice (slab %d+%d), this one is %dx%d (slab %d+%d)"
                             % (int(d["nx"]), int(d["ny"]), int(d["y0"]), int(d["local_ny"]),
                                self.nx, self.ny, self.y0, self.local_ny))
        if int(d["bc_mode"]) != self.bc_mode:
            raise ValueError("checkpoint was written with a different boundary family")
        if str(d["semantics"]) != self.semantics:
            raise ValueError("checkpoint was written with semantics=%r, this lattice has %r" % (str(d["semantics"]), self.semantics))
        for k in ("omega", "inlet_rho", "outlet_rho", "lid_u", "rho0", "inlet_u", "outlet_u"):
            if np.float32(d[k]) != np.float32(getattr(self, k)):
                raise ValueError("checkpoint has %s = %r, this lattice %r" % (k, float(d[k]), getattr(self, k)))

    def load_checkpoint(self, path):
        """Restore a state written by save_checkpoint into this lattice; every parameter must match
        (a different omega or boundary family would silently change the physics)."""
        with np.load(self._ckpt_path(path)) as d:
            self.restore_arrays(d)

    def restore_arrays(self, d):
        self._check_compatible(d)
        if self._kind.has_mask:
            self.set_obstacle_mask(d["mask"] if d["mask"].size else None)
        if "mask_halo_south" in d:
            so, no = d["mask_halo_south"], d["mask_halo_north"]
            self.set_obstacle_mask_halo(so if so.size else None, no if no.size else None)
        self.set_fields(d["rho"], d["u"], d["v"])
        self.set_f(d["f"])
        if self.bc_mode == _native.LB_BC_VELOCITY_INLET:
            self.set_corner_state(d["corner_state"])           # (after set_f, which resets them to f's own corners)
        self._kind.restore(self, d)                            # (after set_f, likewise: edge and corner state)

    def _set_force(self, gx, gy):
        """The force of the last step, two (nx, ny) arrays (a checkpoint's; update_forces and run() overwrite it)."""
        a, b = (_f_order(x, self._shape2) for x in (gx, gy))
        check(self._lib.lb_set_force(self._h, a.ctypes.data, b.ctypes.data))

    def _set_solve_state(self, iterations, stop_word):
        check(self._lib.lb_set_solve_state(self._h, int(iterations), int(stop_word)))

    # -- one fluid of a set of Shan-Chen fluids (semantics='multifluid'); the calls below this block are shared -------------
    def _set_tables(self, handles, count, interactions, reactions):
        """Validate and store both tables with this handle, the first of `handles` (a ctypes array of `count` handles)."""
        if interactions is not None:
            rows = [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), float(np.float32(r[4])), float(np.float32(r[5]))) for r in interactions]
            arr = (_native.Interaction * max(1, len(rows)))(*[_native.Interaction(*r) for r in rows])
            check(self._lib.lb_set_interactions(handles, count, arr, len(rows)))
            self.interactions = rows
        if reactions is not None:
            rows = [(int(r[0]), int(r[1]), int(r[2]), float(np.float32(r[3])), float(np.float32(r[4])), float(np.float32(r[5]))) for r in reactions]
            arr = (_native.FluidReaction * max(1, len(rows)))(*[_native.FluidReaction(*r) for r in rows])
            check(self._lib.lb_set_reactions(handles, count, arr, len(rows)))
            self.reactions = rows

    def _own_set(self):
        return (ct.c_void_p * 1)(self._h)

    def set_interactions(self, table):
        """The interaction table of this fluid as a set of one (self terms only): rows (fluid_1, fluid_2, potential, boundary,
        G_int, parameter) -- potential 0 linear, 1 shan_chen, 2 pow; boundary 0 periodic, 1 zero gradient = this handle's family."""
        self._set_tables(self._own_set(), 1, table, None)

    def set_reactions(self, table):
        """The reaction table of this fluid as a set of one: rows (kind, fluid_a, fluid_b, p0, p1, p2) -- kind 1 (grow): fluid,
        -, min, max, rate; kind 0 (eat) needs two fluids."""
        self._set_tables(self._own_set(), 1, None, table)

    def react(self):
        """The reaction table on the populations, from the stored rho (the reference's additional collisions)."""
        check(self._lib.lb_react_fluids(self._own_set(), 1))
        self.sync()

    # -- forced flow in a porous medium (semantics='porous') -------------------------
    def set_porous(self, epsilon=1., nu_fluid=0., K=1., Fe=0.):
        """Porosity, the fluid's viscosity in the linear drag -epsilon nu_fluid u / K, the permeability K and the factor of the
        quadratic drag -epsilon Fe |u| u / sqrt(K) (lb_set_porous); float32, like omega."""
        vals = [float(np.float32(x)) for x in (epsilon, nu_fluid, K, Fe)]
        check(self._lib.lb_set_porous(self._h, *vals))
        self.epsilon, self.nu_fluid, self.K, self.Fe = vals

    def set_body_force(self, gx, gy):
        """The constant body force per unit mass: the sum of the reference's add_constant_body_force calls."""
        vals = (float(np.float32(gx)), float(np.float32(gy)))
        check(self._lib.lb_set_body_force(self._h, *vals))
        self.body_force = vals

    def set_force_field(self, gx, gy):
        """A position-dependent body force added to the constant one in every cell: two (nx, ny) arrays; None, None drops it."""
        if gx is None and gy is None:
            check(self._lib.lb_set_force_field(self._h, None, None, 0))
            self._force_field = None
            return
        a, b = (_f_order(x, self._shape2) for x in (gx, gy))
        check(self._lib.lb_set_force_field(self._h, a.ctypes.data, b.ctypes.data, 0))
        self._force_field = (a.copy(order="F"), b.copy(order="F"))

    def set_bary_velocity(self, u_bary, v_bary):
        """The barycentric velocity update_feq and collide_particles read: two (nx, ny) arrays."""
        a, b = (_f_order(x, self._shape2) for x in (u_bary, v_bary))
        check(self._lib.lb_set_bary_velocity(self._h, a.ctypes.data, b.ctypes.data))

    def update_forces(self):
        """G := the body force, then the porosity and the two drags from rho, u, v (the reference's Gx, Gy = 0, the additional
        forces and update_forces_pourous: one kernel)."""
        check(self._lib.lb_update_forces(self._h))
        self.sync()

    def update_bary_velocity(self):
        """u_b = (sum f c + rho G / 2) / rho from the populations, rho and G.  rho = 0 gives NaN, as in the reference."""
        check(self._lib.lb_update_bary_velocity(self._h))
        self.sync()

    # -- the LB Poisson solver (semantics='poisson') --------------------------------
    def set_poisson(self, rho_on_boundary=0., react_factor=1., tolerance=1e-6):
        """The value prescribed on the four walls, the factor of the source term (the `delta_t * D` of the reference's
        collide_particles: every cell adds w_k source react_factor) and the tolerance of solve()'s stopping rule."""
        vals = [float(np.float32(x)) for x in (rho_on_boundary, react_factor, tolerance)]
        check(self._lib.lb_set_poisson(self._h, *vals))
        self.rho_on_boundary, self.react_factor, self.tolerance = vals

    def set_source(self, source):
        """The source field: an (nx, ny) array, or a float32 torch tensor of that shape already on this handle's device,
        which is copied device to device (lb_set_source)."""
        if hasattr(source, "data_ptr"):                         # a torch tensor
            import torch
            if tuple(source.shape) != self._shape2 or source.dtype != torch.float32 or not source.is_cuda:
                raise ValueError("a device source must be a float32 tensor of shape %s on the GPU" % (self._shape2,))
            dense = source.t().contiguous()                     # [ny][nx], x fastest: the ABI's layout
            torch.cuda.current_stream(dense.device).synchronize()
            check(self._lib.lb_set_source(self._h, dense.data_ptr(), 1))
            return
        s = _f_order(source, self._shape2)
        check(self._lib.lb_set_source(self._h, s.ctypes.data, 0))

    def get_source(self):
        out = np.zeros(self._shape2, np.float32, order="F")
        check(self._lib.lb_get_source(self._h, out.ctypes.data))
        return out

    def solve(self, max_iterations):
        """Up to max_iterations iterations of the reference's run loop; stops after the first iteration n >= 2 (counted since
        the last solve_reset) with mean |rho - rho_before| / mean rho_before < tolerance, decided on the device (lb_solve).
        Returns (iterations made by this call, converged, the ratio of the last iteration checked)."""
        n, c, r = ct.c_int(), ct.c_int(), ct.c_float()
        check(self._lib.lb_solve(self._h, int(max_iterations), ct.byref(n), ct.byref(c), ct.byref(r)))
        return n.value, bool(c.value), r.value

    def solve_reset(self):
        """The iteration counter back to 0 (what the reference's update_source does); rho and the populations stay."""
        check(self._lib.lb_solve_reset(self._h))

    def solve_state(self):
        """(iterations since the last solve_reset, the device's stop word: 0 or the iteration a solve stopped at)"""
        n, w = ct.c_int(), ct.c_int()
        check(self._lib.lb_get_solve_state(self._h, ct.byref(n), ct.byref(w)))
        return n.value, w.value

    def gradient(self, dx=1.0):
        """(d rho / dx, d rho / dy): central differences over 2 dx, 0 for a neighbour outside the box; (nx, ny) arrays, which
        get_fields()['u'], ['v'] return as well from then on (lb_gradient; it also takes device pointers).  (The
        reference's update_negative_gradient stores MINUS the y-difference as `u` and MINUS the x-difference as `v`: the
        drop-in class LB_D2Q9.poisson.Poisson_Solver keeps those names, this method does not.)"""
        ddx, ddy = np.zeros(self._shape2, np.float32, order="F"), np.zeros(self._shape2, np.float32, order="F")
        inv = float(np.float32(1.) / (np.float32(2.) * np.float32(dx)))
        check(self._lib.lb_gradient(self._h, inv, ddx.ctypes.data, ddy.ctypes.data))
        return ddx, ddy

    # -- scalar lattices (semantics='diffusion') -----------------------------------
    def set_reaction(self, G):
        """Growth rate of the Fisher term w_k G rho (1 - rho) added in the collision (D2Q9_diffusion.cl:95-124), lattice
        units; 0 = none."""
        check(self._lib.lb_set_reaction(self._h, float(np.float32(G))))
        self.G = float(np.float32(G))

    # (the noisy collision: public on LB_D2Q9.noisy_simulation.NoisySimulation; the kind row's checkpoint code reaches it from here)
    def _set_noise(self, Dg, seed=0):
        """The noisy collision (D2Q9_diffusion.cl:127-167): react = G rho (1 - rho) + sqrt(Dg rho (1 - rho)) z, f_k < 0 -> 0, with
        z a standard normal per cell and collision drawn inside the kernels from a counter-based stream (Philox4x32-10 under the
        64-bit `seed`; include/lb_hip.h has the definition).  Dg > 0 switches it on and resets the noise counter; 0 switches back to
        the plain cell.  rho outside [0, 1] gives NaN, as in the reference: check() counts such cells."""
        check(self._lib.lb_set_noise(self._h, float(np.float32(Dg)), int(seed) & 0xFFFFFFFFFFFFFFFF))

    def _noise(self):
        """(Dg, seed, t): t = the noise counter, the number of noisy collisions since set_noise."""
        dg, seed, t = ct.c_float(), ct.c_uint64(), ct.c_uint64()
        check(self._lib.lb_get_noise(self._h, ct.byref(dg), ct.byref(seed), ct.byref(t)))
        return dg.value, seed.value, t.value

    def _set_noise_counter(self, t):
        check(self._lib.lb_set_noise_counter(self._h, int(t)))

    def _noise_fill(self, t):
        """The (nx, ny) normals the kernels draw at noise counter t under the handle's seed (lb_noise_fill)."""
        out = np.zeros(self._shape2, np.float32, order="F")
        check(self._lib.lb_noise_fill(self._h, int(t), out.ctypes.data, 0))
        return out

    def _set_noise_field(self, z):
        """A supplied (nx, ny) field of normals that collide_particles() uses in place of the stream (the reference's random_normal
        buffer); None drops it.  While one is set run() refuses: a field is never used twice."""
        if z is None:
            check(self._lib.lb_set_noise_field(self._h, None, 0))
            return
        a = np.asfortranarray(z, np.float32)
        if a.shape != self._shape2:
            raise ValueError("noise field must have shape (nx, ny)")
        check(self._lib.lb_set_noise_field(self._h, a.ctypes.data, 0))

    def set_velocity_from(self, flow):
        """Take the imposed velocity from a flow Simulation of the same grid on the same device: its current u, v,
        copied device to device behind the flow's enqueued work (lb_set_velocity_from)."""
        check(self._lib.lb_set_velocity_from(self._h, flow._h))

    def edge_floats(self):
        n = self._lib.lb_edge_floats(self._h)
        if n < 0:
            check(n)
        return n

    def get_edge_state(self):
        """bc='open': the links that enter from outside the box, frozen since the last set_f / init_pop: 6 (nx + ny)
        floats in the order of include/lb_hip.h; empty in a periodic box."""
        out = np.zeros(self.edge_floats(), np.float32)
        check(self._lib.lb_get_edge_state(self._h, out.ctypes.data))
        return out

    def set_edge_state(self, values):
        v = np.ascontiguousarray(values, np.float32)
        if v.shape != (self.edge_floats(),):
            raise ValueError("edge state = %d floats" % self.edge_floats())
        check(self._lib.lb_set_edge_state(self._h, v.ctypes.data))

    def get_corner_state(self):
        """bc='velocity_inlet', and bc='box' of a coupled scalar lattice: the eight corner links no kernel of that rule set
        writes (include/lb_hip.h)."""
        out = np.zeros(8, np.float32)
        check(self._lib.lb_get_corner_state(self._h, out.ctypes.data))
        return out

    def set_corner_state(self, values):
        v = np.ascontiguousarray(values, np.float32)
        if v.shape != (8,):
            raise ValueError("corner state = 8 floats")
        check(self._lib.lb_set_corner_state(self._h, v.ctypes.data))

    @classmethod
    def from_checkpoint(cls, path, device=0, eager_macro=False):
        """Build a new Simulation from a checkpoint file.  eager_macro is a property of the handle, not of the state: a
        checkpoint written by a handle that rebuilds rho, u, v on demand holds the moments of the post-collision
        populations, one written by an eager handle the pre-collision ones (equal up to rounding, include/lb_hip.h); the
        populations, and hence every later step, are the same bits either way."""
        with np.load(cls._ckpt_path(path)) as d:
            if int(d["version"]) != cls.CHECKPOINT_VERSION:
                raise ValueError("checkpoint format %d, this build reads %d" % (int(d["version"]), cls.CHECKPOINT_VERSION))
            sim = cls(int(d["nx"]), int(d["ny"]), d["omega"][()], bc=int(d["bc_mode"]),        # (omega as it was given: the restored handle writes the same file)
                      inlet_rho=float(d["inlet_rho"]), outlet_rho=float(d["outlet_rho"]), lid_u=float(d["lid_u"]),
                      rho0=float(d["rho0"]), device=device, y0=int(d["y0"]), local_ny=int(d["local_ny"]),
                      halo=bool(int(d["halo"])), semantics=str(d["semantics"]),
                      inlet_u=float(d["inlet_u"]), outlet_u=float(d["outlet_u"]), eager_macro=eager_macro)
            sim.restore_arrays(d)
        return sim

    # -- row-slab stepping (driven by LB_D2Q9.slabs) -------------------------------
    def step_boundary(self, write_macro=False):
        check(self._lib.lb_step_boundary(self._h, int(bool(write_macro))))

    def step_interior(self, write_macro=False):
        check(self._lib.lb_step_interior(self._h, int(bool(write_macro))))

    def step_finish(self):
        check(self._lib.lb_step_finish(self._h))

    HALO_SEGMENTS = 18

    def halo_floats(self):
        """Length of one halo buffer in floats (18 row segments of nx, three rows deep)."""
        return self.HALO_SEGMENTS * self.nx

    MASK_HALO_ROWS = _native.LB_MASK_HALO_ROWS

    def set_obstacle_mask_halo(self, south_rows=None, north_rows=None):
        """Mask rows of the neighbouring slabs next to this one: south_rows = global rows y0-MASK_HALO_ROWS .. y0-1
        (nearest last), north_rows = rows y0+H .. y0+H+MASK_HALO_ROWS-1 (nearest first), each (MASK_HALO_ROWS, nx),
        non-zero = solid; None = no solid cells."""
        rows = []
        for r in (south_rows, north_rows):
            if r is not None and np.asarray(r).shape != (self.MASK_HALO_ROWS, self.nx):
                raise ValueError("mask halo must have shape (%d, nx)" % self.MASK_HALO_ROWS)
            rows.append(None if r is None else np.ascontiguousarray((np.asarray(r) != 0).astype(np.int32)))
        ptr = lambda a: None if a is None else a.ctypes.data
        check(self._lib.lb_set_mask_halo(self._h, ptr(rows[0]), ptr(rows[1])))
        self._mask_halo_host = tuple(rows)

    def halo_export(self, side, buf):
        """Copy the halo leaving through edge `side` (0 south, 1 north) into buf[18*nx]
        (numpy float32 array or a raw host/device address); layout: include/lb_hip.h."""
        check(self._lib.lb_halo_export(self._h, int(side), _address(buf)))

    def halo_import(self, side, buf):
        check(self._lib.lb_halo_import(self._h, int(side), _address(buf)))

    def use_stream(self, hip_stream):
        """Run on an external hipStream_t (integer handle, e.g. torch.cuda.Stream(...).cuda_stream); None = back to the handle's own
        stream.  Waits for the work enqueued on the stream it leaves.  The legacy default stream cannot be named: its handle is 0,
        which lb_set_stream reads as None -- and the own stream is ordered with nothing else (torch's current stream is that
        default stream unless the caller made another one current), so 0 is refused here instead of silently meaning `own`."""
        if hip_stream is not None and int(hip_stream) == 0:
            raise ValueError("stream handle 0 is the legacy default stream, which lb_set_stream cannot name (NULL = the handle's own "
                             "stream): run the torch side on a torch.cuda.Stream and pass its cuda_stream, or pass None")
        check(self._lib.lb_set_stream(self._h, hip_stream))

    def comm_init(self, unique_id, rank, nranks):
        """Attach an RCCL communicator: run() then exchanges halos itself (lb_comm_init)."""
        check(self._lib.lb_comm_init(self._h, unique_id, int(rank), int(nranks)))

    def peer_export(self):
        """This handle's descriptor for the peer transport (lb_peer_export): IPC handles of its lattices and flag block,
        LB_PEER_HANDLE_BYTES bytes to be carried to the two neighbouring ranks."""
        buf = (ct.c_char * _native.LB_PEER_HANDLE_BYTES)()
        check(self._lib.lb_peer_export(self._h, buf))
        return bytes(buf.raw)

    def peer_connect(self, rank, nranks, south, north, min_h):
        """Map the neighbours' descriptors (bytes from their peer_export(); None at a wall) and switch run() on this slab
        to the peer transport: halo rows stored straight into the neighbours' ghost rows (lb_peer_connect)."""
        check(self._lib.lb_peer_connect(self._h, int(rank), int(nranks), south, north, int(min_h)))

    # -- tuning / introspection ------------------------------------------------
    def copy_calibration(self, iters=10, nontemporal=False):
        """Time `iters` plain float4 copies of one lattice into the other (known bytes).
        Returns (GB/s, bytes per launch).  Only between steps: it overwrites the scratch lattice."""
        nbytes, ms = ct.c_int64(), ct.c_float()
        check(self._lib.lb_copy_calibration(self._h, int(nontemporal), ct.byref(nbytes)))
        check(self._lib.lb_timer_start(self._h))
        for _ in range(iters):
            check(self._lib.lb_copy_calibration(self._h, int(nontemporal), ct.byref(nbytes)))
        check(self._lib.lb_timer_stop(self._h, ct.byref(ms)))
        return nbytes.value * iters / (ms.value * 1e-3) / 1e9, nbytes.value

    def set_variant(self, variant):
        """Which fused kernel runs (lb_set_variant): an int, variants.AUTO (-1, the default) or a word made of the names in
        LB_D2Q9/variants.py, e.g. variants.K_STEP5 or variants.marching(3) | variants.NO_CYCLE.  Results never depend on it."""
        check(self._lib.lb_set_variant(self._h, int(variant)))

    def set_slab_cycle(self, depth):
        """Slab handles: depth of the fused kernel the halo cycle runs on (0 = automatic, 3 ... 7; 8 = seven steps by k_deep2, two waves
        per SIMD); every rank of a run must set the same value (lb_set_slab_cycle)."""
        check(self._lib.lb_set_slab_cycle(self._h, int(depth)))

    def set_exchange_inline(self, on):
        """Slab handles: the halo exchange of a cycle on the compute stream, between the interior launches (True), instead of beside
        them on the communication stream (False, the default); every rank of a run must set the same value (lb_set_exchange_inline)."""
        check(self._lib.lb_set_exchange_inline(self._h, int(bool(on))))

    def exchange_timing(self, enable=True):
        """Slab handles: time every halo exchange of run() on its stream from now on (lb_exchange_timing)."""
        check(self._lib.lb_exchange_timing(self._h, int(bool(enable))))

    def exchange_stats(self):
        """The exchanges timed since the last call: {"n", "total_ms", "max_ms", "cycle_depth", "band_rows"} (lb_exchange_stats)."""
        n, tot, mx, d, b = ct.c_int64(), ct.c_double(), ct.c_double(), ct.c_int(), ct.c_int()
        check(self._lib.lb_exchange_stats(self._h, ct.byref(n), ct.byref(tot), ct.byref(mx), ct.byref(d), ct.byref(b)))
        return {"n": n.value, "total_ms": tot.value, "max_ms": mx.value, "cycle_depth": d.value, "band_rows": b.value}

    def autotune(self):
        """Time the candidate fused-kernel configurations on a few live steps and keep the fastest for this
        grid (bitwise-equivalent candidates).  Returns the number of time steps the simulation advanced."""
        n = self._lib.lb_autotune(self._h)
        if n < 0:
            check(n)
        return n

    def hot_kernel(self):
        """Name of the kernel run() spends its time in for this grid / variant / tuning (lb_hot_kernel)."""
        buf = ct.create_string_buffer(256)
        check(self._lib.lb_hot_kernel(self._h, buf, len(buf)))
        return buf.value.decode()

    def plan_launches(self, num_iterations):
        """The time steps of each launch run(num_iterations) would make, in order (whole-grid OpenCL-path GPU handles; None
        elsewhere): every launch of a marching kernel moves the same bytes whatever number of steps it fuses."""
        buf = (ct.c_int * 256)()
        n = self._lib.lb_plan_launches(self._h, int(num_iterations), buf, 256)
        if n < 0:
            return None
        return [int(buf[i]) for i in range(min(n, 256))]

    def steps_per_launch(self):
        """Time steps one launch of run()'s hot kernel advances for this grid / variant / tuning: 4, 3, 2 or 1."""
        n = self._lib.lb_steps_per_launch(self._h)
        if n < 0:
            check(n)
        return n

    def layout(self):
        a, b, c = ct.c_int64(), ct.c_int64(), ct.c_int64()
        check(self._lib.lb_layout(self._h, ct.byref(a), ct.byref(b), ct.byref(c)))
        return {"pitch": a.value, "plane_stride": b.value, "bytes": c.value, "planar": self.planar}
