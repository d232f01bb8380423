"""ctypes binding of liblbhip.so (C ABI: include/lb_hip.h).

The library is the only compute backend.  If it is missing or no GPU is visible the
functions raise; nothing falls back to the CPU."""
import ctypes as ct
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LB_LIB") or os.path.join(_HERE, "liblbhip.so")   # LB_LIB: diagnostic builds only

LB_BC_PIPE, LB_BC_PERIODIC, LB_BC_CAVITY, LB_BC_VELOCITY_INLET, LB_BC_OPEN, LB_BC_BOX, LB_BC_DIRICHLET = 0, 1, 2, 3, 4, 5, 6
LB_BC_ZERO_GRADIENT = 7
LB_FLAG_HALO = 1
LB_FLAG_PLANAR = 2
LB_FLAG_EAGER_MACRO = 4
LB_MASK_HALO_ROWS = 13
LB_PEER_HANDLE_BYTES = 384
LB_DEVICE_CPU = -1
LB_SEM_OPENCL, LB_SEM_CYTHON, LB_SEM_OPENCL_D2Q9I, LB_SEM_DIFFUSION, LB_SEM_MULTIFIELD, LB_SEM_POISSON = 0, 1, 2, 3, 4, 5
LB_SEM_POROUS = 7        # (6 is not assigned: include/lb_hip.h)
LB_SEM_MULTIFLUID = 9    # (nor is 8)
LB_PSI_LINEAR, LB_PSI_SHAN_CHEN, LB_PSI_POW = 0, 1, 2
LB_REACT_EAT, LB_REACT_GROW = 0, 1
MC_MAX, MC_MAX_INTER, MC_MAX_REACT = 3, 6, 4
LB_SEM_ROCKET = 11       # (nor is 10)
LB_ROCKET_FLOW, LB_ROCKET_FORCES = 0, 1
RY_ROWS = 10             # rows of a 256-cell tile a workgroup of k_ry_step owns (csrc/plan_consts.h; lb_hot_kernel names it)
BC_NAMES = {"pipe": LB_BC_PIPE, "periodic": LB_BC_PERIODIC, "cavity": LB_BC_CAVITY,
            "velocity_inlet": LB_BC_VELOCITY_INLET, "open": LB_BC_OPEN, "box": LB_BC_BOX, "dirichlet": LB_BC_DIRICHLET,
            "zero_gradient": LB_BC_ZERO_GRADIENT}

ABI_VERSION = 11

# every symbol include/lb_hip.h declares (checked by tests/test_abi.py)
EXPORTS = (
    "lb_abi_version", "lb_device_count", "lb_last_error", "lb_create", "lb_destroy", "lb_sync", "lb_set_stream",
    "lb_set_macro", "lb_get_macro", "lb_set_f", "lb_get_f", "lb_get_feq", "lb_set_mask",
    "lb_move", "lb_move_bcs", "lb_update_hydro", "lb_update_feq", "lb_collide_particles",
    "lb_zero_velocity_in_obstacle", "lb_init_pop", "lb_run",
    "lb_step_boundary", "lb_step_interior", "lb_step_finish", "lb_halo_export", "lb_halo_import",
    "lb_halo_floats", "lb_set_mask_halo", "lb_run_group", "lb_run_batch",
    "lb_comm_available", "lb_comm_unique_id", "lb_comm_init", "lb_timer_start", "lb_timer_stop", "lb_layout", "lb_set_variant", "lb_copy_calibration", "lb_steps_per_launch", "lb_plan_launches", "lb_autotune",
    "lb_autotune_quick", "lb_hot_kernel", "lb_get_corner_state", "lb_set_corner_state", "lb_check", "lb_set_debug_sync",
    "lb_peer_export", "lb_peer_connect", "lb_set_params_f64", "lb_set_slab_cycle", "lb_exchange_timing", "lb_exchange_stats",
    "lb_set_exchange_inline",
    "lb_set_reaction", "lb_edge_floats", "lb_get_edge_state", "lb_set_edge_state", "lb_set_velocity_from",
    "lb_run_coupled", "lb_collide_coupled",
    "lb_set_poisson", "lb_set_source", "lb_get_source", "lb_solve", "lb_solve_reset", "lb_get_solve_state", "lb_set_solve_state",
    "lb_gradient",
    "lb_set_porous", "lb_set_body_force", "lb_set_force_field", "lb_get_force", "lb_set_force", "lb_set_bary_velocity",
    "lb_get_bary_velocity", "lb_update_forces", "lb_update_bary_velocity",
    "lb_run_fluids", "lb_set_interactions", "lb_set_reactions", "lb_get_interactions", "lb_get_reactions",
    "lb_update_forces_fluids", "lb_update_bary_fluids", "lb_react_fluids",
    "lb_set_rocket", "lb_get_rocket", "lb_run_rocket", "lb_update_velocity_rocket", "lb_update_forces_rocket", "lb_collide_rocket",
    "lb_get_rocket_fields",
)


class LbParams(ct.Structure):
    _fields_ = [("nx", ct.c_int32), ("ny", ct.c_int32), ("y0", ct.c_int32), ("local_ny", ct.c_int32),
                ("bc_mode", ct.c_int32), ("device", ct.c_int32),
                ("omega", ct.c_float), ("inlet_rho", ct.c_float), ("outlet_rho", ct.c_float),
                ("lid_u", ct.c_float), ("rho0", ct.c_float), ("flags", ct.c_int32), ("semantics", ct.c_int32),
                ("inlet_u", ct.c_float), ("outlet_u", ct.c_float), ("reserved", ct.c_int32 * 1)]


class Interaction(ct.Structure):         # lb_interaction
    _fields_ = [("fluid_1", ct.c_int32), ("fluid_2", ct.c_int32), ("potential", ct.c_int32), ("boundary", ct.c_int32),
                ("G_int", ct.c_float), ("parameter", ct.c_float)]


class FluidReaction(ct.Structure):       # lb_fluid_reaction
    _fields_ = [("kind", ct.c_int32), ("fluid_a", ct.c_int32), ("fluid_b", ct.c_int32),
                ("p0", ct.c_float), ("p1", ct.c_float), ("p2", ct.c_float)]


class RocketParams(ct.Structure):        # lb_rocket_params
    _fields_ = [("mode", ct.c_int32), ("G", ct.c_float), ("G_c", ct.c_float), ("epsilon", ct.c_float), ("rho_o", ct.c_float),
                ("G_chen", ct.c_float), ("c_o", ct.c_float), ("alpha", ct.c_float)]


class LbError(RuntimeError):
    pass


_lib = None


def lib():
    """Load liblbhip.so once.  Raises LbError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LbError("%s not found: build it with `python 2d-lb_amd/build.py` "
                      "(the engine has no CPU fallback)" % LIB_PATH)
    L = ct.CDLL(LIB_PATH)
    h, fp, vp, I = ct.c_void_p, ct.POINTER(ct.c_float), ct.c_void_p, ct.c_int
    L.lb_last_error.restype = ct.c_char_p
    L.lb_create.argtypes = [ct.POINTER(LbParams), ct.POINTER(h)]
    for name in ("lb_destroy", "lb_sync", "lb_move", "lb_move_bcs", "lb_update_hydro", "lb_update_feq",
                 "lb_collide_particles", "lb_zero_velocity_in_obstacle", "lb_init_pop", "lb_step_finish",
                 "lb_timer_start", "lb_steps_per_launch", "lb_autotune"):
        getattr(L, name).argtypes = [h]
    L.lb_plan_launches.argtypes = [h, I, ct.POINTER(ct.c_int), I]
    L.lb_set_stream.argtypes = [h, vp]
    L.lb_set_macro.argtypes = [h, vp, vp, vp]
    L.lb_get_macro.argtypes = [h, vp, vp, vp]
    L.lb_set_f.argtypes = [h, vp]
    L.lb_get_f.argtypes = [h, vp]
    L.lb_get_feq.argtypes = [h, vp]
    L.lb_set_mask.argtypes = [h, vp]
    L.lb_run.argtypes = [h, I]
    L.lb_step_boundary.argtypes = [h, I]
    L.lb_step_interior.argtypes = [h, I]
    L.lb_halo_export.argtypes = [h, I, vp]
    L.lb_halo_import.argtypes = [h, I, vp]
    L.lb_halo_floats.argtypes = [h]
    L.lb_set_mask_halo.argtypes = [h, vp, vp]
    L.lb_run_group.argtypes = [ct.POINTER(h), I, I]
    L.lb_run_batch.argtypes = [ct.POINTER(h), I, I]
    L.lb_comm_unique_id.argtypes = [vp]
    # (an older diagnostic build selected with LB_LIB -- A/B timing of kernels across rounds -- lacks the newest entry points)
    older = bool(os.environ.get("LB_LIB")) and L.lb_abi_version() < ABI_VERSION
    if not older:
        L.lb_peer_export.argtypes = [h, vp]
        L.lb_peer_connect.argtypes = [h, I, I, vp, vp, I]
        L.lb_set_params_f64.argtypes = [h, ct.c_double, ct.c_double, ct.c_double]
    if L.lb_abi_version() >= 9:
        L.lb_set_slab_cycle.argtypes = [h, I]
        L.lb_exchange_timing.argtypes = [h, I]
        L.lb_exchange_stats.argtypes = [h, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_double), ct.POINTER(ct.c_double),
                                        ct.POINTER(ct.c_int), ct.POINTER(ct.c_int)]
    if L.lb_abi_version() >= 10:
        L.lb_set_exchange_inline.argtypes = [h, I]
    if L.lb_abi_version() >= 11:
        L.lb_set_reaction.argtypes = [h, ct.c_float]
        L.lb_edge_floats.argtypes = [h]
        L.lb_get_edge_state.argtypes = [h, vp]
        L.lb_set_edge_state.argtypes = [h, vp]
        L.lb_set_velocity_from.argtypes = [h, h]
    if hasattr(L, "lb_run_coupled"):                # (added within ABI 11: an older diagnostic build of that version lacks them)
        L.lb_run_coupled.argtypes = [ct.POINTER(h), I, I]
        L.lb_collide_coupled.argtypes = [ct.POINTER(h), I]
    if hasattr(L, "lb_solve"):                      # (likewise: the LB Poisson solver)
        ip = ct.POINTER(ct.c_int)
        L.lb_set_poisson.argtypes = [h, ct.c_float, ct.c_float, ct.c_float]
        L.lb_set_source.argtypes = [h, vp, I]
        L.lb_get_source.argtypes = [h, vp]
        L.lb_solve.argtypes = [h, I, ip, ip, fp]
        L.lb_solve_reset.argtypes = [h]
        L.lb_get_solve_state.argtypes = [h, ip, ip]
        L.lb_set_solve_state.argtypes = [h, I, I]
        L.lb_gradient.argtypes = [h, ct.c_float, vp, vp]
    if hasattr(L, "lb_set_porous"):                 # (likewise: forced flow in a porous medium; bound by presence, not by version)
        L.lb_set_porous.argtypes = [h, ct.c_float, ct.c_float, ct.c_float, ct.c_float]
        L.lb_set_body_force.argtypes = [h, ct.c_float, ct.c_float]
        L.lb_set_force_field.argtypes = [h, vp, vp, I]
        for name in ("lb_get_force", "lb_set_force", "lb_set_bary_velocity", "lb_get_bary_velocity"):
            getattr(L, name).argtypes = [h, vp, vp]
        L.lb_update_forces.argtypes = [h]
        L.lb_update_bary_velocity.argtypes = [h]
    if hasattr(L, "lb_run_fluids"):                 # (likewise: multicomponent Shan-Chen fluids)
        hp, ip = ct.POINTER(h), ct.POINTER(ct.c_int)
        L.lb_run_fluids.argtypes = [hp, I, I]
        L.lb_set_interactions.argtypes = [hp, I, ct.POINTER(Interaction), I]
        L.lb_set_reactions.argtypes = [hp, I, ct.POINTER(FluidReaction), I]
        L.lb_get_interactions.argtypes = [h, ct.POINTER(Interaction), ip]
        L.lb_get_reactions.argtypes = [h, ct.POINTER(FluidReaction), ip]
        for name in ("lb_update_forces_fluids", "lb_update_bary_fluids", "lb_react_fluids"):
            getattr(L, name).argtypes = [hp, I]
    if hasattr(L, "lb_run_rocket"):                 # (likewise: surfactant-propelled colonies)
        hp = ct.POINTER(h)
        L.lb_set_rocket.argtypes = [hp, I, ct.POINTER(RocketParams)]
        L.lb_get_rocket.argtypes = [h, ct.POINTER(RocketParams)]
        L.lb_run_rocket.argtypes = [hp, I, I]
        for name in ("lb_update_velocity_rocket", "lb_update_forces_rocket", "lb_collide_rocket"):
            getattr(L, name).argtypes = [hp, I]
        L.lb_get_rocket_fields.argtypes = [hp, I, vp, vp, vp, vp, vp]
    L.lb_comm_init.argtypes = [h, vp, I, I]
    L.lb_timer_stop.argtypes = [h, fp]
    L.lb_layout.argtypes = [h, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]
    L.lb_set_variant.argtypes = [h, I]
    L.lb_copy_calibration.argtypes = [h, I, ct.POINTER(ct.c_int64)]
    L.lb_autotune_quick.argtypes = [h, I]
    L.lb_get_corner_state.argtypes = [h, vp]
    L.lb_set_corner_state.argtypes = [h, vp]
    L.lb_hot_kernel.argtypes = [h, ct.c_char_p, I]
    L.lb_check.argtypes = [h, I, ct.POINTER(ct.c_int64), fp, ct.POINTER(ct.c_double)]
    L.lb_set_debug_sync.argtypes = [I]
    if L.lb_abi_version() != ABI_VERSION and not older:
        raise LbError("liblbhip.so ABI %d != binding ABI %d: rebuild" % (L.lb_abi_version(), ABI_VERSION))
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise LbError("liblbhip: %s (status %d)" % (lib().lb_last_error().decode(), rc))


def device_count():
    n = lib().lb_device_count()
    if n < 0:
        raise LbError("liblbhip: %s" % lib().lb_last_error().decode())
    return n
