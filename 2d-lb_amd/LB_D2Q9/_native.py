"""ctypes binding of liblbhip.so (C ABI: include/lb_hip.h).

The library is the only compute backend.  If it is missing or no GPU is visible the
functions raise; nothing falls back to the CPU."""
import ctypes as ct
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LB_LIB") or os.path.join(_HERE, "liblbhip.so")   # LB_LIB: diagnostic builds only

# boundary families (lb_params.bc_mode)
LB_BC_PIPE, LB_BC_PERIODIC, LB_BC_CAVITY, LB_BC_VELOCITY_INLET, LB_BC_OPEN, LB_BC_BOX, LB_BC_DIRICHLET, LB_BC_ZERO_GRADIENT = range(8)
BC_NAMES = {"pipe": LB_BC_PIPE, "periodic": LB_BC_PERIODIC, "cavity": LB_BC_CAVITY,
            "velocity_inlet": LB_BC_VELOCITY_INLET, "open": LB_BC_OPEN, "box": LB_BC_BOX, "dirichlet": LB_BC_DIRICHLET,
            "zero_gradient": LB_BC_ZERO_GRADIENT}
# handle kinds (lb_params.semantics; 6, 8 and 10 are not assigned: include/lb_hip.h)
LB_SEM_OPENCL, LB_SEM_CYTHON, LB_SEM_OPENCL_D2Q9I, LB_SEM_DIFFUSION, LB_SEM_MULTIFIELD, LB_SEM_POISSON = 0, 1, 2, 3, 4, 5
LB_SEM_POROUS, LB_SEM_MULTIFLUID, LB_SEM_ROCKET = 7, 9, 11
# lb_params.flags and .device
LB_FLAG_HALO, LB_FLAG_PLANAR, LB_FLAG_EAGER_MACRO = 1, 2, 4
LB_DEVICE_CPU = -1
# slabs
LB_MASK_HALO_ROWS = 13
LB_PEER_HANDLE_BYTES = 384
# the tables of a set of fluids, the modes of a colony
LB_PSI_LINEAR, LB_PSI_SHAN_CHEN, LB_PSI_POW = 0, 1, 2
LB_REACT_EAT, LB_REACT_GROW = 0, 1
MC_MAX, MC_MAX_INTER, MC_MAX_REACT = 3, 6, 4
LB_ROCKET_FLOW, LB_ROCKET_FORCES = 0, 1
RY_ROWS = 10             # rows of a 256-cell tile a workgroup of k_ry_step owns (csrc/plan_consts.h; lb_hot_kernel names it)
MC_ROWS = {1: 6, 2: 6, 3: 2}    # ... of k_mc_step, by the number of fluids (csrc/multifluid.cpp, step_rows)
SN_ROWS = 4              # ... of k_sn_step (csrc/nutrient_launch.h)

ABI_VERSION = 11


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


class NutrientParams(ct.Structure):      # lb_nutrient_params
    _fields_ = [("G", ct.c_float), ("scale", ct.c_float), ("clumpy", ct.c_int32), ("rho_o", ct.c_float), ("G_chen", ct.c_float)]


class ExpansionParams(ct.Structure):     # lb_expansion_params
    _fields_ = [("zero_cutoff", ct.c_float)]


class LbError(RuntimeError):
    pass


_h, _hp, _vp, _I, _F, _D = ct.c_void_p, ct.POINTER(ct.c_void_p), ct.c_void_p, ct.c_int, ct.c_float, ct.c_double
_ip, _fp, _dp, _i64p = ct.POINTER(ct.c_int), ct.POINTER(ct.c_float), ct.POINTER(ct.c_double), ct.POINTER(ct.c_int64)
_U64, _u64p = ct.c_uint64, ct.POINTER(ct.c_uint64)

# every function include/lb_hip.h declares, in its order: name -> (argtypes[, restype]); tests/test_abi.py holds the names to the header
SIGNATURES = {
    "lb_abi_version": ([],), "lb_device_count": ([],), "lb_last_error": ([], ct.c_char_p),
    "lb_create": ([ct.POINTER(LbParams), _hp],), "lb_destroy": ([_h],),
    "lb_set_params_f64": ([_h, _D, _D, _D],), "lb_sync": ([_h],), "lb_set_stream": ([_h, _vp],),
    "lb_set_macro": ([_h, _vp, _vp, _vp],), "lb_get_macro": ([_h, _vp, _vp, _vp],),
    "lb_set_f": ([_h, _vp],), "lb_get_f": ([_h, _vp],), "lb_get_feq": ([_h, _vp],), "lb_set_mask": ([_h, _vp],),
    "lb_get_corner_state": ([_h, _vp],), "lb_set_corner_state": ([_h, _vp],),
    # scalar lattices
    "lb_set_reaction": ([_h, _F],), "lb_edge_floats": ([_h],), "lb_get_edge_state": ([_h, _vp],),
    "lb_set_edge_state": ([_h, _vp],), "lb_set_velocity_from": ([_h, _h],),
    # ... their noisy collision
    "lb_set_noise": ([_h, _F, _U64],), "lb_get_noise": ([_h, _fp, _u64p, _u64p],), "lb_set_noise_counter": ([_h, _U64],),
    "lb_noise_fill": ([_h, _U64, _vp, _I],), "lb_set_noise_field": ([_h, _vp, _I],),
    # the LB Poisson solver
    "lb_set_poisson": ([_h, _F, _F, _F],), "lb_set_source": ([_h, _vp, _I],), "lb_get_source": ([_h, _vp],),
    "lb_solve": ([_h, _I, _ip, _ip, _fp],), "lb_solve_reset": ([_h],), "lb_get_solve_state": ([_h, _ip, _ip],),
    "lb_set_solve_state": ([_h, _I, _I],), "lb_gradient": ([_h, _F, _vp, _vp],),
    # forced flow in a porous medium
    "lb_set_porous": ([_h, _F, _F, _F, _F],), "lb_set_body_force": ([_h, _F, _F],), "lb_set_force_field": ([_h, _vp, _vp, _I],),
    "lb_get_force": ([_h, _vp, _vp],), "lb_set_force": ([_h, _vp, _vp],),
    "lb_set_bary_velocity": ([_h, _vp, _vp],), "lb_get_bary_velocity": ([_h, _vp, _vp],),
    "lb_update_forces": ([_h],), "lb_update_bary_velocity": ([_h],),
    # multicomponent Shan-Chen fluids
    "lb_run_fluids": ([_hp, _I, _I],),
    "lb_set_interactions": ([_hp, _I, ct.POINTER(Interaction), _I],), "lb_set_reactions": ([_hp, _I, ct.POINTER(FluidReaction), _I],),
    "lb_get_interactions": ([_h, ct.POINTER(Interaction), _ip],), "lb_get_reactions": ([_h, ct.POINTER(FluidReaction), _ip],),
    "lb_update_forces_fluids": ([_hp, _I],), "lb_update_bary_fluids": ([_hp, _I],), "lb_react_fluids": ([_hp, _I],),
    # surfactant-propelled colonies
    "lb_set_rocket": ([_hp, _I, ct.POINTER(RocketParams)],), "lb_get_rocket": ([_h, ct.POINTER(RocketParams)],),
    "lb_run_rocket": ([_hp, _I, _I],), "lb_update_velocity_rocket": ([_hp, _I],), "lb_update_forces_rocket": ([_hp, _I],),
    "lb_collide_rocket": ([_hp, _I],), "lb_get_rocket_fields": ([_hp, _I, _vp, _vp, _vp, _vp, _vp],),
    # the phases and the hot path
    "lb_move": ([_h],), "lb_move_bcs": ([_h],), "lb_update_hydro": ([_h],), "lb_update_feq": ([_h],),
    "lb_collide_particles": ([_h],), "lb_zero_velocity_in_obstacle": ([_h],), "lb_init_pop": ([_h],), "lb_run": ([_h, _I],),
    # row slabs, sets of handles, communicators
    "lb_step_boundary": ([_h, _I],), "lb_step_interior": ([_h, _I],), "lb_step_finish": ([_h],), "lb_halo_floats": ([_h],),
    "lb_halo_export": ([_h, _I, _vp],), "lb_halo_import": ([_h, _I, _vp],), "lb_set_mask_halo": ([_h, _vp, _vp],),
    "lb_run_group": ([_hp, _I, _I],), "lb_run_batch": ([_hp, _I, _I],), "lb_run_coupled": ([_hp, _I, _I],),
    "lb_collide_coupled": ([_hp, _I],),
    "lb_comm_available": ([],), "lb_comm_unique_id": ([_vp],), "lb_comm_init": ([_h, _vp, _I, _I],),
    "lb_peer_export": ([_h, _vp],), "lb_peer_connect": ([_h, _I, _I, _vp, _vp, _I],),
    # health, timing, tuning
    "lb_check": ([_h, _I, _i64p, _fp, _dp],), "lb_set_debug_sync": ([_I],),
    "lb_timer_start": ([_h],), "lb_timer_stop": ([_h, _fp],), "lb_layout": ([_h, _i64p, _i64p, _i64p],),
    "lb_steps_per_launch": ([_h],), "lb_plan_launches": ([_h, _I, _ip, _I],), "lb_hot_kernel": ([_h, ct.c_char_p, _I],),
    "lb_autotune": ([_h],), "lb_autotune_quick": ([_h, _I],), "lb_copy_calibration": ([_h, _I, _i64p],),
    "lb_set_variant": ([_h, _I],), "lb_set_slab_cycle": ([_h, _I],), "lb_set_exchange_inline": ([_h, _I],),
    "lb_exchange_timing": ([_h, _I],), "lb_exchange_stats": ([_h, _i64p, _dp, _dp, _ip, _ip],),
    # the spectral screened-Poisson solver (an lb_spectral is not a handle kind; which: 0 charge, 1 xgrad, 2 ygrad)
    "lb_spectral_create": ([_I, _I, _I, _D, _hp],), "lb_spectral_destroy": ([_h],), "lb_spectral_set_lambda": ([_h, _D],),
    "lb_spectral_set": ([_h, _I, _vp, _I],), "lb_spectral_get": ([_h, _I, _vp],),
    "lb_spectral_transform": ([_h, _I, _I],), "lb_spectral_screen": ([_h],), "lb_spectral_grad_multiply": ([_h],),
    "lb_spectral_solve": ([_h],), "lb_spectral_velocity": ([_h, _h, _F, _I],), "lb_run_screened": ([_h, _h, _F, _I],),
    # a population and its nutrient under the solver's velocity (two scalar lattices and an lb_spectral; the parameters: NutrientParams)
    "lb_run_nutrient": ([_h, _hp, _I, ct.POINTER(NutrientParams), _I],), "lb_nutrient_velocity": ([_h, _hp, _I, _F, _I],),
    "lb_update_forces_nutrient": ([_hp, _I, ct.POINTER(NutrientParams)],), "lb_collide_nutrient": ([_hp, _I, ct.POINTER(NutrientParams)],),
    "lb_get_nutrient_fields": ([_hp, _I, _vp, _vp, _vp],),
    # noisy strains on a shared nutrient (2 ... 4 scalar lattices, the nutrient last; the parameters: ExpansionParams)
    "lb_run_expansion": ([_hp, _I, ct.POINTER(ExpansionParams), _I],), "lb_update_hydro_expansion": ([_hp, _I, ct.POINTER(ExpansionParams)],),
    "lb_collide_expansion": ([_hp, _I, ct.POINTER(ExpansionParams)],),
    # a flow and the scalars it carries (flow, scalars, count, n_steps, form); the name of what runs (count, form, cells, buf, buflen)
    "lb_run_advected": ([_h, _hp, _I, _I, _I],), "lb_advected_kernel": ([_I, _I, ct.c_int64, ct.c_char_p, _I],),
}
EXPORTS = tuple(SIGNATURES)

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
    for name, (argtypes, *restype) in SIGNATURES.items():
        if hasattr(L, name):        # (an older diagnostic build selected with LB_LIB -- A/B timing of kernels -- lacks the newest entry points)
            getattr(L, name).argtypes = argtypes
            if restype:
                getattr(L, name).restype = restype[0]
    older = bool(os.environ.get("LB_LIB")) and L.lb_abi_version() < ABI_VERSION
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
