"""One row per value of ``Simulation(semantics=...)``: the handle kind's code in the library, whether ``run()`` makes the
tuning pass first, whether a checkpoint restores an obstacle mask, and what the kind adds to a checkpoint and puts back from
one.  ``Simulation`` reads the row; a new physics adds a row (and its setters to ``Simulation``).

``save(sim, d)`` adds the kind's entries to the dict ``d`` of ``checkpoint_arrays()``; ``restore(sim, d)`` runs behind ``set_f``,
which resets a lattice's edge and corner state to the populations' own.  The corner state of ``bc='velocity_inlet'`` belongs to
the boundary family, not to a kind: ``Simulation`` handles it itself."""
from collections import namedtuple

import numpy as np

from . import _native

Kind = namedtuple("Kind", "name sem tunes has_mask save restore")


def _nothing(sim, d):
    pass


# -- the scalar lattices: the growth rate, and the links no kernel of their boundary rule writes ----------------------------
def _save_growth(sim, d):
    d["G"] = np.float32(sim.G)


def _restore_growth(sim, d):
    sim.set_reaction(float(d["G"]))


def _save_diffusion(sim, d):
    _save_growth(sim, d)
    d["edge_state"] = sim.get_edge_state()
    # the noisy collision: [Dg as its float32 bit pattern, seed, noise counter], uint64 -- only where it is on (a checkpoint of a
    # handle without noise keeps its entries); a supplied noise field is not part of a checkpoint
    dg, seed, t = sim._noise()
    if dg != 0.:
        d["noise"] = np.array([int(np.float32(dg).view(np.uint32)), seed, t], np.uint64)


def _restore_diffusion(sim, d):
    _restore_growth(sim, d)
    sim.set_edge_state(d["edge_state"])
    if "noise" in d:
        bits, seed, t = (int(x) for x in d["noise"])
        sim._set_noise(float(np.uint32(bits).view(np.float32)), seed)
        sim._set_noise_counter(t)


def _save_multifield(sim, d):
    _save_growth(sim, d)
    d["corner_state"] = sim.get_corner_state()


def _restore_multifield(sim, d):
    _restore_growth(sim, d)
    sim.set_corner_state(d["corner_state"])


def _save_poisson(sim, d):
    d["corner_state"] = sim.get_corner_state()
    d["source"] = sim.get_source()
    d["poisson"] = np.array([sim.rho_on_boundary, sim.react_factor, sim.tolerance], np.float32)
    d["solve_state"] = np.array(sim.solve_state(), np.int32)


def _restore_poisson(sim, d):
    sim.set_poisson(*[float(x) for x in d["poisson"]])
    sim.set_source(d["source"])
    sim.set_corner_state(d["corner_state"])
    sim._set_solve_state(*d["solve_state"])


# -- the forced fluids: body force, force field, barycentric velocity and the force of the last step ------------------------
def _save_forcing(sim, d):
    g = sim.get_fields(("u_bary", "v_bary", "Gx", "Gy"))
    d["body_force"] = np.array(sim.body_force, np.float32)
    d["bary"] = np.stack([g["u_bary"], g["v_bary"]])
    d["force"] = np.stack([g["Gx"], g["Gy"]])
    if sim._force_field is not None:
        d["force_field"] = np.stack(sim._force_field)


def _restore_forcing(sim, d):
    sim.set_body_force(*[float(x) for x in d["body_force"]])
    sim.set_force_field(*(d["force_field"] if "force_field" in d else (None, None)))
    sim.set_bary_velocity(d["bary"][0], d["bary"][1])
    sim._set_force(d["force"][0], d["force"][1])


def _save_porous(sim, d):
    d["porous"] = np.array([sim.epsilon, sim.nu_fluid, sim.K, sim.Fe], np.float32)
    _save_forcing(sim, d)


def _restore_porous(sim, d):
    sim.set_porous(*[float(x) for x in d["porous"]])
    _restore_forcing(sim, d)


def _save_multifluid(sim, d):
    _save_forcing(sim, d)
    # the tables as rows of float64 (exact for the int32 and float32 they hold)
    d["interactions"] = np.array(sim.interactions, np.float64).reshape(len(sim.interactions), 6)
    d["reactions"] = np.array(sim.reactions, np.float64).reshape(len(sim.reactions), 6)


def _restore_multifluid(sim, d):
    _restore_forcing(sim, d)
    inter, react = [tuple(r) for r in d["interactions"]], [tuple(r) for r in d["reactions"]]
    others = [r[0] for r in inter] + [r[1] for r in inter] + [r[1] for r in react] + [r[2] for r in react]
    if not others or max(others) == 0:      # (tables that name further fluids are restored by the set: Shan_Chen_Fluids)
        sim.set_interactions(inter)
        sim.set_reactions(react)


# Only the plain flow kinds have obstacles and candidate kernels to time: every other kind's kernel is the planner's size rule.
KINDS = {k.name: k for k in (
    Kind("opencl", _native.LB_SEM_OPENCL, True, True, _nothing, _nothing),
    Kind("cython", _native.LB_SEM_CYTHON, True, True, _nothing, _nothing),
    Kind("d2q9i", _native.LB_SEM_OPENCL_D2Q9I, True, True, _nothing, _nothing),
    Kind("diffusion", _native.LB_SEM_DIFFUSION, False, False, _save_diffusion, _restore_diffusion),
    Kind("multifield", _native.LB_SEM_MULTIFIELD, False, False, _save_multifield, _restore_multifield),
    Kind("poisson", _native.LB_SEM_POISSON, False, False, _save_poisson, _restore_poisson),
    Kind("porous", _native.LB_SEM_POROUS, False, False, _save_porous, _restore_porous),
    Kind("multifluid", _native.LB_SEM_MULTIFLUID, False, False, _save_multifluid, _restore_multifluid),
    Kind("rocket", _native.LB_SEM_ROCKET, False, False, _nothing, _nothing),
)}
