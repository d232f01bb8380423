"""Multicomponent, multiphase Shan-Chen fluids: the surface of the reference's ``LB_D2Q9.multicomponent_multiphase`` on
liblbhip (``multi.Simulation_Runner``, ``multi.Fluid``)."""
from .multi import Fluid, Simulation_Runner, Simulation_RunnerD2Q25  # noqa: F401
