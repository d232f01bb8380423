"""Forced flow in a porous medium: the surface of the reference's ``LB_D2Q9.porous_media`` on liblbhip
(``single_component.Simulation_Runner``, ``single_component.Pourous_Media``)."""
from .single_component import Pourous_Media, Simulation_Runner  # noqa: F401
