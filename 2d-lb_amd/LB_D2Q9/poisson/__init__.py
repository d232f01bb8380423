"""The LB Poisson solver: the surface of the reference's ``LB_D2Q9.poisson`` on liblbhip (``solver.Poisson_Solver``)."""
from .solver import Poisson_Solver, poisson_parameters  # noqa: F401
