"""The spectral screened-Poisson solver: the surface of the reference's ``LB_D2Q9.spectral_poisson`` on liblbhip
(``screened_poisson.Screened_Poisson``)."""
from .screened_poisson import Screened_Poisson  # noqa: F401
