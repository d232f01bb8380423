"""Competing populations advected by an imposed flow (the reference's ``LB_D2Q9.advecting_range_expansion``)."""
