"""Scalar transport (the reference's ``reaction_diffusion`` package): ``diffusion`` holds the classes."""
