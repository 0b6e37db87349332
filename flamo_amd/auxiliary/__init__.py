"""Helpers behind the processor classes that are not per-bin kernels themselves (flamo/auxiliary)."""
from .scattering import ScatteringMapping, get_random_shifts, hadamard_matrix  # noqa: F401
