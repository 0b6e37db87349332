"""Helpers behind the processor classes that are not per-bin kernels themselves (flamo/auxiliary)."""
from .scattering import ScatteringMapping, get_random_shifts, hadamard_matrix  # noqa: F401

# flamo/auxiliary/reverb.py.  Its classes derive from processor.dsp, which imports this package for the scattering helpers: the
# names resolve on first use.
_REVERB = ("HomogeneousFDN", "parallelFDNGEQ", "parallelFDNAccurateGEQ", "parallelFirstOrderShelving", "rt2slope",
           "rt2absorption", "map_gamma", "inverse_map_gamma", "map_gfdn_gamma")


def __getattr__(name):
    if name == "reverb" or name in _REVERB:
        import importlib
        reverb = importlib.import_module(".reverb", __name__)
        return reverb if name == "reverb" else getattr(reverb, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + list(_REVERB) + ["reverb"])
