"""Helpers behind the processor classes that are not per-bin kernels themselves (flamo/auxiliary)."""
from .scattering import ScatteringMapping, get_random_shifts, hadamard_matrix  # noqa: F401

# flamo/auxiliary/reverb.py.  Its classes derive from processor.dsp, which imports this package for the scattering helpers: the
# names resolve on first use.
_REVERB = ("HomogeneousFDN", "parallelFDNGEQ", "parallelFDNAccurateGEQ", "parallelFirstOrderShelving", "rt2slope",
           "rt2absorption", "map_gamma", "inverse_map_gamma", "map_gfdn_gamma")
# flamo/auxiliary/filterbank.py, resolved the same way
_FILTERBANK = ("FilterBank",)
_LAZY = {"reverb": _REVERB, "filterbank": _FILTERBANK}


def __getattr__(name):
    for module, names in _LAZY.items():
        if name == module or name in names:
            import importlib
            mod = importlib.import_module("." + module, __name__)
            return mod if name == module else getattr(mod, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + [n for module, names in _LAZY.items() for n in (module, *names)])
