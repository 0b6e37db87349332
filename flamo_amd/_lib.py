"""ctypes binding of libflamo_hip.so.  The C ABI is declared in include/flamo_hip.h (and, for the energy-decay-curve and the
average-power criteria, the FDN attenuation designs, the multi-resolution STFT, the energy-decay-relief and the mel multi-scale spectral criteria,
include/flamo_hip_edc.h, include/flamo_hip_avgpow.h, include/flamo_hip_fdnatt.h, include/flamo_hip_mrstft.h,
include/flamo_hip_edr.h, include/flamo_hip_melmss.h and include/flamo_hip_mss.h, and for the band split of the filter bank include/flamo_hip_filterbank.h), and the restype / argtypes of every entry point are read from those headers at import
(_parse_header): no signature is written a second time here.

The shared library is built in-tree (``flamo_amd/libflamo_hip.so``) by ``build()`` /
``make -C flamo_amd/csrc``.  There is NO fallback: if the library is missing or a tensor is
not on a ROCm device the ops raise -- the product path never routes through torch.fft,
torch.einsum, torch.linalg or any CPU code.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLAMO_HIP_LIB") or os.path.join(_HERE, "libflamo_hip.so")   # override: A/B builds
CSRC = os.path.join(_HERE, "csrc")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip.h")
HEADER_EDC_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip_edc.h")      # the criterion of csrc/edc.hip
HEADER_AVGPOW_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip_avgpow.h")      # ... of csrc/avgpow.hip
HEADER_FDNATT_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip_fdnatt.h")      # the designs of csrc/fdnatt.hip
HEADER_MRSTFT_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip_mrstft.h")      # the criterion of csrc/mrstft.hip
HEADER_EDR_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip_edr.h")      # ... of csrc/edr.hip
HEADER_MELMSS_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip_melmss.h")      # ... of csrc/melmss.hip
HEADER_MSS_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip_mss.h")      # ... of csrc/mss.hip
HEADER_FILTERBANK_PATH = os.path.join(os.path.dirname(_HERE), "include", "flamo_hip_filterbank.h")      # the band split of csrc/filterbank.hip

_lock = threading.Lock()
_lib = None

# C type -> ctypes type, for return values and parameters alike.  Only the pointers the host side reads or writes itself keep
# their element type; every other pointer is a device address, handed over as an integer.
_CTYPES = {
    "int": C.c_int,
    "long": C.c_long,
    "double": C.c_double,
    "size_t": C.c_size_t,
    "unsigned": C.c_uint,
    "int*": C.POINTER(C.c_int),
    "const char*": C.c_char_p,
    "void*": C.c_void_p,
    "const void*": C.c_void_p,
    "int32_t*": C.c_void_p,
    "const int32_t*": C.c_void_p,
}

# RET fl_name(PARAMS); -- a declaration starts where the one before it ended (or behind the brace of extern "C")
_DECL = re.compile(r"(?:\A|(?<=[;{}]))\s*([\w\s*]*?)\b(fl_\w+)\s*\(([^()]*)\)\s*;")


def _parse_header(text: str) -> dict:
    """name -> (restype, argtypes) of every ``RET fl_name(PARAMS);`` in the text of a C header as regular as
    include/flamo_hip.h: one declaration per ``;``, every parameter named, types from _CTYPES only.  Anything else is a
    ValueError that names the function -- a type is never guessed, and a declaration is never passed over."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = text.replace("*", " * ")          # "const void *x" and "const void* x" read alike

    def ctype(name, words):
        key = " ".join(words).replace(" *", "*")
        if key not in _CTYPES:
            raise ValueError(f"{name}: no ctypes type for {key!r}")
        return _CTYPES[key]

    def param(name, p):          # the last word of a parameter is its name; the words before it are its type
        words = p.split()
        if len(words) < 2 or not words[-1].isidentifier():
            raise ValueError(f"{name}: parameter {' '.join(words)!r} is not TYPE NAME")
        return ctype(name, words[:-1])

    sigs = {}
    for ret, name, params in _DECL.findall(text):
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (ctype(name, ret.split()), [param(name, p) for p in params])
    unparsed = set(re.findall(r"\b(fl_\w+)\s*\(", text)) - set(sigs)
    if unparsed:
        raise ValueError("declarations not understood: " + ", ".join(sorted(unparsed)))
    return sigs


def _read_header(path: str = HEADER_PATH) -> dict:
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the ctypes signatures of libflamo_hip.so are read from it.")
    with open(path) as f:
        return _parse_header(f.read())


# name -> (restype, argtypes), in the header's order.  The header is the one place where a signature is written: the compiler
# holds the entry bodies to it (csrc/common.h includes it), and this table is read from it.
_SIGNATURES = _read_header()

EXPORTS = tuple(_SIGNATURES)

# the entries of include/flamo_hip_edc.h, a table of their own: bound by lib() like the others
_SIGNATURES_EDC = _read_header(HEADER_EDC_PATH)

# ... and those of include/flamo_hip_avgpow.h
_SIGNATURES_AVGPOW = _read_header(HEADER_AVGPOW_PATH)

# ... and those of include/flamo_hip_fdnatt.h
_SIGNATURES_FDNATT = _read_header(HEADER_FDNATT_PATH)

# ... and those of include/flamo_hip_mrstft.h
_SIGNATURES_MRSTFT = _read_header(HEADER_MRSTFT_PATH)

# ... and those of include/flamo_hip_edr.h
_SIGNATURES_EDR = _read_header(HEADER_EDR_PATH)

# ... and those of include/flamo_hip_melmss.h
_SIGNATURES_MELMSS = _read_header(HEADER_MELMSS_PATH)

# ... and those of include/flamo_hip_mss.h
_SIGNATURES_MSS = _read_header(HEADER_MSS_PATH)

# ... and those of include/flamo_hip_filterbank.h
_SIGNATURES_FILTERBANK = _read_header(HEADER_FILTERBANK_PATH)


def build(force: bool = False) -> str:
    """Compile every HIP source for gfx950 into flamo_amd/libflamo_hip.so (hipcc cross-compiles
    without a GPU).  Returns the library path."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("building libflamo_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-8000:])
    return LIB_PATH


# A launch pair is open on this thread (ops.paired_launch): a recorded response launch must go out before ANY other library
# call than the column pass that carries it -- every call site fetches the handle through lib(), which is where that is enforced.
# _pair.stream_of / _pair.issued: ops' hooks (the current stream; drop the references that kept the record's buffers alive).
_pair = threading.local()


def lib(pair_ok: bool = False) -> C.CDLL:
    """The loaded library.  Raises (never falls back) when it has not been built.  ``pair_ok``: the caller is the launch that
    carries a recorded one (see ops.paired_launch); every other call flushes it first."""
    global _lib
    if not pair_ok and getattr(_pair, "stream_of", None) is not None and _lib is not None and _lib.fl_launch_pair_pending():
        rc = _lib.fl_launch_pair_flush(_pair.stream_of())
        _lib.fl_launch_pair_begin()
        _pair.issued()
        if rc != 0:
            raise RuntimeError(f"libflamo_hip launch pair flush failed (code {rc}): " + _lib.fl_last_error().decode("utf-8", "replace"))
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise RuntimeError(
                        f"{LIB_PATH} not found: the HIP extension is required (run "
                        "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C flamo_amd/csrc`)."
                    )
                handle = C.CDLL(LIB_PATH)
                for name, (res, args) in (*_SIGNATURES.items(), *_SIGNATURES_EDC.items(), *_SIGNATURES_AVGPOW.items(),
                                           *_SIGNATURES_FDNATT.items(), *_SIGNATURES_MRSTFT.items(), *_SIGNATURES_EDR.items(),
                                           *_SIGNATURES_MELMSS.items(), *_SIGNATURES_MSS.items(),
                                           *_SIGNATURES_FILTERBANK.items()):
                    fn = getattr(handle, name)  # AttributeError if the symbol is missing
                    fn.restype = res
                    fn.argtypes = args
                _lib = handle
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().fl_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libflamo_hip {what} failed (code {rc}): {msg}")
