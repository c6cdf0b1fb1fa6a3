"""ctypes binding of the C-ABI library `libodil_hip.so`, derived from its header include/odil_hip.h.

The header is the one text the binding follows: `declarations` parses its prototypes and `load` gives every exported
function the return and argument types found there.  A new entry point needs nothing in this file.

The library is the product's only compute path.  There is no CPU fallback: if the
shared object is missing, or a call is made with tensors that are not on a HIP
device, the call raises.
"""

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ODIL_HIP_LIB") or os.path.join(_HERE, "libodil_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "odil_hip.h")

# The subset of C that the header is written in.  Pointers are spelled with one space around every `*` here, as
# `declarations` normalises them.
_SCALARS = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "size_t": c_size_t, "double": c_double,
            "float": c_float}
_RETURNS = {"int": c_int, "int64_t": c_int64, "size_t": c_size_t, "const char *": c_char_p}
_PROTOTYPE = re.compile(r"(.+?) (odil_\w+) \( (.*?) ?\)")
_PARAMETER = re.compile(r"(const )?(void|char|{})( \*( const \*)?)? (?!const$)[A-Za-z_]\w*".format("|".join(_SCALARS)))


def declarations(text):
    """{name: (restype, [argtypes])} of every prototype in the text of a header like include/odil_hip.h, in its order.
    Scalars map to the ctypes type of the same width, `const char*` to c_char_p, every other pointer to c_void_p (the C
    type does not tell a host array from a device pointer).  Anything that is not a comment, a preprocessor line, the
    `extern "C"` wrapper or a prototype of the header's subset of C raises ValueError: nothing is skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'^[ \t]*(#.*|extern\s+"C"\s*\{|\})[ \t]*$', " ", text, flags=re.M)
    *statements, rest = text.replace("*", " * ").replace("(", " ( ").replace(")", " ) ").split(";")
    if rest.strip():
        raise ValueError("C-ABI header: text after the last prototype: {!r}".format(rest.strip()))
    found = dict()
    for statement in statements:
        statement = " ".join(statement.split())
        match = _PROTOTYPE.fullmatch(statement)
        if match is None or match.group(1) not in _RETURNS or match.group(2) in found:
            raise ValueError("C-ABI header: not a prototype the binding understands: {!r}".format(statement))
        parameters = [] if match.group(3) in ("", "void") else match.group(3).split(",")
        argtypes = [_argtype(parameter.strip()) for parameter in parameters]
        if None in argtypes:
            raise ValueError("C-ABI header: parameter {!r} not understood in: {!r}".format(
                parameters[argtypes.index(None)].strip(), statement))
        found[match.group(2)] = (_RETURNS[match.group(1)], argtypes)
    return found


def _argtype(parameter):
    """The ctypes type of `T name`, `[const] T * name` or `[const] T * const * name`; None for anything else."""
    form = _PARAMETER.fullmatch(parameter)
    const, base, pointer = form.group(1, 2, 3) if form else (None, None, None)
    if pointer:
        return c_char_p if (const, base, pointer) == ("const ", "char", " *") else c_void_p
    return None if const else _SCALARS.get(base)


_lib = None
_declared = None  # declarations(the header), read once


class OdilHipError(RuntimeError):
    pass


def _header_declarations():
    global _declared
    if _declared is None:
        if not os.path.exists(HEADER_PATH):
            raise OdilHipError(
                "C-ABI header {} is missing: the binding of libodil_hip.so is derived from it.".format(HEADER_PATH))
        with open(HEADER_PATH) as f:
            _declared = declarations(f.read())
    return _declared


def __getattr__(name):
    if name == "EXPORTED":  # every entry point the header declares, hence the library exports
        return list(_header_declarations())
    raise AttributeError("module {!r} has no attribute {!r}".format(__name__, name))


def load():
    """Loads the shared library (once) and types its functions as the header declares them.  Raises if it has not been
    built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OdilHipError(
            "HIP extension not built: {} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C odil_amd/csrc`. There is no CPU fallback.".format(LIB_PATH)
        )
    declared = _header_declarations()
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in declared.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def suffix_of(dtype):
    if dtype == torch.float64:
        return "f64"
    if dtype == torch.float32:
        return "f32"
    raise TypeError("unsupported dtype {} (float32 / float64 only)".format(dtype))


def call(name, dtype, *args, unserved_ok=False):
    """Calls odil_<name>_<f32|f64>(*args); raises OdilHipError on a non-zero status.  unserved_ok: the entry point may
    return 1 = "layout not served, nothing launched" (odil_interp_add_ld / _adj_ld); returns whether it served."""
    fn = _entry.get((name, dtype))
    if fn is None:
        fn = _entry[(name, dtype)] = getattr(load(), "odil_{}_{}".format(name, suffix_of(dtype)))
    status = fn(*args)
    if status == 1 and unserved_ok:
        return False
    if status != 0:
        raise OdilHipError("odil_{}: {} (status {})".format(name, load().odil_last_error().decode(), status))
    return True


_entry = dict()  # (name, dtype) -> the bound entry point (a launch is a few microseconds of host time: no lookups per call)


def ptr(t):
    """Device pointer of a tensor (or None)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError("expected a torch.Tensor, got {}".format(type(t).__name__))
    if not t.is_cuda:
        raise OdilHipError("tensor is on '{}': the HIP kernels need device memory (no CPU fallback)".format(t.device))
    if not t.is_contiguous():
        raise OdilHipError("tensor must be contiguous (C order)")
    return c_void_p(t.data_ptr())


def i64(values):
    values = [int(v) for v in values]
    return (c_int64 * len(values))(*values)


def ptr_array(tensors):
    """HOST array of device pointers."""
    arr = (c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
        if t is not None and (not t.is_cuda or not t.is_contiguous()):
            raise OdilHipError("level arrays must be contiguous device tensors")
    return arr


def host_reals(values, dtype):
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    arr = np.ascontiguousarray(np.asarray(values, dtype=np_dtype))
    return arr, arr.ctypes.data_as(c_void_p)


def stream_ptr():
    """The current HIP stream of the current device as a pointer argument.  (torch.cuda.current_stream() builds a Stream
    object through several Python layers, ~8 us per call -- more than the launch it precedes costs; the raw handle is one
    C call.)"""
    return c_void_p(_raw_stream(_current_device()))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_current_device = getattr(torch._C, "_cuda_getDevice", None)
if _raw_stream is None or _current_device is None:  # (another torch build: the documented route)
    def stream_ptr():  # noqa: F811
        return c_void_p(torch.cuda.current_stream().cuda_stream)


def reduce_workspace_elems():
    return load().odil_reduce_workspace_bytes() // 8
