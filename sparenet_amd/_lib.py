"""ctypes binding of libsparenet_hip.so (the C ABI declared in include/sparenet_hip.h and, for the operators added
after the reference's own, in include/sparenet_hip_ext.h).

A header is the single description of a call: `prototypes()` parses it, `lib()` derives the ctypes signatures and
one prepared parameter list per function from that parse, and `call()` / `workspace()` are the one path on which
Python values become C arguments -- checked against the declared pointee type, under the declared parameter name.
`ext_call()` / `ext_workspace()` are the same path for the functions of the extension header, which are bound into a
registry of their own: the main header's function list is pinned by the test suite, so new entry points are declared
in the second header and reached by these two names.  That header's list is pinned in turn, so a later group of entry
points has a header of its own, include/sparenet_hip_ext_<topic>.h: `lib()` binds each of them into a registry per
topic, and `topic_call(topic, name, ...)` is the same path for those.  The set of topic headers is pinned as well, so an
operator added after them declares its entry points in include/ops/<name>.h: `lib()` binds every header of that
directory into a registry per file name, `op_call(name_of_header, name, ...)` / `op_workspace(...)` are the same path
for those, and the next operator adds a header there and nothing here.

There is deliberately NO fallback: if the HIP library or its header is missing, or a tensor is not a contiguous
CUDA(ROCm) tensor of the declared dtype, these helpers raise.  PyTorch is used only for device memory and streams.
"""
import collections
import ctypes
import glob
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsparenet_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sparenet_hip.h")
EXT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sparenet_hip_ext.h")
_lib = None
_calls = {}     # name -> (ctypes function, prepared parameters, has a trailing stream, int result is a status code)
_ext_calls = {}     # the same for the functions of the extension header
_topic_calls = {}   # topic -> the same for the functions of include/sparenet_hip_ext_<topic>.h
_op_calls = {}      # stem -> the same for the functions of include/ops/<stem>.h

SN_EINVAL = -22


class SparenetHipError(RuntimeError):
    pass


# The C ABI this Python side was written against (include/sparenet_hip.h: SN_ABI_VERSION).  The library is built
# separately and is not tracked: a stale .so next to newer Python (or the reverse) would make ctypes pass shifted
# arguments -- memory corruption instead of an error -- so lib() refuses any other version.
EXPECTED_ABI = 4

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double}
# pointee type -> (dtype a tensor must have, element type a host ctypes array must have); void takes any tensor
_POINTEES = {"float": (torch.float32, ctypes.c_float), "int": (torch.int32, ctypes.c_int),
             "double": (torch.float64, ctypes.c_double), "long long": (torch.int64, ctypes.c_longlong),
             "unsigned": (torch.int32, ctypes.c_uint), "void": (None, None), "char": (None, ctypes.c_char)}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong, "void": None,
            "const char *": ctypes.c_char_p}

Param = collections.namedtuple("Param", "name ctype pointer const")     # `const float *xyz1`: xyz1, float, True, True
Workspace = collections.namedtuple("Workspace", "tensor nbytes")        # a uint8 tensor and its size export's answer

_POINTER, _WORKSPACE, _INTEGER, _REAL, _TEXT = range(5)


def prototypes(path=None):
    """{name: (return type, [Param, ...])} of every function include/sparenet_hip.h declares."""
    txt = re.sub(r"/\*.*?\*/", "", open(path or HEADER_PATH).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^(int|size_t|void|long long|const char \*)\s*(sn_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt,
                         re.M | re.S):
        args = m.group(3).strip()
        params = []
        for a in ([] if args in ("", "void") else args.split(",")):
            p = re.fullmatch(r"(const )?([a-z_ ]+?) ?(\*)? ?(\w+)", " ".join(a.split()))
            params.append(Param(p.group(4), p.group(2), bool(p.group(3)), bool(p.group(1))))
        out[m.group(2)] = (m.group(1), params)
    return out


def topic_headers():
    """{topic: path} of every include/sparenet_hip_ext_<topic>.h next to the main header."""
    paths = sorted(glob.glob(os.path.join(os.path.dirname(HEADER_PATH), "sparenet_hip_ext_*.h")))
    return {os.path.basename(p)[len("sparenet_hip_ext_"):-2]: p for p in paths}


def op_headers():
    """{stem: path} of every include/ops/<stem>.h: one header per operator added after the pinned ones."""
    paths = sorted(glob.glob(os.path.join(os.path.dirname(HEADER_PATH), "ops", "*.h")))
    return {os.path.basename(p)[:-2]: p for p in paths}


def _prepare(params):
    """The parameters `call` takes for a declared parameter list, as (kind, name, dtype, element type) -- without the
    trailing `void *stream`, and with `void *workspace, size_t workspace_bytes` as one -- and whether there is a stream."""
    has_stream = bool(params) and params[-1] == Param("stream", "void", True, False)
    steps = []
    for i, p in enumerate(params[:len(params) - has_stream]):
        if p.pointer and p.ctype == "char":
            steps.append((_TEXT, p.name, None, None))
        elif p.pointer:
            sized = p.name == "workspace" and params[i + 1:i + 2] == [Param("workspace_bytes", "size_t", False, False)]
            steps.append((_WORKSPACE if sized else _POINTER, p.name) + _POINTEES[p.ctype])
        elif steps and steps[-1][0] == _WORKSPACE and p.name == "workspace_bytes":
            continue
        else:
            steps.append((_REAL if p.ctype in ("float", "double") else _INTEGER, p.name, None, _SCALARS[p.ctype]))
    return steps, has_stream


def lib():
    """Load (once) and return the HIP library; raises if it is not built, was built for another ABI, or the header
    that describes its calls is not next to the package."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise SparenetHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` or `make -C sparenet_amd/csrc`. sparenet_amd has no CPU fallback.")
        for header in (HEADER_PATH, EXT_HEADER_PATH):
            if not os.path.isfile(header):
                raise SparenetHipError(
                    f"{header} not found: the header is the description of every call into {LIB_PATH} (argument "
                    "types, names and counts); the library is not loaded without it.")
        L = ctypes.CDLL(LIB_PATH)
        got = L.sn_abi_version()
        if got != EXPECTED_ABI:
            raise SparenetHipError(
                f"{LIB_PATH} implements C ABI version {got}, this Python side needs {EXPECTED_ABI}: rebuild the "
                "library (`make -C sparenet_amd/csrc`)")
        _topic_calls.clear()
        topics = [(_topic_calls.setdefault(topic, {}), header) for topic, header in topic_headers().items()]
        _op_calls.clear()
        ops = [(_op_calls.setdefault(stem, {}), header) for stem, header in op_headers().items()]
        for registry, header in [(_calls, HEADER_PATH), (_ext_calls, EXT_HEADER_PATH)] + topics + ops:
            registry.clear()
            for name, (ret, params) in prototypes(header).items():
                fn = getattr(L, name, None)
                if fn is None:          # a missing export is test_abi's finding, not a load-time failure
                    continue
                fn.restype = _RETURNS[ret]
                fn.argtypes = [(ctypes.c_char_p if p.ctype == "char" else ctypes.c_void_p) if p.pointer
                               else _SCALARS[p.ctype] for p in params]
                # an int function WITH parameters returns a status code; one without (sn_wait_policy, sn_emd_mode,
                # sn_device_status ...) is a query whose number goes back to the caller
                registry[name] = (fn,) + _prepare(params) + (ret == "int" and bool(params),)
        _lib = L
    return _lib


def signature(name):
    """Names of the arguments `call(name, ...)` (or `ext_call(name, ...)`, `topic_call(topic, name, ...)`,
    `op_call(stem, name, ...)`) takes, in order."""
    lib()
    for registry in [_calls, _ext_calls] + list(_topic_calls.values()) + list(_op_calls.values()):
        if name in registry:
            return [step[1] for step in registry[name][1]]
    raise KeyError(name)


def check(code, what):
    if code != 0:
        msg = lib().sn_last_error().decode("utf-8", "replace")
        raise SparenetHipError(f"{what} failed (code {code}): {msg}")


def device_check(what="sparenet_amd"):
    """Raise if a bounded wait inside an EARLIER multi-workgroup launch on the current device gave up (the persistent EMD
    auction's team barriers, the density sampler's teams; that call's outputs are NaN / -1).  Reads one word of pinned
    host memory (sn_device_status): no synchronisation -- meaningful for work that has FINISHED, so the wrappers call
    it on entry (an earlier step's failure surfaces at the next op) and `loss_item` calls it where the host has just
    waited for the loss."""
    check(call("sn_device_status"), what)


def _address(t, dtype, name, host=False):
    """Address of a contiguous tensor on the expected side (device, or host for the Chamfer host entry points) and of
    the expected dtype (None: any)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.is_cuda == host:
        if host:
            raise SparenetHipError(f"{name}: expected a CPU tensor, got device {t.device}")
        raise SparenetHipError(
            f"{name}: expected a CUDA (ROCm) tensor, got device {t.device}. sparenet_amd runs on "
            "MI355X only; there is no CPU path for this op (the reference has none either; only ChamferDistance "
            "accepts CPU tensors, as in the reference).")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t.data_ptr()


def require_device(t, name):
    """Refuse a CPU tensor (or a non-tensor) with the message of a device entry point, before a wrapper uploads or
    allocates anything for it."""
    _address(t, None, name)


def call(name, *args, host=False):
    """Call the declared function `name`.  `args` are its parameters in the header's order, without the trailing
    `void *stream` (the current stream of the tensors' device is passed) and with ONE value -- a `workspace()` or
    None -- for `void *workspace, size_t workspace_bytes`.  Per declared type: a typed pointer takes a contiguous
    device tensor of that dtype (`host=True`: a CPU tensor, and no stream), None (a null pointer; the library says
    where that is allowed) or a host ctypes array of that element type; integers must be integral.  All device tensors
    must share one device, and the call runs under it.  A status code goes through check(); size_t / long long
    functions and parameterless queries return their number."""
    return _invoke(_calls, HEADER_PATH, name, args, host)


def ext_call(name, *args, host=False):
    """`call` for a function declared in include/sparenet_hip_ext.h: the same conversion, checks and result."""
    return _invoke(_ext_calls, EXT_HEADER_PATH, name, args, host)


def topic_call(topic, name, *args, host=False):
    """`call` for a function declared in include/sparenet_hip_ext_<topic>.h: the same conversion, checks and result."""
    if topic not in _topic_calls:
        lib()
        if topic not in _topic_calls:
            raise SparenetHipError(f"no header include/sparenet_hip_ext_{topic}.h next to {HEADER_PATH}")
    header = os.path.join(os.path.dirname(HEADER_PATH), f"sparenet_hip_ext_{topic}.h")
    return _invoke(_topic_calls[topic], header, name, args, host)


def _op_registry(stem):
    """(registry, header path) of include/ops/<stem>.h."""
    if stem not in _op_calls:
        lib()
        if stem not in _op_calls:
            raise SparenetHipError(f"no header include/ops/{stem}.h next to {HEADER_PATH}")
    return _op_calls[stem], os.path.join(os.path.dirname(HEADER_PATH), "ops", f"{stem}.h")


def op_call(stem, name, *args, host=False):
    """`call` for a function declared in include/ops/<stem>.h: the same conversion, checks and result."""
    registry, header = _op_registry(stem)
    return _invoke(registry, header, name, args, host)


def _invoke(registry, header, name, args, host):
    """The body of call / ext_call: `registry` holds what lib() prepared from `header`."""
    spec = registry.get(name)
    if spec is None:
        lib()
        spec = registry.get(name)
        if spec is None:
            raise SparenetHipError(f"{name} is not declared in {header} or not exported by {LIB_PATH}")
    fn, steps, has_stream, is_status = spec
    if len(args) != len(steps):
        raise TypeError(f"{name} takes {len(steps)} arguments ({', '.join(s[1] for s in steps)}), got {len(args)}")
    c = []
    first = dev = None      # the first device tensor (it decides device and stream) and its device index
    for (kind, pname, dtype, ctype), v in zip(steps, args):
        if kind == _INTEGER:
            i = int(v)
            if i != v:
                raise TypeError(f"{name}: {pname} must be an integer, got {v!r}")
            c.append(i)
        elif kind == _REAL:
            c.append(float(v))
        elif kind == _TEXT:
            c.append(v)
        else:
            if kind == _WORKSPACE and v is not None:
                if not isinstance(v, Workspace):
                    raise TypeError(f"{name}: {pname} takes a workspace() or None")
                v, nbytes = v
            # the accepted tensor first and inline (this loop is the host cost of every op); _address has the refusals
            if (isinstance(v, torch.Tensor) and v.is_cuda != host and (dtype is None or v.dtype == dtype)
                    and v.is_contiguous()):
                c.append(v.data_ptr())
                if not host:
                    if first is None:
                        first, dev = v, v.get_device()
                    elif v.get_device() != dev:
                        raise ValueError(f"{name}: {pname} is on {v.device}, earlier tensor arguments on "
                                         f"{first.device}")
            elif v is None:
                c.append(None)
            elif isinstance(v, ctypes.Array):
                if v._type_ is not ctype:
                    raise TypeError(f"{name}: {pname} expected a host array of {ctype.__name__}, "
                                    f"got {v._type_.__name__}")
                c.append(v)
            else:
                c.append(_address(v, dtype, pname, host))      # raises: which check failed, in its documented order
            if kind == _WORKSPACE:
                c.append(0 if v is None else nbytes)
    if first is None:
        if has_stream:
            c.append(None)
        result = fn(*c)
    else:
        with torch.cuda.device_of(first):
            if has_stream:
                c.append(stream_of(first))
            result = fn(*c)
    if is_status:
        return check(result, name) if result else None
    return result


def workspace(size_export, like, *shape):
    """The scratch buffer of an op: `size_export(*shape)` is asked under `like`'s device (some layouts depend on its
    compute-unit count), and a uint8 tensor of that size -- at least one byte, so that it has an address -- is
    allocated there.  `call` passes the exported size, not the tensor's."""
    return _sized(call, size_export, like, shape)


def ext_workspace(size_export, like, *shape):
    """`workspace` for a size export declared in include/sparenet_hip_ext.h."""
    return _sized(ext_call, size_export, like, shape)


def op_workspace(stem, size_export, like, *shape):
    """`workspace` for a size export declared in include/ops/<stem>.h."""
    return _sized(lambda name, *dims: op_call(stem, name, *dims), size_export, like, shape)


def _sized(ask, size_export, like, shape):
    with torch.cuda.device_of(like):
        nbytes = ask(size_export, *shape)
        return Workspace(torch.empty(max(nbytes, 1), dtype=torch.uint8, device=like.device), nbytes)


def ptr(t, dtype, name, host=False):
    """Device (host=True: host) pointer of a contiguous tensor (validated)."""
    return ctypes.c_void_p(_address(t, dtype, name, host))


def hptr(t, dtype, name):
    """HOST pointer of a contiguous CPU tensor (validated) -- only the Chamfer host entry points take these."""
    return ptr(t, dtype, name, host=True)


def fptr(t, name):
    return ptr(t, torch.float32, name)


def iptr(t, name):
    return ptr(t, torch.int32, name)


def dptr(t, name):
    return ptr(t, torch.float64, name)


def stream_of(t):
    """Current HIP stream of the tensor's device, as void*."""
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def cfloat(x):
    return ctypes.c_float(float(x))
