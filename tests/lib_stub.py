"""The stub the wrapper tests put in place of the library: it only CONVERTS what a call path of sparenet_amd._lib hands
it, with the argtypes parsed from the header, and records the calls.  CPU tensors stand in for device tensors."""
import ctypes

import torch


def install(monkeypatch, registries, size_t=4096, record=lambda name, args: (name, args)):
    """Replace the functions of `registries` (names among _calls, _ext_calls, _topic_calls, _op_calls) and the device
    checks of _lib through `monkeypatch`; returns the list the calls are recorded in.  A size_t function (a workspace
    size) returns `size_t`, every other one 0."""
    from sparenet_amd import _lib

    _lib.lib()
    calls = []

    def converting(name, fn):
        def call(*args):
            assert len(args) == len(fn.argtypes), f"{name}: {len(args)} arguments, prototype has {len(fn.argtypes)}"
            for i, (t, a) in enumerate(zip(fn.argtypes, args)):
                try:
                    t.from_param(a)
                except (TypeError, ctypes.ArgumentError) as e:
                    raise AssertionError(f"{name}: argument {i} ({a!r}) does not convert to {t.__name__}: {e}")
            calls.append(record(name, args))
            return size_t if fn.restype is ctypes.c_size_t else 0
        return call

    def stubbed(registry):
        return {n: (converting(n, s[0]),) + s[1:] for n, s in registry.items()}

    for attr in registries:
        registry = getattr(_lib, attr)
        flat = attr in ("_calls", "_ext_calls")      # the other two hold one registry per header
        monkeypatch.setattr(_lib, attr, stubbed(registry) if flat else {k: stubbed(r) for k, r in registry.items()})

    def fake_address(t, dtype, name, host=False):      # _lib._address without the device check
        assert isinstance(t, torch.Tensor), name
        assert dtype is None or t.dtype == dtype, f"{name}: expected {dtype}, got {t.dtype}"
        assert t.is_contiguous(), name
        return t.data_ptr() or 8

    monkeypatch.setattr(_lib, "_address", fake_address)
    monkeypatch.setattr(_lib, "require_device", lambda t, name: None)
    monkeypatch.setattr(_lib, "stream_of", lambda t: ctypes.c_void_p(0))
    return calls


def _scalars(args):
    """A call's arguments without the stream, every pointer reduced to whether it was given."""
    return tuple(a if isinstance(a, (int, float)) and not isinstance(a, bool) and abs(a) < 2 ** 20 else a is not None
                 for a in args[:-1])
