"""The one loader of the native libraries described in _build.LIBRARIES: path, build-id check, signatures, cache.  No torch import
at module level: the tree library loads without it."""
from __future__ import annotations

import ctypes
import os
import threading

from . import _build

_lock = threading.Lock()
_loaded = {}


class RubikHipError(RuntimeError):
    pass


def path(name) -> str:
    """Where library `name` is loaded from: its override variable (A/B builds in experiments, sanitizer builds), else next to the package."""
    spec = _build.LIBRARIES[name]
    return os.environ.get(spec.env) or spec.built


def signature(sig):
    """(argtypes, restype) of one signature-table entry: a list of argument types (the result is a C int) or (argtypes, restype)."""
    return sig if isinstance(sig, tuple) else (sig, ctypes.c_int)


def declare(L, signatures):
    """Give every entry point of a CDLL its signature.  signatures: {function name: entry}, one entry per function the header declares."""
    for fn, sig in signatures.items():
        f = getattr(L, fn)
        f.argtypes, f.restype = signature(sig)


def load(name, signatures):
    """The loaded library `name` (loads on first use).  There is NO fallback: a missing library, or one built from other sources than
    the tree's, raises."""
    if name not in _loaded:
        with _lock:
            if name not in _loaded:
                spec, p = _build.LIBRARIES[name], path(name)
                if not os.path.exists(p):
                    raise RubikHipError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                                        + (" (hipcc --offload-arch=gfx950). There is no CPU fallback." if spec.gpu else ""))
                if spec.gpu:
                    import torch  # noqa: F401  -- before the library, so that both share one HIP runtime (libamdhip64.so.7)
                L = ctypes.CDLL(p)
                if not hasattr(L, spec.id_symbol):
                    raise RubikHipError(f"{p} predates {spec.id_symbol}: rebuild it with __graft_entry__.build()")
                declare(L, signatures)
                try:                                             # the binary must be the tree's sources (RC_ALLOW_STALE=1: A/B experiments)
                    _build.check_loaded(p, build_id(name, L), spec.sources)
                except RuntimeError as e:
                    raise RubikHipError(str(e)) from None
                _loaded[name] = L
    return _loaded[name]


def extension(base_loader, signatures, name):
    """The loader of an extension of library `name`: further entry points of the SAME binary, declared in a header of their own.
    Calling it takes the library base_loader() has loaded (build-id check included), gives the functions of `signatures` their
    signatures, once, and returns that one CDLL object every time.  A library without them is an error, as everywhere else."""
    lock, declared = threading.Lock(), []

    def loader():
        if not declared:
            with lock:
                if not declared:
                    L = base_loader()
                    missing = [fn for fn in signatures if not hasattr(L, fn)]
                    if missing:
                        raise RubikHipError(f"{path(name)} has no {', '.join(missing)}: rebuild it with __graft_entry__.build()")
                    declare(L, signatures)
                    declared.append(L)
        return declared[0]
    return loader


def build_id(name, L) -> str:
    """The source hash the loaded library L was built from."""
    return getattr(L, _build.LIBRARIES[name].id_symbol)().decode()


def error(name, L, rc) -> RubikHipError:
    """The exception for a non-zero return code of library `name`, with the library's own last-error text."""
    spec = _build.LIBRARIES[name]
    return RubikHipError(f"{spec.file[:-3]} error {rc}: {getattr(L, spec.error_symbol)().decode()}")
