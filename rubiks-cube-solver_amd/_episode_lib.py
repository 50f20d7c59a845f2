"""ctypes binding of the rcx_* extension of librubikhip.so (include/rubikepisode.h): episode bookkeeping and the masked re-scramble.

The extension lives in the SAME library as include/rubikhip.h's functions, so there is nothing to load here: episode_lib() takes
the library _lib.lib() has loaded (build-id check included: csrc/rc_episode.h and rubikepisode.h are among its hashed sources) and
gives the rcx_* entry points their signatures.  A library without them is an error, as everywhere else."""
from __future__ import annotations

import threading
from ctypes import c_char_p, c_int as i32, c_int64 as i64, c_uint64 as u64, c_void_p as vp

from . import _lib, _native
from ._native import RubikHipError

# every function of include/rubikepisode.h, once (the format of _lib.SIGNATURES)
EPISODE_SIGNATURES = {
    "rcx_episode_end": [vp, i64, i64, i32, vp, vp, i32, vp, i32, i32, u64, u64, i64, i64, vp, vp, vp],
    "rcx_episode_build_tag": ([], c_char_p),
}

_lock = threading.Lock()
_declared = None


def episode_lib():
    """librubikhip.so with the rcx_* signatures applied (once)."""
    global _declared
    if _declared is None:
        with _lock:
            if _declared is None:
                L = _lib.lib()
                missing = [fn for fn in EPISODE_SIGNATURES if not hasattr(L, fn)]
                if missing:
                    raise RubikHipError(f"{_lib.LIB_PATH} has no {', '.join(missing)}: rebuild it with __graft_entry__.build()")
                _native.declare(L, EPISODE_SIGNATURES)
                _declared = L
    return _declared


def build_tag() -> str:
    """rcx_episode_build_tag(): the library's build id, reported through the extension."""
    return episode_lib().rcx_episode_build_tag().decode()
