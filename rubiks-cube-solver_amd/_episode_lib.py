"""ctypes binding of the rcx_* extension of librubikhip.so (include/rubikepisode.h): episode bookkeeping and the masked re-scramble.

The extension lives in the SAME library as include/rubikhip.h's functions, so there is nothing to load here: episode_lib() takes
the library _lib.lib() has loaded (build-id check included: csrc/rc_episode.h and rubikepisode.h are among its hashed sources) and
gives the rcx_* entry points their signatures.  A library without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import c_char_p, c_int as i32, c_int64 as i64, c_uint64 as u64, c_void_p as vp

from . import _lib, _native

# every function of include/rubikepisode.h, once (the format of _lib.SIGNATURES)
EPISODE_SIGNATURES = {
    "rcx_episode_end": [vp, i64, i64, i32, vp, vp, i32, vp, i32, i32, u64, u64, i64, i64, vp, vp, vp],
    "rcx_episode_build_tag": ([], c_char_p),
}

# librubikhip.so with the rcx_* signatures applied (once)
episode_lib = _native.extension(_lib.lib, EPISODE_SIGNATURES, "hip")


def build_tag() -> str:
    """rcx_episode_build_tag(): the library's build id, reported through the extension."""
    return episode_lib().rcx_episode_build_tag().decode()
