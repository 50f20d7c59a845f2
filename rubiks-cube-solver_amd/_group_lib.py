"""ctypes binding of the cg_* section of librubikhip.so (include/rubikhip.h "Cube group"): product and inverse of whole cubes,
uniformly random cubes, and the inverse of an action list.

The functions live in the SAME library and the same header as the rc_*, rcc_*, rce_*, rct_*, ida_* and tp_* ones, so there is nothing
to load here: group_lib() takes the library _lib.lib() has loaded (build-id check included) and gives the cg_* entry points their
signatures.  A library without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import c_int as i32, c_int64 as i64, c_uint64 as u64, c_void_p as vp

from . import _lib, _native

# every cg_* function of include/rubikhip.h, once (the format of _lib.SIGNATURES)
GROUP_SIGNATURES = {
    "cg_product": [vp, i64, vp, i64, i64, i32, vp, i64, vp, vp],
    "cg_inverse": [vp, i64, i64, i32, vp, i64, vp, vp],
    "cg_random": [u64, u64, i64, i64, i32, vp, i64, vp],
    "cg_invert_actions": [vp, i64, i64, i64, i32, vp, i64, vp, vp],
}

# librubikhip.so with the cg_* signatures applied (once)
group_lib = _native.extension(_lib.lib, GROUP_SIGNATURES, "hip")
