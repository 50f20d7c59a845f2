"""ctypes binding of the rcs_* extension of librubiksearch.so (include/rubiksym.h): the cube symmetries on the device.

The extension lives in the SAME library as include/rubiksearch.h's functions, so there is nothing to load here: sym_lib() takes the
library _search_lib.search_lib() has loaded (build-id check included: csrc/rc_sym.h, csrc/rc_sym_tables.h and rubiksym.h are among
its hashed sources) and gives the rcs_* entry points their signatures.  A library without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import c_int as i32, c_int64 as i64, c_void_p as vp

import numpy as np

from . import _native, _search_lib

# every function of include/rubiksym.h, once (the format of _search_lib.SIGNATURES)
SYM_SIGNATURES = {
    "rcs_sym_count": [i32],
    "rcs_sym_tables": [i32, vp, vp, vp, vp, vp],
    "rcs_sym_apply": [vp, vp, i64, i64, i64, i32, vp, i32, vp, vp],
    "rcs_sym_canonical": [vp, i64, i64, i32, vp, vp, i64, vp],
}

# librubiksearch.so with the rcs_* signatures applied (once)
sym_lib = _native.extension(_search_lib.search_lib, SYM_SIGNATURES, "search")


def count(cube_size) -> int:
    """rcs_sym_count: K, the number of symmetries (no device needed)."""
    k = sym_lib().rcs_sym_count(cube_size)
    if k < 0:
        raise NotImplementedError(f"cube_size {cube_size}")
    return k


def tables(cube_size):
    """rcs_sym_tables: the LIBRARY's tables as numpy arrays dict(perm [K, S], relabel [K, 6], amap [K, A + 1], inverse [K],
    compose [K, K]) -- what the kernels were compiled with; tables.get_symmetries is what they were generated from."""
    from .tables import get_tables
    t, K = get_tables(cube_size), count(cube_size)
    out = {"perm": np.zeros((K, t.n_stickers), np.uint8), "relabel": np.zeros((K, 6), np.uint8), "amap": np.zeros((K, t.n_actions + 1), np.uint8),
           "inverse": np.zeros(K, np.uint8), "compose": np.zeros((K, K), np.uint8)}
    _search_lib.check(sym_lib().rcs_sym_tables(cube_size, *(a.ctypes.data for a in out.values())))
    return out
