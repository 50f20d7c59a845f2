"""ctypes binding of the rcp_* extension of librubiksearch.so (include/rubiksearch.h "Corner pattern database"): the exact distance
table over the corner states -- build, unrank, look up, score.

The extension lives in the SAME library and the same header as the rc_search_* and rca_* functions, so there is nothing to load here:
pattern_lib() takes the library _search_lib.search_lib() has loaded (build-id check included) and gives the rcp_* entry points their
signatures.  A library without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import c_float as f32, c_int as i32, c_int64 as i64, c_void_p as vp

import numpy as np

from . import _native, _search_lib

# every rcp_* function of include/rubiksearch.h, once (the format of _search_lib.SIGNATURES)
PATTERN_SIGNATURES = {
    "rcp_table_bytes": ([i32], i64),
    "rcp_tables": [i32, vp, vp],
    "rcp_build_begin": [vp, i64, i32, vp],
    "rcp_build_level": [vp, i64, i32, i32, vp, vp],
    "rcp_unrank": [vp, i64, i32, vp, i64, vp, vp],
    "rcp_lookup": [vp, i64, i64, i32, vp, i64, vp, vp],
    "rcp_score_keys": [vp, i64, i32, i64, i32, vp, i64, vp, vp],
    "rcp_relax": [i64, i32, i32, i64, i64, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp],
}

# librubiksearch.so with the rcp_* signatures applied (once)
pattern_lib = _native.extension(_search_lib.search_lib, PATTERN_SIGNATURES, "search")


def table_bytes(cube_size) -> int:
    """rcp_table_bytes: N, the number of corner states = the bytes of a table (no device needed)."""
    n = pattern_lib().rcp_table_bytes(cube_size)
    if n < 0:
        raise NotImplementedError(f"cube_size {cube_size}")
    return int(n)


def tables(cube_size):
    """rcp_tables: the LIBRARY's move tables (src, twist), uint8 [A, NC] each -- what the kernels were compiled with;
    tables.get_corner_moves is what they were generated from."""
    from .tables import get_cubies, get_tables
    if cube_size not in (2, 3):
        raise NotImplementedError(f"cube_size {cube_size}")
    shape = (get_tables(cube_size).n_actions, get_cubies(cube_size).nc)
    src, twist = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    _search_lib.check(pattern_lib().rcp_tables(cube_size, src.ctypes.data, twist.ctypes.data))
    return src, twist
