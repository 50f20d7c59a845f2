"""ctypes binding of the rca_* entry points of librubiksearch.so (include/rubiksearch.h "Batch-weighted A*"): the node pool, pop and
merge kernels of search.astar_search.

They live in the SAME library as the beam's functions, so there is nothing to load here: astar_lib() takes the library
_search_lib.search_lib() has loaded (build-id check included) and gives the rca_* entry points their signatures, as _sym_lib does
for rcs_*.  A library without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import c_float as f32, c_int as i32, c_int64 as i64, c_void_p as vp

from . import _native, _search_lib

OPEN, CLOSED, NEW = 1, 2, 8
# every rca_* function of include/rubiksearch.h, once (the format of _search_lib.SIGNATURES)
ASTAR_SIGNATURES = {
    "rca_workspace_bytes": ([i32, i64, i64], i64),
    "rca_init": [vp, i64, i64, i32, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp],
    "rca_pop": [i64, i32, i32, i64, i64, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp, vp],
    "rca_merge": [i64, i32, i32, i64, i64, i64, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64,
                  vp, i64, vp],
    "rca_backtrack": [i64, i32, i64, vp, vp, vp, vp, vp, i32, vp],
}

# librubiksearch.so with the rca_* signatures applied (once)
astar_lib = _native.extension(_search_lib.search_lib, ASTAR_SIGNATURES, "search")


def workspace_bytes(cube_size, n_problems, capacity) -> int:
    """rca_workspace_bytes: bytes of the persistent table (no device needed); -1 for bad arguments."""
    return int(astar_lib().rca_workspace_bytes(int(cube_size), int(n_problems), int(capacity)))
