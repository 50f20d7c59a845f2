"""ctypes binding of the ida_* section of librubikhip.so (include/rubikhip.h "Iterative-deepening A*"): Korf's IDA* under the corner
and edge pattern databases -- the frame's first contents and a budgeted search step.

The functions live in the SAME library and the same header as the rc_*, rcc_*, rce_* and rct_* ones, so there is nothing to load
here: ida_lib() takes the library _lib.lib() has loaded (build-id check included) and gives the ida_* entry points their signatures.
A library without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import c_int as i32, c_int64 as i64, c_void_p as vp

import numpy as np

from . import _lib, _native

MAX_DEPTH = 32             # rows of a path, nibbles of a trail
MAX_EDGE_TABLES = 4
NOOP = 12                  # "no move": what the caller prefills path with
INF = 2 ** 31 - 1          # next of an iteration that has dropped nothing yet
SOLVED, EXHAUSTED, ILLEGAL, BAD_FRAME = 1, 2, 4, 8      # IDA_*: the status bits

_TABLES = [vp, i64, i32, vp, vp, vp]                     # corner_table, corner_bytes, n_edge, masks, edge_tables, edge_bytes
_FRAME = [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]   # path, max_depth, path_pitch, floor, limit, trail, cursor, depth, bound, next, nodes, status

# every ida_* function of include/rubikhip.h, once (the format of _lib.SIGNATURES)
IDA_SIGNATURES = {
    "ida_max_steps": ([], i64),
    "ida_canonical": [vp],
    "ida_init": [vp, i64, i64] + _TABLES + _FRAME + [vp],
    "ida_search": [vp, i64, i64] + _TABLES + _FRAME + [i64, vp, vp],
}

# librubikhip.so with the ida_* signatures applied (once)
ida_lib = _native.extension(_lib.lib, IDA_SIGNATURES, "hip")


def max_steps() -> int:
    """ida_max_steps: the largest max_steps one ida_search call takes (no device needed)."""
    return int(ida_lib().ida_max_steps())


def canonical():
    """ida_canonical: bool [13, 13, 12], allowed[p2, p1, m] -- the canonical-move rule as the kernel was compiled with it (12 = no move)."""
    out = np.zeros((13, 13, 12), np.uint8)
    _lib.check(ida_lib().ida_canonical(out.ctypes.data))
    return out.astype(bool)


def prefixes(k):
    """uint8 [count, k]: the canonical sequences of length k in the search's order (12 | 114 | 1068 for k = 1 | 2 | 3; one empty row for 0)."""
    allowed = canonical()
    rows = [()]
    for _ in range(k):
        rows = [r + (m,) for r in rows for m in range(12)
                if allowed[r[-2] if len(r) > 1 else NOOP, r[-1] if r else NOOP, m]]
    return np.array(rows, np.uint8).reshape(len(rows), k)
