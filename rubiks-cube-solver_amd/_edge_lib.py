"""ctypes binding of the rce_* section of librubikhip.so (include/rubikhip.h "Edge pattern databases"): exact distance tables over
up to 7 of the 12 edge pieces of the 3x3x3 -- build, unrank, look up, score.

The functions live in the SAME library and the same header as the rc_* and rcc_* ones, so there is nothing to load here: edge_lib()
takes the library _lib.lib() has loaded (build-id check included) and gives the rce_* entry points their signatures.  A library
without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import c_int as i32, c_int64 as i64, c_void_p as vp

import numpy as np

from . import _lib, _native

MAX_TRACKED = 7        # k, the pieces of one table: N(7) = 510 935 040 is the last count below 2^32
N_EDGES = 12

# every rce_* function of include/rubikhip.h, once (the format of _lib.SIGNATURES)
EDGE_SIGNATURES = {
    "rce_table_bytes": ([i32], i64),
    "rce_home_index": ([i32], i64),
    "rce_tables": [vp, vp],
    "rce_build_begin": [vp, i64, i32, vp],
    "rce_build_level": [vp, i64, i32, i32, vp, vp],
    "rce_unrank": [vp, i64, i32, vp, i64, vp, vp],
    "rce_lookup": [vp, i64, i64, i32, vp, i64, vp, vp],
    "rce_score_codes": [vp, i64, i32, i64, i32, vp, i64, vp, i32, vp],
}

# librubikhip.so with the rce_* signatures applied (once)
edge_lib = _native.extension(_lib.lib, EDGE_SIGNATURES, "hip")


def edge_mask(edges) -> int:
    """The 12-bit mask of `edges`: a mask (int) or an iterable of piece numbers.  ValueError unless it names 1..7 of the pieces 0..11."""
    if isinstance(edges, (int, np.integer)) and not isinstance(edges, bool):
        mask = int(edges)
    else:
        pieces = [int(e) for e in edges]
        if any(not 0 <= e < N_EDGES for e in pieces) or len(set(pieces)) != len(pieces):
            raise ValueError(f"edges must be distinct piece numbers in 0..{N_EDGES - 1}, got {pieces}")
        mask = sum(1 << e for e in pieces)
    if not 0 < mask < 1 << N_EDGES or not 1 <= bin(mask).count("1") <= MAX_TRACKED:
        raise ValueError(f"an edge table tracks 1..{MAX_TRACKED} of the pieces 0..{N_EDGES - 1}, got mask {mask:#x}")
    return mask


def table_bytes(mask) -> int:
    """rce_table_bytes: N(k) = 12!/(12-k)! * 2^k, the number of patterns = the bytes of a table (no device needed)."""
    n = edge_lib().rce_table_bytes(edge_mask(mask))
    assert n > 0
    return int(n)


def home_index(mask) -> int:
    """rce_home_index: the index of the pattern with every tracked piece at home, unflipped -- not 0 in general."""
    return int(edge_lib().rce_home_index(edge_mask(mask)))


def tables():
    """rce_tables: the LIBRARY's move tables (esrc, eflip), uint8 [12, 12] each -- what the kernels were compiled with;
    tables.get_edge_moves is what they were generated from."""
    esrc, eflip = np.zeros((12, N_EDGES), np.uint8), np.zeros((12, N_EDGES), np.uint8)
    _lib.check(edge_lib().rce_tables(esrc.ctypes.data, eflip.ctypes.data))
    return esrc, eflip
