"""ctypes binding of the tp_* section of librubikhip.so (include/rubikhip.h "Two-phase"): Kociemba's two-phase algorithm -- four
coset-distance tables, their index, and the two budgeted search steps.

The functions live in the SAME library and the same header as the rc_*, rcc_*, rce_*, rct_* and ida_* ones, so there is nothing to
load here: twophase_lib() takes the library _lib.lib() has loaded (build-id check included) and gives the tp_* entry points their
signatures.  A library without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import byref, c_int as i32, c_int64 as i64, c_void_p as vp

import numpy as np

from . import _lib, _native

TABLES = 4                 # twist-slice, flip-slice (phase 1), corner-slice, edge-slice (phase 2)
MAX_DEPTH = 48             # rows of a path
MAX_TRAIL = 32             # nibbles of a trail: actions of phase 1, generators of phase 2
MAX_CANDIDATES = 4096
NOOP = 12                  # "no move": what the caller prefills path with
INF = 2 ** 31 - 1
SOLVED = FULL = 1          # TP_*: the status bits
EXHAUSTED, ILLEGAL, BAD_FRAME, OUTSIDE = 2, 4, 8, 16

_CUBES = [vp, i64, i64, vp, i64, vp, i64]                 # cubies, n, cubie_pitch, table_a, bytes_a, table_b, bytes_b
_FRAME1 = [vp, i32, i64, vp, i32, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]   # limit, candidates, stride, path, max_depth, path_pitch,
#                                 cand_length, cand_cubies, cand_pitch, trail, cursor, depth, bound, next, nodes, found, status
_FRAME2 = [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]   # path, max_depth, path_pitch, floor, limit, trail, cursor, depth, bound, next, nodes, status

# every tp_* function of include/rubikhip.h, once (the format of _lib.SIGNATURES)
TWOPHASE_SIGNATURES = {
    "tp_table_bytes": ([i32], i64),
    "tp_generators": [i32, vp, vp, vp],
    "tp_max_steps": ([], i64),
    "tp_build_begin": [vp, i64, i32, vp],
    "tp_build_level": [vp, i64, i32, i32, vp, vp],
    "tp_index": [vp, i64, i64, i32, vp, vp],
    "tp_phase1_init": _CUBES + _FRAME1 + [vp],
    "tp_phase1_search": _CUBES + _FRAME1 + [i64, vp, vp],
    "tp_phase2_init": _CUBES + _FRAME2 + [vp],
    "tp_phase2_search": _CUBES + _FRAME2 + [i64, vp, vp],
}

# librubikhip.so with the tp_* signatures applied (once)
twophase_lib = _native.extension(_lib.lib, TWOPHASE_SIGNATURES, "hip")


def check_which(which) -> int:
    if isinstance(which, bool) or not isinstance(which, (int, np.integer)) or not 0 <= which < TABLES:
        raise ValueError(f"which must be an integer in 0..{TABLES - 1}, got {which!r}")
    return int(which)


def table_bytes(which) -> int:
    """tp_table_bytes: N of a table = its bytes (no device needed)."""
    return int(twophase_lib().tp_table_bytes(check_which(which)))


def max_steps() -> int:
    """tp_max_steps: the largest max_steps one tp_phase1_search / tp_phase2_search call takes (no device needed)."""
    return int(twophase_lib().tp_max_steps())


def generators(phase):
    """tp_generators: (uint8 [count, 2], the one or two quarter-turn actions of each generator of phase 1 | 2 in the rule's order (0xFF:
    no second action); uint8 [count], its cost)."""
    if phase not in (1, 2) or isinstance(phase, bool):
        raise ValueError(f"phase must be 1 or 2, got {phase!r}")
    gens, cost, count = np.zeros((12, 2), np.uint8), np.zeros(12, np.uint8), i32(0)
    _lib.check(twophase_lib().tp_generators(int(phase), gens.ctypes.data, cost.ctypes.data, byref(count)))
    return gens[:count.value].copy(), cost[:count.value].copy()
