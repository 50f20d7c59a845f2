"""ctypes binding of the rct_* section of librubikhip.so (include/rubikhip.h "Subgroup chain"): Thistlethwaite's four coset-distance
tables of the 3x3x3 -- build, index, unrank, descend.

The functions live in the SAME library and the same header as the rc_*, rcc_* and rce_* ones, so there is nothing to load here:
chain_lib() takes the library _lib.lib() has loaded (build-id check included) and gives the rct_* entry points their signatures.  A
library without them is an error, as everywhere else."""
from __future__ import annotations

from ctypes import byref, c_int as i32, c_int64 as i64, c_void_p as vp

import numpy as np

from . import _lib, _native

STAGES = 4
N_COSETS = 96              # |H|, the corner permutations half turns reach
MAX_GENERATORS = 47        # 7 + 11 + 14 + 15, the depths of the four tables
MAX_LENGTH = 87            # quarter turns: 7 + 2 * 11 + 2 * 14 + 2 * 15
ILLEGAL, OUTSIDE, NO_ROOM, STUCK = 1, 2, 4, 8      # RCT_*: rct_descend's status bits

# every rct_* function of include/rubikhip.h, once (the format of _lib.SIGNATURES)
CHAIN_SIGNATURES = {
    "rct_table_bytes": ([i32], i64),
    "rct_generators": [i32, vp, vp],
    "rct_corner_cosets": [vp],
    "rct_build_begin": [vp, i64, i32, vp],
    "rct_build_level": [vp, i64, i32, i32, vp, vp],
    "rct_index": [vp, i64, i64, i32, vp, vp],
    "rct_unrank": [vp, i64, i32, vp, i64, vp, vp],
    "rct_descend": [vp, i64, i64, i32, vp, i64, vp, i32, i64, vp, vp, vp, vp],
}

# librubikhip.so with the rct_* signatures applied (once)
chain_lib = _native.extension(_lib.lib, CHAIN_SIGNATURES, "hip")


def check_stage(stage) -> int:
    if isinstance(stage, bool) or not isinstance(stage, (int, np.integer)) or not 0 <= stage < STAGES:
        raise ValueError(f"stage must be an integer in 0..{STAGES - 1}, got {stage!r}")
    return int(stage)


def table_bytes(stage) -> int:
    """rct_table_bytes: N of a stage = the bytes of its table (no device needed)."""
    return int(chain_lib().rct_table_bytes(check_stage(stage)))


def generators(stage):
    """rct_generators: uint8 [count, 2], the one or two quarter-turn actions of each generator of a stage, in the rule's order (0xFF:
    no second action)."""
    gens, count = np.zeros((12, 2), np.uint8), i32(0)
    _lib.check(chain_lib().rct_generators(check_stage(stage), gens.ctypes.data, byref(count)))
    return gens[:count.value].copy()


def corner_cosets():
    """rct_corner_cosets: sorted H, uint16 [96] -- what the kernels were compiled with; tables.get_chain is what it was generated from."""
    h = np.zeros(N_COSETS, np.uint16)
    _lib.check(chain_lib().rct_corner_cosets(h.ctypes.data))
    return h
