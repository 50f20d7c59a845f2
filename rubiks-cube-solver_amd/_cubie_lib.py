"""ctypes binding of the rcc_* section of librubikhip.so (include/rubikhip.h "Cubie coordinates"): the cube as (piece, orientation)
bytes, the legality status, the perfect indices and the inverse map.

The functions live in the SAME library and the same header as the rc_* ones, so there is nothing to load here: cubie_lib() takes the
library _lib.lib() has loaded (build-id check included) and gives the rcc_* entry points their signatures.  A library without them is
an error, as everywhere else."""
from __future__ import annotations

from ctypes import c_int as i32, c_int64 as i64, c_void_p as vp

from . import _lib, _native
from .tables import (RCC_BAD_COLOUR, RCC_BAD_FIXED, RCC_BAD_PIECE, RCC_DUP_PIECE, RCC_FLIP, RCC_NAMES, RCC_PARITY, RCC_TWIST,  # noqa: F401
                     rcc_status_names)

# every rcc_* function of include/rubikhip.h, once (the format of _lib.SIGNATURES)
CUBIE_SIGNATURES = {
    "rcc_cubies": [vp, i64, i64, i32, vp, i64, vp, vp, vp, vp],
    "rcc_from_cubies": [vp, i64, i64, i32, vp, i64, vp, vp],
    "rcc_tables": [i32, vp, vp, vp, vp],
}

# librubikhip.so with the rcc_* signatures applied (once)
cubie_lib = _native.extension(_lib.lib, CUBIE_SIGNATURES, "hip")


def tables(cube_size):
    """Host copy of the rule's tables baked into the library (rcc_tables; needs no GPU): dict of uint8 numpy arrays corner_cw [NC, 3],
    edge_facelets [NE, 2], corner_colours [NC, 3], edge_colours [NE, 2] -- the same numbers as tables.get_cubies."""
    import numpy as np

    if cube_size not in (2, 3):
        raise NotImplementedError(f"cube_size {cube_size}")
    nc, ne = (8, 12) if cube_size == 3 else (7, 0)
    out = dict(corner_cw=np.zeros((nc, 3), np.uint8), edge_facelets=np.zeros((max(ne, 1), 2), np.uint8),
               corner_colours=np.zeros((nc, 3), np.uint8), edge_colours=np.zeros((max(ne, 1), 2), np.uint8))
    _lib.check(cubie_lib().rcc_tables(cube_size, *(v.ctypes.data_as(vp) for v in out.values())))
    out["edge_facelets"], out["edge_colours"] = out["edge_facelets"][:ne], out["edge_colours"][:ne]
    return out
