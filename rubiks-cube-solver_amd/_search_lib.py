"""ctypes binding of librubiksearch.so (include/rubiksearch.h): the kernels of the batched beam search (search.py).

Built by __graft_entry__.build() with hipcc for gfx950.  Like _lib.py there is no fallback: if the library is missing or was built
from other sources, search_lib() raises (_native.load)."""
from __future__ import annotations

from ctypes import c_char_p, c_int as i32, c_int64 as i64, c_void_p as vp

from . import _native
from ._native import RubikHipError  # noqa: F401

LIB_PATH = _native.path("search")
VALID, SOLVED, SURVIVOR = 1, 2, 4
SIGNATURES = {
    "rc_search_build_id": ([], c_char_p),
    "rc_search_last_error": ([], c_char_p),
    "rc_search_workspace_bytes": ([i32, i64, i32], i64),
    "rc_search_init": [vp, i64, i64, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp],
    "rc_search_expand": [vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp],
    "rc_search_select": [vp, vp, vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp],
    "rc_search_advance": [vp, vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp],
    "rc_search_backtrack": [vp, vp, i64, i32, i64, i32, i32, vp, vp, vp, vp],
}


def search_lib():
    return _native.load("search", SIGNATURES)


def build_id() -> str:
    """The source hash the loaded library was built from (rc_search_build_id)."""
    return _native.build_id("search", search_lib())


def check(rc):
    if rc != 0:
        raise _native.error("search", search_lib(), rc)
