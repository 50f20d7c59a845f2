"""ctypes binding of librubiksearch.so (include/rubiksearch.h): the kernels of the batched beam search (search.py).

Built by __graft_entry__.build() with hipcc for gfx950.  Like _lib.py there is no fallback: if the library is missing or was built
from other sources, search_lib() raises."""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  -- loaded before the library so that both share one HIP runtime

from ._lib import RubikHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RUBIKSEARCH_LIB") or os.path.join(_HERE, "librubiksearch.so")   # env override: A/B builds in experiments
VALID, SOLVED, SURVIVOR = 1, 2, 4
_lib = None


def search_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RubikHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        from . import _build
        L.rc_search_build_id.restype = ctypes.c_char_p
        try:                                                    # a stale build is refused, not used (RC_ALLOW_STALE=1: A/B experiments)
            _build.check_loaded(LIB_PATH, L.rc_search_build_id().decode(), _build.SEARCH_SOURCES)
        except RuntimeError as e:
            raise RubikHipError(str(e)) from None
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.rc_search_last_error.restype = ctypes.c_char_p
        L.rc_search_workspace_bytes.argtypes, L.rc_search_workspace_bytes.restype = [i32, i64, i32], i64
        for name, args in (("rc_search_init", [vp, i64, i64, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp]),
                           ("rc_search_expand", [vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp]),
                           ("rc_search_select", [vp, vp, vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp]),
                           ("rc_search_advance", [vp, vp, i64, i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
                           ("rc_search_backtrack", [vp, vp, i64, i32, i64, i32, i32, vp, vp, vp, vp])):
            f = getattr(L, name)
            f.argtypes, f.restype = args, i32
        _lib = L
    return _lib


def build_id() -> str:
    """The source hash the loaded library was built from (rc_search_build_id)."""
    return search_lib().rc_search_build_id().decode()


def check(rc):
    if rc != 0:
        raise RubikHipError(f"librubiksearch error {rc}: {search_lib().rc_search_last_error().decode()}")
