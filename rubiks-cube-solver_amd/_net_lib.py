"""ctypes binding of librubiknet.so (include/rubiknet.h): the value net's first layer from compact codes (codenet.py).

Built by __graft_entry__.build() with hipcc for gfx950.  Like _lib.py there is no fallback: if the library is missing or was built
from other sources, net_lib() raises."""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  -- loaded before the library so that both share one HIP runtime

from ._lib import RubikHipError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RUBIKNET_LIB") or os.path.join(_HERE, "librubiknet.so")   # env override: A/B builds in experiments
ACT_NONE, ACT_ELU = 0, 1
_lib = None


def net_lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RubikHipError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        from . import _build
        L.rc_net_build_id.restype = ctypes.c_char_p
        try:                                                    # a stale build is refused, not used (RC_ALLOW_STALE=1: A/B experiments)
            _build.check_loaded(LIB_PATH, L.rc_net_build_id().decode(), _build.NET_SOURCES)
        except RuntimeError as e:
            raise RubikHipError(str(e)) from None
        vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
        L.rc_net_last_error.restype = ctypes.c_char_p
        L.rc_net_first_layer.argtypes = [vp, i64, i64, i32, vp, vp, i32, i32, i32, vp, i32, i64, vp]
        L.rc_net_first_layer.restype = i32
        _lib = L
    return _lib


def build_id() -> str:
    """The source hash the loaded library was built from (rc_net_build_id)."""
    return net_lib().rc_net_build_id().decode()


def check(rc):
    if rc != 0:
        raise RubikHipError(f"librubiknet error {rc}: {net_lib().rc_net_last_error().decode()}")
