"""ctypes binding of librubiknet.so (include/rubiknet.h): the value net's first layer from compact codes (codenet.py).

Built by __graft_entry__.build() with hipcc for gfx950.  Like _lib.py there is no fallback: if the library is missing or was built
from other sources, net_lib() raises (_native.load)."""
from __future__ import annotations

from ctypes import c_char_p, c_int as i32, c_int64 as i64, c_void_p as vp

from . import _native
from ._native import RubikHipError  # noqa: F401

LIB_PATH = _native.path("net")
ACT_NONE, ACT_ELU = 0, 1
SIGNATURES = {
    "rc_net_build_id": ([], c_char_p),
    "rc_net_last_error": ([], c_char_p),
    "rc_net_first_layer": [vp, i64, i64, i32, vp, vp, i32, i32, i32, vp, i32, i64, vp],
}


def net_lib():
    return _native.load("net", SIGNATURES)


def build_id() -> str:
    """The source hash the loaded library was built from (rc_net_build_id)."""
    return _native.build_id("net", net_lib())


def check(rc):
    if rc != 0:
        raise _native.error("net", net_lib(), rc)
