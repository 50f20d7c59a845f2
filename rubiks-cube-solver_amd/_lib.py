"""ctypes binding of librubikhip.so (include/rubikhip.h) over PyTorch-ROCm tensors.

PyTorch is plumbing only: it owns the device buffers and the HIP stream; every cube
operation is a kernel of librubikhip.so.  There is NO fallback: if the library is missing
or was not built, importing this module's `lib()` raises, loudly.
"""
from __future__ import annotations

import ctypes

import torch  # must be imported before the library so both share one HIP runtime (libamdhip64.so.7)

from . import _native
from ._native import RubikHipError  # noqa: F401  -- the package's error type lives with the loader; importable from here as before

LIB_PATH = _native.path("hip")

FMT_NONE, FMT_CODE, FMT_U8, FMT_F16, FMT_F32, FMT_BF16 = 0, 1, 2, 3, 4, 5
_FMT_DTYPE = {FMT_U8: torch.uint8, FMT_F16: torch.float16, FMT_F32: torch.float32, FMT_BF16: torch.bfloat16}
STATUS_BAD_ACTION = 1

_inited = set()

vp, i64, i32, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_uint64
# every function of include/rubikhip.h, once: argument types, or (argument types, result type) where the result is not a C int
SIGNATURES = {
    "rc_version": [],
    "rc_build_id": ([], ctypes.c_char_p),
    "rc_last_error": ([], ctypes.c_char_p),
    "rc_init": [i32],
    "rc_get_tables": [i32, vp, vp, vp, vp, vp, vp, vp],
    "rc_fill_solved": [vp, i64, i64, i32, vp],
    "rc_apply_moves": [vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, i32, i64, vp],
    "rc_apply_moves_ex": [vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, i32, i64, vp, i32],
    "rc_apply_moves_ws": [vp, vp, vp, i64, i64, i64, i32, vp, vp, vp, i32, i64, vp, i64, vp],
    "rc_encode_ws": [vp, i64, i64, i32, vp, i32, i64, vp, i64, vp],
    "rc_workspace_bytes": ([i32, i32, i64, i32], i64),
    "rc_facade_step": [vp, i64, i32, i32, vp, ctypes.c_uint32, i32, vp],
    "rc_facade_steps": [vp, i64, i32, vp, i32, vp, ctypes.c_uint32, i32, vp],
    "rc_facade_expand": [vp, i64, i32, vp, ctypes.c_uint32, i32, i32, vp],
    "rc_scramble": [vp, i64, i64, i32, i32, u64, u64, i64, vp, vp, i64, vp, vp, vp],
    "rc_legacy_scramble_actions": [vp, vp, i32, i32, i64, i32, vp, i64, vp],
    "rc_is_solved": [vp, i64, i64, i32, vp, vp, vp],
    "rc_encode": [vp, i64, i64, i32, vp, i32, i64, vp],
    "rc_onehot_from_code": [vp, i64, i64, i32, vp, i32, vp],
    "rc_onehot_from_code_ex": [vp, i64, i64, i32, vp, i32, vp, i32],
    "rc_onehot_from_code_blocks": [vp, i64, i64, i32, vp, i32, i32, i64, i64, vp],
    "rc_expand_children": [vp, i64, i64, i32, vp, vp, vp, i64, vp],
    "rc_expand_children_ex": [vp, i64, i64, i32, vp, vp, vp, i64, vp, i32],
    "rc_adi_generate": [u64, u64, i64, i64, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp],
    "rc_adi_generate_ex": [u64, u64, i64, i64, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, i32],
    "rc_adi_generate_family": [u64, u64, i64, i64, i32, i32, i64, vp, vp, vp, vp, vp, vp, i32],
    "rc_family_layout": [i32, vp, vp],
    "rc_onehot_from_family": [vp, i64, i64, i32, vp, i32, i64, vp],
    "rc_adi_targets": [vp, vp, vp, vp, i64, i64, i32, vp, vp, vp, vp],
    "rc_adi_targets_depths": [vp, i64, i64, vp, i64, vp, i64, vp, i64, i32, i32, vp, vp, vp, i64, vp],
    "rc_onehot_from_family_depths": [vp, i64, i64, i32, vp, i32, i64, i32, vp],
    "rc_legacy_scramble_actions_ex": [vp, vp, i32, i32, i64, i32, vp, i64, vp, i32],
    "rc_read_status": [vp, vp],
    "rc_describe_dispatch": [i32, i32, i64, i32, ctypes.c_uint32, i32, i32, ctypes.c_char_p, i32],
    "rc_facade_release": [vp],
    "rc_host_alias": [vp, vp],
    "rc_scramble_from": [vp, vp, i64, i64, i32, i32, u64, u64, i64, vp, vp, i64, vp, vp, vp],
    "rc_search_pack": [vp, vp, vp, i64, i64, i32, vp, vp, vp, vp],
}


def lib():
    """The loaded library (loads on first use).  Raises if it was not built."""
    return _native.load("hip", SIGNATURES)


def build_id() -> str:
    """The source hash the loaded library was built from (rc_build_id)."""
    return _native.build_id("hip", lib())


def check(rc):
    if rc != 0:
        raise _native.error("hip", lib(), rc)


def init(device: torch.device):
    """rc_init for the tensor's device (once per device per process)."""
    if device.type != "cuda":
        raise RubikHipError(f"cube tensors must live on a HIP device, got {device}")
    cur = torch.cuda.current_device()
    idx = device.index if device.index is not None else cur
    if idx != cur:
        # kernels are launched for the CURRENT device; one process per GPU is the deployment model
        raise RubikHipError(f"tensor lives on cuda:{idx} but cuda:{cur} is current: call torch.cuda.set_device({idx}) "
                            f"(or use `with torch.cuda.device({idx}):`) around cube operations")
    if idx not in _inited:
        check(lib().rc_init(idx))
        _inited.add(idx)
    return idx


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # the current stream's handle without building a Stream object


def stream_ptr(device=None):
    """hipStream_t of torch's CURRENT stream on `device` as a void* (looked up per call: the library is stream-ordered)."""
    if _raw_stream is not None:
        if isinstance(device, str):
            device = torch.device(device)
        idx = device.index if isinstance(device, torch.device) else device if isinstance(device, int) else None
        if idx is None:
            idx = torch.cuda.current_device()
        return ctypes.c_void_p(_raw_stream(idx))
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def host_alias(t):
    """Device address of a pinned (host-mapped) CPU tensor, as a void*: kernels may read it in place (rc_host_alias)."""
    if t.is_cuda or not t.is_pinned():
        raise RubikHipError("host_alias: need a pinned CPU tensor")
    out = ctypes.c_void_p(0)
    check(lib().rc_host_alias(ctypes.c_void_p(t.data_ptr()), ctypes.byref(out)))
    return out


def pitch_for(n: int, align: int = 256) -> int:
    """Row pitch: >= n, multiple of `align` bytes (256 keeps every row segment line-aligned)."""
    return max(align, (n + align - 1) // align * align)


def dense_dtype(fmt):
    return _FMT_DTYPE[fmt]


def fmt_of(dtype):
    for f, d in _FMT_DTYPE.items():
        if d == dtype:
            return f
    raise RubikHipError(f"no dense one-hot format for dtype {dtype}")


def read_status(device=None) -> int:
    out = ctypes.c_uint32(0)
    check(lib().rc_read_status(ctypes.byref(out), stream_ptr(device)))
    return out.value


OP_STEP, OP_EXPAND, OP_ADI, OP_CODE_TO_DENSE, OP_FAMILY_TO_DENSE = 1, 2, 3, 4, 5
OUT_STATES, OUT_CODE, OUT_FLAGS, OUT_REWARD, OUT_INPLACE, OUT_DONE, OUT_WORKSPACE, OUT_FAMILY = 1, 2, 4, 8, 16, 32, 64, 128


def describe(op, cube_size, n, depth=0, outputs=0, fmt=FMT_NONE, variant=0) -> str:
    """The kernel instantiation + launch geometry a call WOULD use (rc_describe_dispatch): the library's own dispatch
    functions decide, nothing is launched.  Works without a GPU."""
    buf = ctypes.create_string_buffer(160)
    check(lib().rc_describe_dispatch(op, cube_size, n, depth, outputs, fmt, variant, buf, len(buf)))
    return buf.value.decode()


def get_tables(cube_size):
    """Host copy of the tables baked into the library (for tests: same numbers as tables.py)."""
    import numpy as np

    dims = (ctypes.c_int32 * 6)()
    check(lib().rc_get_tables(cube_size, None, None, None, None, None, None, dims))
    S, A, NC, NE, R, C = list(dims)
    out = dict(perm=np.zeros((A, S), np.uint8), solved=np.zeros(S, np.uint8), corner_defs=np.zeros((NC, 3), np.uint8),
               edge_defs=np.zeros((max(NE, 1), 2), np.uint8), corner_code=np.zeros(72, np.uint8), edge_code=np.zeros(72, np.uint8))
    check(lib().rc_get_tables(cube_size, *(v.ctypes.data_as(ctypes.c_void_p) for v in out.values()), dims))
    out["edge_defs"] = out["edge_defs"][:NE]
    out["dims"] = (S, A, NC, NE, R, C)
    return out


_family = {}


def family_layout(cube_size):
    """(NF, rows) of the FAMILY record (include/rubikhip.h rc_adi_generate_family): rows[a][p] = the family row that is slot p's code of
    child a (a = A: the parent), uint8 numpy [A + 1, SLOTS].  Needs no GPU."""
    if cube_size not in _family:
        import numpy as np
        A, SL = (12, 20) if cube_size == 3 else (6, 7)
        rows = np.zeros((A + 1, SL), np.uint8)
        nf = ctypes.c_int32(0)
        check(lib().rc_family_layout(cube_size, rows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(nf)))
        _family[cube_size] = (int(nf.value), rows)
    return _family[cube_size]
