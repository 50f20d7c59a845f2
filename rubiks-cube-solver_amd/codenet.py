"""The value net fed from compact codes (DESIGN.md "Net front"): the first layer of the reference's DeepCube (model.py:13-29,
`Flatten, Linear(R * C, H1), ELU`) of a one-hot is the sum of SLOTS rows of the transposed weight plus the bias, and
librubiknet.so (include/rubiknet.h) computes it from an RC_FMT_CODE buffer.  No dense one-hot exists on this path.

There is no fallback: a module that does not have the reference's layout is refused with a TypeError."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, _net_lib, ops
from ._lib import RubikHipError, ptr, stream_ptr
from .ops import N_SLOTS
from .tables import STATE_DIM

_FMT = {torch.float32: _lib.FMT_F32, torch.bfloat16: _lib.FMT_BF16}
N_CODES = {3: 24, 2: 21}


def onehot_index(cube_size):
    """int64 numpy [SLOTS, n_codes]: the flat index k(s, c) of the dense one-hot's 1 for slot s holding code c (include/rubikhip.h
    "One-hot formats") = the row of the transposed first-layer weight.  The one place the mapping is written down in Python."""
    if cube_size not in (2, 3):
        raise NotImplementedError(f"cube_size {cube_size}")
    s = np.arange(N_SLOTS[cube_size], dtype=np.int64)[:, None]
    c = np.arange(N_CODES[cube_size], dtype=np.int64)[None, :]
    if cube_size == 3:
        return s * 24 + c                       # row = slot, column = code
    return (c // 3) * 21 + s * 3 + c % 3        # row = piece, column = slot * 3 + orientation


def first_layer(code, n, cube_size, weight_t, bias, out, act=True):
    """out[:n, :H] = act(bias + the rows of weight_t picked by the codes), one launch of rc_net_first_layer.
    code: an RC_FMT_CODE buffer [tiles, SLOTS, pitch] (or [SLOTS, pitch]); weight_t: contiguous [R * C, H] float32 | bfloat16;
    bias: [H] of the same dtype or None; out: [>= n, >= H] float32 | bfloat16 with unit column stride; act: ELU (alpha 1) or none."""
    R, C = STATE_DIM[cube_size]
    cp = ops._tiled(code, N_SLOTS[cube_size], n, "first_layer")
    if weight_t.dtype not in _FMT or out.dtype not in _FMT:
        raise RubikHipError(f"first_layer: weight and output must be float32 or bfloat16, got {weight_t.dtype} and {out.dtype}")
    if weight_t.dim() != 2 or weight_t.shape[0] != R * C or not weight_t.is_contiguous() or weight_t.device != code.device:
        raise RubikHipError(f"first_layer: weight_t must be a contiguous [{R * C}, hidden] tensor on {code.device}")
    H = weight_t.shape[1]
    if bias is not None and (bias.dtype != weight_t.dtype or bias.shape != (H,) or not bias.is_contiguous() or bias.device != code.device):
        raise RubikHipError(f"first_layer: bias must be a contiguous [{H}] {weight_t.dtype} tensor on {code.device}")
    if out.dim() != 2 or out.shape[0] < n or out.shape[1] < H or (out.shape[1] > 1 and out.stride(1) != 1) or out.device != code.device:
        raise RubikHipError(f"first_layer: out must be [>= {n}, >= {H}] with unit column stride on {code.device}")
    _lib.init(code.device)
    _net_lib.check(_net_lib.net_lib().rc_net_first_layer(ptr(code), n, cp, cube_size, ptr(weight_t), ptr(bias), H, _FMT[weight_t.dtype],
                                                         _net_lib.ACT_ELU if act else _net_lib.ACT_NONE, ptr(out), _FMT[out.dtype],
                                                         out.stride(0), stream_ptr(code.device)))
    return out


class CodeNet:
    """A module with the reference's layout -- encoder_net = Sequential(Flatten, Linear(R * C, H1), ELU(alpha=1), ...), value_net,
    policy_net -- evaluated from compact codes: forward_codes(code, n) equals model(onehot of the codes).

    The wrapper holds W1 transposed ([R * C, H1], contiguous, the model's dtype).  Every call compares the weight's `_version` and
    `data_ptr()` with those of the last copy and refreshes the table with copy_ into the SAME storage when either changed: an
    optimiser step between two searches is seen, and a captured graph keeps a valid address.  (A write through `weight.data`
    bypasses the version counter: call refresh().)"""

    def __init__(self, model, cube_size=None):
        nn = torch.nn
        enc = getattr(model, "encoder_net", None)
        if not isinstance(enc, nn.Sequential) or len(enc) < 3:
            raise TypeError("CodeNet: expected a module with encoder_net = Sequential(Flatten, Linear(R * C, H1), ELU, ...) (model.py:13-19), "
                            f"got {type(model).__name__} with encoder_net = {type(enc).__name__}")
        if not isinstance(enc[0], nn.Flatten) or not isinstance(enc[1], nn.Linear) or not isinstance(enc[2], nn.ELU):
            raise TypeError("CodeNet: expected encoder_net to start with Flatten, Linear, ELU, got " + ", ".join(type(m).__name__ for m in list(enc)[:3]))
        if enc[2].alpha != 1.0:
            raise TypeError(f"CodeNet: expected ELU(alpha=1) after the first Linear, got alpha = {enc[2].alpha}")
        for head in ("value_net", "policy_net"):
            if not isinstance(getattr(model, head, None), nn.Module):
                raise TypeError(f"CodeNet: expected a module with a {head} (model.py:20-29)")
        sizes = {STATE_DIM[cs][0] * STATE_DIM[cs][1]: cs for cs in (2, 3)}
        want = sizes if cube_size is None else {STATE_DIM[cube_size][0] * STATE_DIM[cube_size][1]: cube_size}
        if enc[1].in_features not in want:
            raise TypeError(f"CodeNet: expected Linear.in_features == R * C = {' | '.join(map(str, sorted(want)))}, got {enc[1].in_features}")
        H = enc[1].out_features
        if H % 8 or not 8 <= H <= 4096:
            raise TypeError(f"CodeNet: expected a first layer of a multiple of 8 in 8..4096 outputs (include/rubiknet.h), got {H}")
        self.model, self.cube_size, self.hidden = model, want[enc[1].in_features], H
        self.linear, self.tail = enc[1], enc[3:]
        self.weight_t, self._seen = None, None
        self.refresh()

    @property
    def dtype(self):
        return self.linear.weight.dtype

    @property
    def device(self):
        return self.linear.weight.device

    @torch.no_grad()
    def refresh(self):
        """Copy W1 transposed into the table (same storage unless the dtype or the device changed)."""
        w = self.linear.weight
        if w.dtype not in _FMT:
            raise ValueError(f"CodeNet: the first-layer kernel takes float32 and bfloat16 weights, the model has {w.dtype}")
        if self.weight_t is None or self.weight_t.dtype != w.dtype or self.weight_t.device != w.device:
            self.weight_t = torch.empty((w.shape[1], w.shape[0]), dtype=w.dtype, device=w.device)
        self.weight_t.copy_(w.t())
        self._seen = (w._version, w.data_ptr(), w.dtype, w.device)

    def _sync(self):
        w = self.linear.weight
        if self._seen != (w._version, w.data_ptr(), w.dtype, w.device):
            self.refresh()

    def hidden_codes(self, code, n, out=None):
        """ELU(W1 onehot + b1) of the n states of `code`: [n, H1] in the model's dtype (a view of `out`, [>= n, >= H1], if given)."""
        self._sync()
        if out is None:
            out = torch.empty((n, self.hidden), dtype=self.dtype, device=self.device)
        b = self.linear.bias
        first_layer(code, n, self.cube_size, self.weight_t, None if b is None else b.detach(), out, act=True)
        return out[:n, :self.hidden]

    def forward_codes(self, code, n, out=None):
        """(value [n, 1], policy [n, A]) = model(onehot of the codes)."""
        x = self.tail(self.hidden_codes(code, n, out))
        return self.model.value_net(x), self.model.policy_net(x)

    def value_codes(self, code, n, out=None):
        """value [n, 1] only: the rest of the encoder and the value head (the policy head is not run)."""
        return self.model.value_net(self.tail(self.hidden_codes(code, n, out)))
