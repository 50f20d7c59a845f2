"""The corner pattern database (include/rubiksearch.h "Corner pattern database", DESIGN.md "Corner pattern database"): an exact
distance table over the corner states, built, read and searched with on the device.

On the 2x2x2 the corner index is a bijection onto the group, so the table is God's algorithm: CornerTable.distance IS the optimal
solution length, and astar_search(table, env, 1, n, weight=1.0, front="table") walks an optimal solution.  On the 3x3x3 it is the
classical admissible lower bound: h <= true distance, with the distance's parity.

    table = CornerTable.build(2, "cuda")          # 3.67 MB | 88 MB, breadth-first, one launch per level
    table.levels                                  # states per distance, level 0 first
    table.distance(env)                           # uint8 [N]
    torch.save(table.table.cpu(), path); CornerTable(torch.load(path).cuda(), 2)
"""
from __future__ import annotations

import torch

from . import _lib, _pattern_lib, ops
from ._lib import ptr, stream_ptr
from ._search_lib import check

MAX_LEVELS = 32        # a build that has not finished by then is an error (the deepest corner state is at 14 | 11)
ILLEGAL = 0xFF         # distance() of a cube whose corners are no legal corner state


class CornerTable:
    """table: uint8 device tensor [N], N = rcp_table_bytes(cube_size); levels: states per distance (None for a wrapped tensor)."""

    def __init__(self, table, cube_size, levels=None):
        """Wrap a table built earlier (CornerTable.build(...).table, loaded from disk and moved to the device).  ValueError for a tensor
        that cannot be one: wrong size, dtype or device are found before the device is touched, table[0] != 0 by reading one byte."""
        if cube_size not in (2, 3):
            raise ValueError(f"cube_size must be 2 or 3, got {cube_size!r}")
        n = _pattern_lib.table_bytes(cube_size)
        if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or table.dim() != 1 or table.numel() != n or not table.is_contiguous():
            raise ValueError(f"a {cube_size}x{cube_size}x{cube_size} corner table is a contiguous uint8 tensor of {n} entries, got "
                             f"{tuple(table.shape) if isinstance(table, torch.Tensor) else type(table).__name__}"
                             f"{' of ' + str(table.dtype) if isinstance(table, torch.Tensor) else ''}")
        if not table.is_cuda:
            raise ValueError(f"the table must live on a HIP device (there is no CPU fallback), got {table.device}")
        if table.data_ptr() % 16:
            raise ValueError("the table must start 16-byte aligned (a slice at an odd offset?)")
        if levels is None and int(table[0]) != 0:
            raise ValueError("not a corner table: table[0], the solved state's distance, is not 0")
        self.table, self.cube_size, self.device = table, int(cube_size), table.device
        self.levels = None if levels is None else tuple(int(c) for c in levels)

    @classmethod
    def build(cls, cube_size, device="cuda"):
        """Breadth-first over the index space: rcp_build_begin, then one rcp_build_level per distance until a level sets nothing (the
        count is read back once per level)."""
        n = _pattern_lib.table_bytes(cube_size)                # NotImplementedError for another size
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        _lib.init(dev)
        L = _pattern_lib.pattern_lib()
        table = torch.empty(n, dtype=torch.uint8, device=dev)
        count = torch.zeros(4, dtype=torch.int32, device=dev)  # one uint32, 16-byte aligned
        check(L.rcp_build_begin(ptr(table), n, cube_size, stream_ptr(dev)))
        levels = [1]
        for depth in range(MAX_LEVELS + 1):
            check(L.rcp_build_level(ptr(table), n, cube_size, depth, ptr(count), stream_ptr(dev)))
            c = int(count[0])
            if c == 0:
                return cls(table, cube_size, levels)
            levels.append(c)
        raise RuntimeError(f"the corner table of the {cube_size}x{cube_size}x{cube_size} has more than {MAX_LEVELS} levels")

    @property
    def depth(self):
        """The largest distance in the table (needs levels: a built table)."""
        return None if self.levels is None else len(self.levels) - 1

    def distance(self, cubes, n=None, pitch=None):
        """uint8 [N]: table[corner_index] of every cube (one rcp_lookup launch); ILLEGAL = 0xFF where the corners are no legal corner
        state.  cubes: a VecCubeEnv, or a tiled sticker buffer with n cubes (pitch None: its last dimension)."""
        if hasattr(cubes, "stickers"):
            if cubes.cube_size != self.cube_size:
                raise ValueError(f"the table is a {self.cube_size}x{self.cube_size}x{self.cube_size}'s, the cubes are {cubes.cube_size}x{cubes.cube_size}x{cubes.cube_size}")
            cubes, n = cubes.stickers, cubes.num_envs
        if n is None:
            raise ValueError("distance(stickers, n): the number of cubes is required for a sticker buffer")
        if cubes.device != self.device:
            raise ValueError(f"the table is on {self.device}, the cubes on {cubes.device}")
        S = ops._size(self.cube_size)[0]
        p = ops._state_arg(cubes, S, n, pitch, "distance stickers")
        out = torch.empty(_lib.pitch_for(max(n, 1), 16), dtype=torch.uint8, device=self.device)[:n]
        _lib.init(self.device)
        check(_pattern_lib.pattern_lib().rcp_lookup(ptr(cubes), n, p, self.cube_size, ptr(self.table), self.table.numel(), ptr(out),
                                                    stream_ptr(self.device)))
        return out

    def cubies(self, indices, out=None, cubie_pitch=None, bad=None):
        """rcp_unrank: corner indices (any integer tensor or sequence; values >= N are flagged) -> cubie rows in the rcc_* layout.  bad:
        the flag, a uint8 device tensor [1] the caller zeroes and reads; None: read back at once and raised as IndexError."""
        idx = torch.as_tensor(indices).to(self.device)
        if idx.dim() != 1 or idx.dtype.is_floating_point:
            raise ValueError("indices must be a 1-D integer tensor or sequence")
        n = idx.numel()
        if idx.dtype != torch.int32:                           # uint32 values in an int32 tensor (torch has no arithmetic on uint32)
            if n and (int(idx.min()) < 0 or int(idx.max()) > 0xFFFFFFFF):
                raise ValueError("indices must be in 0..2^32 - 1")
            idx = torch.where(idx >= 1 << 31, idx - (1 << 32), idx).to(torch.int32)
        buf = torch.empty(_lib.pitch_for(max(n, 1) * 4, 16) // 4, dtype=torch.int32, device=self.device)
        buf[:n] = idx
        SL = ops._size(self.cube_size)[2]
        if out is None:
            out = ops.alloc_code(n, self.cube_size, self.device, cubie_pitch)
        p = ops._state_arg(out, SL, n, cubie_pitch, "cubies out")
        flag = torch.zeros(1, dtype=torch.uint8, device=self.device) if bad is None else ops._vec(bad, 1, torch.uint8, "cubies bad")
        _lib.init(self.device)
        check(_pattern_lib.pattern_lib().rcp_unrank(ptr(buf), n, self.cube_size, ptr(out), p, ptr(flag), stream_ptr(self.device)))
        if bad is None and int(flag):
            raise IndexError(f"corner index out of range 0..{self.table.numel() - 1}")
        return out

    def states(self, indices):
        """Tiled sticker states [tiles, S, pitch] of the corner states `indices` (rcp_unrank, then ops.from_cubies); on the 3x3x3 the
        edges are home (the last two trade places under an odd corner permutation, so that the cube is reachable)."""
        cub = self.cubies(indices)
        return ops.from_cubies(cub, len(indices), self.cube_size, bad=torch.zeros(1, dtype=torch.uint8, device=self.device))

    def score_keys(self, keys, n_problems, width, pitch, scores):
        """rcp_score_keys: scores[j] = -table[index] for every slot of rc_search_expand's key array; -255 for a key that names no
        legal corner state."""
        check(_pattern_lib.pattern_lib().rcp_score_keys(ptr(keys), n_problems, width, pitch, self.cube_size, ptr(self.table), self.table.numel(),
                                                        ptr(scores), stream_ptr(self.device)))
