"""The corner pattern database (include/rubiksearch.h "Corner pattern database", DESIGN.md "Corner pattern database"): an exact
distance table over the corner states, built, read and searched with on the device.

On the 2x2x2 the corner index is a bijection onto the group, so the table is God's algorithm: CornerTable.distance IS the optimal
solution length, and astar_search(table, env, 1, n, weight=1.0, front="table") walks an optimal solution.  On the 3x3x3 it is the
classical admissible lower bound: h <= true distance, with the distance's parity.

    table = CornerTable.build(2, "cuda")          # 3.67 MB | 88 MB, breadth-first, one launch per level
    table.levels                                  # states per distance, level 0 first
    table.distance(env)                           # uint8 [N]
    torch.save(table.table.cpu(), path); CornerTable(torch.load(path).cuda(), 2)

The 3x3x3's corner table sees 8 of 20 cubies.  EdgeTable (include/rubikhip.h "Edge pattern databases", DESIGN.md "Edge pattern
databases") is its companion over up to 7 tracked edge pieces, and MaxTable(corner, *edge_tables) the maximum of several tables --
admissible and consistent like its members, and accepted by front="table" wherever a CornerTable is.  ChainTables and TwoPhaseTables
are coset-distance tables: distances to a subgroup, not to the solved cube (include/rubikhip.h "Subgroup chain", "Two-phase").
"""
from __future__ import annotations

import torch

from . import _lib, _pattern_lib, ops
from ._lib import ptr, stream_ptr
from ._search_lib import check

MAX_LEVELS = 32        # a build that has not finished by then is an error (the deepest corner state is at 14 | 11)
ILLEGAL = 0xFF         # distance() of a cube whose corners are no legal corner state


def _device(device):
    """torch.device(device), "cuda" resolved to the current device's index."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _check_table(t, n, what, tables="the table", every="the table"):
    """ValueError unless t can be `what`: a contiguous uint8 tensor of n entries on a HIP device, 16-byte aligned.  Nothing here
    touches the device."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what} is a contiguous uint8 tensor of {n} entries, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}"
                         f"{' of ' + str(t.dtype) if isinstance(t, torch.Tensor) else ''}")
    if not t.is_cuda:
        raise ValueError(f"{tables} must live on a HIP device (there is no CPU fallback), got {t.device}")
    if t.data_ptr() % 16:
        raise ValueError(f"{every} must start 16-byte aligned (a slice at an odd offset?)")


def _index_buffer(indices, device):
    """(int32 device buffer padded to 16 bytes, n) of any 1-D integer tensor or sequence of uint32 values."""
    idx = torch.as_tensor(indices).to(device)
    if idx.dim() != 1 or idx.dtype.is_floating_point:
        raise ValueError("indices must be a 1-D integer tensor or sequence")
    n = idx.numel()
    if idx.dtype != torch.int32:                           # uint32 values in an int32 tensor (torch has no arithmetic on uint32)
        if n and (int(idx.min()) < 0 or int(idx.max()) > 0xFFFFFFFF):
            raise ValueError("indices must be in 0..2^32 - 1")
        idx = torch.where(idx >= 1 << 31, idx - (1 << 32), idx).to(torch.int32)
    buf = torch.empty(_lib.pitch_for(max(n, 1) * 4, 16) // 4, dtype=torch.int32, device=device)
    buf[:n] = idx
    return buf, n


def _build_levels(begin, level, table, n, dev, first_level, what):
    """Breadth-first over an index space: begin(ptr, n, stream), then level(ptr, n, depth, count ptr, stream) per distance until a
    level sets nothing (the count is read back once per level).  -> entries per distance; first_level(table): those at distance 0."""
    count = torch.zeros(4, dtype=torch.int32, device=dev)  # one uint32, 16-byte aligned
    begin(ptr(table), n, stream_ptr(dev))
    levels = [first_level(table)]
    for depth in range(MAX_LEVELS + 1):
        level(ptr(table), n, depth, ptr(count), stream_ptr(dev))
        c = int(count[0])
        if c == 0:
            return levels
        levels.append(c)
    raise RuntimeError(f"{what} has more than {MAX_LEVELS} levels")


class CornerTable:
    """table: uint8 device tensor [N], N = rcp_table_bytes(cube_size); levels: states per distance (None for a wrapped tensor)."""

    def __init__(self, table, cube_size, levels=None):
        """Wrap a table built earlier (CornerTable.build(...).table, loaded from disk and moved to the device).  ValueError for a tensor
        that cannot be one: wrong size, dtype or device are found before the device is touched, table[0] != 0 by reading one byte."""
        if cube_size not in (2, 3):
            raise ValueError(f"cube_size must be 2 or 3, got {cube_size!r}")
        _check_table(table, _pattern_lib.table_bytes(cube_size), f"a {cube_size}x{cube_size}x{cube_size} corner table")
        if levels is None and int(table[0]) != 0:
            raise ValueError("not a corner table: table[0], the solved state's distance, is not 0")
        self.table, self.cube_size, self.device = table, int(cube_size), table.device
        self.levels = None if levels is None else tuple(int(c) for c in levels)

    @classmethod
    def build(cls, cube_size, device="cuda"):
        """Breadth-first over the index space: rcp_build_begin, then one rcp_build_level per distance until a level sets nothing (the
        count is read back once per level)."""
        n = _pattern_lib.table_bytes(cube_size)                # NotImplementedError for another size
        dev = _device(device)
        _lib.init(dev)
        L = _pattern_lib.pattern_lib()
        table = torch.empty(n, dtype=torch.uint8, device=dev)
        levels = _build_levels(lambda t, n, st: check(L.rcp_build_begin(t, n, cube_size, st)),
                               lambda t, n, depth, count, st: check(L.rcp_build_level(t, n, cube_size, depth, count, st)),
                               table, n, dev, lambda table: 1, f"the corner table of the {cube_size}x{cube_size}x{cube_size}")
        return cls(table, cube_size, levels)

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
        buf, n = _index_buffer(indices, self.device)
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


class EdgeTable:
    """An edge pattern database of the 3x3x3 (include/rubikhip.h "Edge pattern databases", DESIGN.md "Edge pattern databases"): the
    exact number of quarter turns that bring up to 7 tracked edge pieces home, whatever the other cubies do -- an admissible,
    consistent lower bound that sees what the corner table is blind to.

        e = EdgeTable.build(range(6), "cuda")         # pieces 0..5: 42.6 MB, breadth-first, one launch per level
        e.distance(env)                               # uint8 [N]
        MaxTable(corner, e, EdgeTable.build(range(6, 12)))   # Korf's maximum, for front="table"

    table: uint8 device tensor [N(k)]; mask / edges: the tracked pieces; levels: patterns per distance (None for a wrapped tensor)."""
    cube_size = 3

    def __init__(self, table, edges, levels=None, cube_size=3):
        """Wrap a table built earlier.  ValueError for a tensor that cannot be one: wrong size, dtype or device are found before the
        device is touched, table[home] != 0 by reading one byte."""
        from . import _edge_lib
        if cube_size != 3:
            raise ValueError(f"edge tables exist for the 3x3x3 only (the 2x2x2 has no edges), got cube_size {cube_size!r}")
        self.mask = _edge_lib.edge_mask(edges)
        self.edges = tuple(e for e in range(_edge_lib.N_EDGES) if self.mask >> e & 1)
        _check_table(table, _edge_lib.table_bytes(self.mask), f"an edge table of the pieces {self.edges}")
        self.home = _edge_lib.home_index(self.mask)
        if levels is None and int(table[self.home]) != 0:
            raise ValueError(f"not an edge table of the pieces {self.edges}: table[{self.home}], the home pattern's distance, is not 0")
        self.table, self.device = table, table.device
        self.levels = None if levels is None else tuple(int(c) for c in levels)

    @classmethod
    def build(cls, edges, device="cuda", cube_size=3):
        """Breadth-first over the index space: rce_build_begin, then one rce_build_level per distance until a level sets nothing (the
        count is read back once per level)."""
        from . import _edge_lib
        if cube_size != 3:
            raise ValueError(f"edge tables exist for the 3x3x3 only (the 2x2x2 has no edges), got cube_size {cube_size!r}")
        mask = _edge_lib.edge_mask(edges)
        n = _edge_lib.table_bytes(mask)
        dev = _device(device)
        _lib.init(dev)
        L = _edge_lib.edge_lib()
        table = torch.empty(n, dtype=torch.uint8, device=dev)
        levels = _build_levels(lambda t, n, st: _lib.check(L.rce_build_begin(t, n, mask, st)),
                               lambda t, n, depth, count, st: _lib.check(L.rce_build_level(t, n, mask, depth, count, st)),
                               table, n, dev, lambda table: 1, f"the edge table of mask {mask:#x}")
        return cls(table, mask, levels)

    @property
    def depth(self):
        """The largest distance in the table (needs levels: a built table)."""
        return None if self.levels is None else len(self.levels) - 1

    def distance(self, cubes, n=None, pitch=None):
        """uint8 [N]: table[index] of every cube (one rce_lookup launch); ILLEGAL = 0xFF where the edge bytes are no pattern.  cubes: a
        VecCubeEnv (encoded to compact codes first), or a tiled RC_FMT_CODE / cubie buffer [tiles, 20, pitch] with n cubes (pitch
        None: its last dimension)."""
        from . import _edge_lib
        if hasattr(cubes, "stickers"):
            if cubes.cube_size != 3:
                raise ValueError(f"the table is a 3x3x3's, the cubes are {cubes.cube_size}x{cubes.cube_size}x{cubes.cube_size}")
            if cubes.stickers.device != self.device:
                raise ValueError(f"the table is on {self.device}, the cubes on {cubes.stickers.device}")
            n, pitch = cubes.num_envs, None
            code = ops.alloc_code(n, 3, self.device, cubes.stickers.shape[-1])
            ops.encode(cubes.stickers, n, 3, code, _lib.FMT_CODE)
            cubes = code
        if n is None:
            raise ValueError("distance(rows, n): the number of cubes is required for a code or cubie buffer")
        if cubes.device != self.device:
            raise ValueError(f"the table is on {self.device}, the cubes on {cubes.device}")
        p = ops._state_arg(cubes, 20, n, pitch, "distance rows")
        out = torch.empty(_lib.pitch_for(max(n, 1), 16), dtype=torch.uint8, device=self.device)[:n]
        _lib.init(self.device)
        _lib.check(_edge_lib.edge_lib().rce_lookup(ptr(cubes), n, p, self.mask, ptr(self.table), self.table.numel(), ptr(out),
                                                   stream_ptr(self.device)))
        return out

    def cubies(self, indices, out=None, cubie_pitch=None, bad=None):
        """rce_unrank: pattern indices (any integer tensor or sequence; values >= N are flagged) -> the cubie rows of a reachable cube
        with that pattern.  bad: the flag, a uint8 device tensor [1] the caller zeroes and reads; None: read back at once and raised
        as IndexError."""
        from . import _edge_lib
        buf, n = _index_buffer(indices, self.device)
        if out is None:
            out = ops.alloc_code(n, 3, self.device, cubie_pitch)
        p = ops._state_arg(out, 20, n, cubie_pitch, "cubies out")
        flag = torch.zeros(1, dtype=torch.uint8, device=self.device) if bad is None else ops._vec(bad, 1, torch.uint8, "cubies bad")
        _lib.init(self.device)
        _lib.check(_edge_lib.edge_lib().rce_unrank(ptr(buf), n, self.mask, ptr(out), p, ptr(flag), stream_ptr(self.device)))
        if bad is None and int(flag):
            raise IndexError(f"edge pattern index out of range 0..{self.table.numel() - 1}")
        return out

    def states(self, indices):
        """Tiled sticker states [tiles, S, pitch] of the patterns `indices` (rce_unrank, then ops.from_cubies): corners home, the
        untracked edges in ascending order, adjusted so that the cube is reachable."""
        cub = self.cubies(indices)
        return ops.from_cubies(cub, len(indices), 3, bad=torch.zeros(1, dtype=torch.uint8, device=self.device))

    def score_codes(self, code, n_problems, width, pitch, scores, combine=0):
        """rce_score_codes: over every slot of rc_search_expand's candidate code buffer, scores[j] = -table[index] (combine 0) or the
        lesser of that and what scores[j] holds (combine 1); -255 for an illegal row set."""
        from . import _edge_lib
        _lib.check(_edge_lib.edge_lib().rce_score_codes(ptr(code), n_problems, width, pitch, self.mask, ptr(self.table), self.table.numel(),
                                                        ptr(scores), int(combine), stream_ptr(self.device)))


class MaxTable:
    """The maximum of pattern databases, Korf's heuristic: MaxTable(corner, *edge_tables), corner a CornerTable of the 3x3x3 or None.
    Every member is admissible and consistent, so their maximum is; front="table" takes it wherever it takes a CornerTable.
    ValueError for no table at all, a member that is no table, or members on different devices -- before any launch."""
    cube_size = 3

    def __init__(self, corner=None, *edge_tables):
        if corner is not None and not isinstance(corner, CornerTable):
            raise ValueError(f"MaxTable(corner, *edge_tables): corner is a pattern.CornerTable or None, got {type(corner).__name__}")
        for e in edge_tables:
            if not isinstance(e, EdgeTable):
                raise ValueError(f"MaxTable(corner, *edge_tables): every further member is a pattern.EdgeTable, got {type(e).__name__}")
        if corner is not None and corner.cube_size != 3:
            raise ValueError(f"MaxTable is the 3x3x3's (the 2x2x2 has no edges); the corner table is a {corner.cube_size}x{corner.cube_size}x{corner.cube_size}'s")
        members = ([corner] if corner is not None else []) + list(edge_tables)
        if not members:
            raise ValueError("MaxTable needs at least one table")
        if any(m.device != members[0].device for m in members):
            raise ValueError(f"the tables of a MaxTable must live on one device, got {[str(m.device) for m in members]}")
        self.corner, self.edge_tables, self.device = corner, tuple(edge_tables), members[0].device

    def distance(self, env):
        """uint8 [N]: the element-wise maximum of the members' distances (0xFF, illegal, wins)."""
        parts = ([self.corner.distance(env)] if self.corner is not None else []) + [e.distance(env) for e in self.edge_tables]
        out = parts[0]
        for p in parts[1:]:
            out = torch.maximum(out, p)
        return out

    def score(self, keys, code, n_problems, width, pitch, scores):
        """scores = -max over the members, over every candidate slot: rcp_score_keys for the corner table (it writes), then one
        rce_score_codes(combine=1) per edge table; without a corner table the first edge table writes (combine=0)."""
        wrote = self.corner is not None
        if wrote:
            self.corner.score_keys(keys, n_problems, width, pitch, scores)
        for e in self.edge_tables:
            e.score_codes(code, n_problems, width, pitch, scores, combine=int(wrote))
            wrote = True


class ChainTables:
    """The four coset-distance tables of Thistlethwaite's subgroup chain (include/rubikhip.h "Subgroup chain", DESIGN.md "Subgroup
    chain"): <all> > <U,D,R,L,F2,B2> > <U,D,F2,R2,B2,L2> > <half turns> > {solved}.  3x3x3 only, 5.2 MB in all; search.chain_solve
    walks any legal cube home through them, without a net and without a search, in at most 87 quarter turns.

        chain = ChainTables.build("cuda")             # breadth-first, one launch per level
        chain.levels[2], chain.depth[2]               # cosets per distance of stage 2, its largest distance
        chain.distance(env, 0)                        # uint8 [N]: generators to stage 0's goal; 0xFF outside the stage's domain
        chain_solve(chain, env)["length"]

    tables: four uint8 device tensors [N(stage)]; levels / depth: per stage (None for wrapped tensors)."""
    cube_size = 3

    def __init__(self, tables, levels=None, cube_size=3):
        """Wrap tables built earlier.  ValueError for tensors that cannot be them: a wrong count, size, dtype or device -- found
        before the device is touched."""
        from . import _chain_lib
        if cube_size != 3:
            raise ValueError(f"the subgroup chain exists for the 3x3x3 only, got cube_size {cube_size!r}")
        tables = tuple(tables)
        if len(tables) != _chain_lib.STAGES:
            raise ValueError(f"a chain has {_chain_lib.STAGES} tables, got {len(tables)}")
        for s, t in enumerate(tables):
            _check_table(t, _chain_lib.table_bytes(s), f"the table of stage {s}", "the tables", "every table")
            if t.device != tables[0].device:
                raise ValueError(f"the tables of a chain must live on one device, got {[str(x.device) for x in tables]}")
        self.tables, self.device = tables, tables[0].device
        self.levels = None if levels is None else tuple(tuple(int(c) for c in lv) for lv in levels)

    @classmethod
    def build(cls, device="cuda", cube_size=3):
        """Breadth-first over each stage's index space: rct_build_begin, then one rct_build_level per distance until a level sets
        nothing (the count is read back once per level)."""
        from . import _chain_lib
        if cube_size != 3:
            raise ValueError(f"the subgroup chain exists for the 3x3x3 only, got cube_size {cube_size!r}")
        dev = _device(device)
        _lib.init(dev)
        L = _chain_lib.chain_lib()
        tables, levels = [], []
        for stage in range(_chain_lib.STAGES):
            n = _chain_lib.table_bytes(stage)
            tables.append(torch.empty(n, dtype=torch.uint8, device=dev))
            levels.append(_build_levels(lambda t, n, st: _lib.check(L.rct_build_begin(t, n, stage, st)),
                                        lambda t, n, depth, count, st: _lib.check(L.rct_build_level(t, n, stage, depth, count, st)),
                                        tables[-1], n, dev, lambda table: int((table == 0).sum()), f"the table of stage {stage}"))
        return cls(tables, levels)

    @property
    def depth(self):
        """The largest distance of each table (needs levels: built tables)."""
        return None if self.levels is None else tuple(len(lv) - 1 for lv in self.levels)

    def _cubie_arg(self, cubes, n, pitch, what):
        """(cubie buffer, n, pitch) of a VecCubeEnv (one rcc_cubies launch) or of a tiled cubie buffer [tiles, 20, pitch] with n cubes."""
        if hasattr(cubes, "stickers"):
            if cubes.cube_size != 3:
                raise ValueError(f"the chain is a 3x3x3's, the cubes are {cubes.cube_size}x{cubes.cube_size}x{cubes.cube_size}")
            if cubes.stickers.device != self.device:
                raise ValueError(f"the tables are on {self.device}, the cubes on {cubes.stickers.device}")
            n, pitch = cubes.num_envs, None
            cubes = ops.cubies(cubes.stickers, n, 3, status=False)["cubies"]
        if n is None:
            raise ValueError(f"{what}(cubies, stage, n): the number of cubes is required for a cubie buffer")
        if cubes.device != self.device:
            raise ValueError(f"the tables are on {self.device}, the cubes on {cubes.device}")
        return cubes, n, ops._state_arg(cubes, 20, n, pitch, f"{what} cubies")

    def index(self, cubes, stage, n=None, pitch=None):
        """int64 [N]: the stage's index of every cube (one rct_index launch), -1 for an illegal row set and for a cube outside the
        stage's domain.  cubes: a VecCubeEnv, or a tiled cubie buffer [tiles, 20, pitch] with n cubes."""
        from . import _chain_lib
        stage = _chain_lib.check_stage(stage)
        cubes, n, p = self._cubie_arg(cubes, n, pitch, "index")
        out = torch.empty(_lib.pitch_for(max(n, 1) * 4, 16) // 4, dtype=torch.int32, device=self.device)[:n]
        _lib.init(self.device)
        _lib.check(_chain_lib.chain_lib().rct_index(ptr(cubes), n, p, stage, ptr(out), stream_ptr(self.device)))
        return out.to(torch.int64)                             # all-ones, the uint32 of an int32 tensor, is -1

    def distance(self, cubes, stage, n=None, pitch=None):
        """uint8 [N]: the stage's generators between every cube and the stage's goal set, ILLEGAL = 0xFF where index() is -1 and for
        a stage-3 entry no cube has."""
        idx = self.index(cubes, stage, n, pitch)
        t = self.tables[stage]
        d = t[idx.clamp(0, t.numel() - 1)]
        return torch.where(idx < 0, torch.full_like(d, ILLEGAL), d)

    def cubies(self, indices, stage, out=None, cubie_pitch=None, bad=None):
        """rct_unrank: a stage's indices (any integer tensor or sequence) -> the cubie rows of a reachable cube of its domain with
        that index.  An index >= N and a stage-3 index of the wrong parity are flagged.  bad: the flag, a uint8 device tensor [1] the
        caller zeroes and reads; None: read back at once and raised as IndexError."""
        from . import _chain_lib
        stage = _chain_lib.check_stage(stage)
        buf, n = _index_buffer(indices, self.device)
        if out is None:
            out = ops.alloc_code(n, 3, self.device, cubie_pitch)
        p = ops._state_arg(out, 20, n, cubie_pitch, "cubies out")
        flag = torch.zeros(1, dtype=torch.uint8, device=self.device) if bad is None else ops._vec(bad, 1, torch.uint8, "cubies bad")
        _lib.init(self.device)
        _lib.check(_chain_lib.chain_lib().rct_unrank(ptr(buf), n, stage, ptr(out), p, ptr(flag), stream_ptr(self.device)))
        if bad is None and int(flag):
            raise IndexError(f"stage {stage}: an index is out of range 0..{self.tables[stage].numel() - 1} or names no cube")
        return out


class TwoPhaseTables:
    """The four coset-distance tables of Kociemba's two-phase algorithm (include/rubikhip.h "Two-phase", DESIGN.md "Two-phase"):
    0 twist-slice and 1 flip-slice over every cube under the 12 actions (phase 1), 2 corner-slice and 3 edge-slice over
    G1 = <U,D,F2,R2,B2,L2> under U, U', F2, R2, D, D', B2, L2 with a half turn costing 2 (phase 2).  3x3x3 only, 4.0 MB in all;
    search.two_phase_solve searches under them.

        tp = TwoPhaseTables.build("cuda")             # breadth-first, one launch per level
        tp.levels[2], tp.depth[2]                     # entries per distance of the corner-slice table, its largest distance
        tp.distance(0, env)                           # uint8 [N]: quarter turns to twist 0 and the slice edges in the slice
        two_phase_solve(tp, chain, env)["length"]

    tables: four uint8 device tensors [N(which)]; levels / depth: per table (None for wrapped tensors)."""
    cube_size = 3

    def __init__(self, tables, levels=None, cube_size=3):
        """Wrap tables built earlier.  ValueError for tensors that cannot be them: a wrong count, size, dtype or device -- found
        before the device is touched."""
        from . import _twophase_lib
        if cube_size != 3:
            raise ValueError(f"the two-phase tables exist for the 3x3x3 only, got cube_size {cube_size!r}")
        tables = tuple(tables)
        if len(tables) != _twophase_lib.TABLES:
            raise ValueError(f"two phases have {_twophase_lib.TABLES} tables, got {len(tables)}")
        for w, t in enumerate(tables):
            _check_table(t, _twophase_lib.table_bytes(w), f"table {w}", "the tables", "every table")
            if t.device != tables[0].device:
                raise ValueError(f"the two-phase tables must live on one device, got {[str(x.device) for x in tables]}")
        self.tables, self.device = tables, tables[0].device
        self.levels = None if levels is None else tuple(tuple(int(c) for c in lv) for lv in levels)

    @classmethod
    def build(cls, device="cuda", cube_size=3):
        """Breadth-first over each table's index space: tp_build_begin, then one tp_build_level per distance (the count is read back
        once per level) until a level sets nothing -- two levels in a row for the weighted tables 2 and 3."""
        from . import _twophase_lib
        if cube_size != 3:
            raise ValueError(f"the two-phase tables exist for the 3x3x3 only, got cube_size {cube_size!r}")
        dev = _device(device)
        _lib.init(dev)
        L = _twophase_lib.twophase_lib()
        count = torch.zeros(4, dtype=torch.int32, device=dev)  # one uint32, 16-byte aligned
        tables, levels = [], []
        for which in range(_twophase_lib.TABLES):
            n = _twophase_lib.table_bytes(which)
            t = torch.empty(n, dtype=torch.uint8, device=dev)
            _lib.check(L.tp_build_begin(ptr(t), n, which, stream_ptr(dev)))
            lv, empty = [1], 0
            for depth in range(MAX_LEVELS + 2):
                _lib.check(L.tp_build_level(ptr(t), n, which, depth, ptr(count), stream_ptr(dev)))
                lv.append(int(count[0]))
                empty = empty + 1 if lv[-1] == 0 else 0
                if empty == (2 if which >= 2 else 1):
                    break
            else:
                raise RuntimeError(f"two-phase table {which} has more than {MAX_LEVELS} levels")
            tables.append(t)
            levels.append(lv[:len(lv) - empty])
        return cls(tables, levels)

    @property
    def depth(self):
        """The largest distance of each table (needs levels: built tables)."""
        return None if self.levels is None else tuple(len(lv) - 1 for lv in self.levels)

    def _cubie_arg(self, cubes, n, pitch, what):
        """(cubie buffer, n, pitch) of a VecCubeEnv (one rcc_cubies launch) or of a tiled cubie buffer [tiles, 20, pitch] with n cubes."""
        if hasattr(cubes, "stickers"):
            if cubes.cube_size != 3:
                raise ValueError(f"the tables are a 3x3x3's, the cubes are {cubes.cube_size}x{cubes.cube_size}x{cubes.cube_size}")
            if cubes.stickers.device != self.device:
                raise ValueError(f"the tables are on {self.device}, the cubes on {cubes.stickers.device}")
            n, pitch = cubes.num_envs, None
            cubes = ops.cubies(cubes.stickers, n, 3, status=False)["cubies"]
        if n is None:
            raise ValueError(f"{what}(which, cubies, n): the number of cubes is required for a cubie buffer")
        if cubes.device != self.device:
            raise ValueError(f"the tables are on {self.device}, the cubes on {cubes.device}")
        return cubes, n, ops._state_arg(cubes, 20, n, pitch, f"{what} cubies")

    def index(self, which, cubes, n=None, pitch=None):
        """int64 [N]: table which's index of every cube (one tp_index launch), -1 for an illegal row set and for a cube outside the
        table's domain.  cubes: a VecCubeEnv, or a tiled cubie buffer [tiles, 20, pitch] with n cubes."""
        from . import _twophase_lib
        which = _twophase_lib.check_which(which)
        cubes, n, p = self._cubie_arg(cubes, n, pitch, "index")
        out = torch.empty(_lib.pitch_for(max(n, 1) * 4, 16) // 4, dtype=torch.int32, device=self.device)[:n]
        _lib.init(self.device)
        _lib.check(_twophase_lib.twophase_lib().tp_index(ptr(cubes), n, p, which, ptr(out), stream_ptr(self.device)))
        return out.to(torch.int64)                             # all-ones, the uint32 of an int32 tensor, is -1

    def distance(self, which, cubes, n=None, pitch=None):
        """uint8 [N]: table[index], ILLEGAL = 0xFF where index() is -1."""
        idx = self.index(which, cubes, n, pitch)
        t = self.tables[which]
        d = t[idx.clamp(0, t.numel() - 1)]
        return torch.where(idx < 0, torch.full_like(d, ILLEGAL), d)
