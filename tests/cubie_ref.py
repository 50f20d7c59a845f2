"""The cubie rule (include/rubikhip.h "Cubie coordinates") restated in numpy from the cube's geometry alone: the sticker positions and
normals of tables._sticker_geometry and the slot names.  Nothing here reads the generated header, tables.get_cubies or the library.

  corner byte  piece * 3 + ori, ori = clockwise steps (seen from outside) from the slot's U/D sticker to the piece's U/D colour
  edge byte    piece * 2 + ori, ori = 0 when the piece's first colour shows on the slot's first sticker
  0xFF         no cubie has the slot's colours
Clockwise here: b follows a clockwise around an outward corner exactly when a x b points INTO the cube along the third normal."""
import functools
import itertools

import numpy as np

from rubiks_cube_solver_amd import tables as T

BAD_COLOUR, BAD_FIXED, BAD_PIECE, DUP_PIECE, TWIST, FLIP, PARITY = 1, 2, 4, 8, 16, 32, 64
NONE = 0xFF
S_OF, A_OF = {2: 24, 3: 54}, {2: 6, 3: 12}


class Rule:
    def __init__(self, cs):
        geo = T._sticker_geometry(cs)
        normal = {f: T._NORMAL[f] for f in T.FACES}
        cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        neg = lambda a: tuple(-x for x in a)

        def sticker(faces, face):                                  # the sticker on `face` of the cubie that touches exactly `faces`
            hits = [i for i, (p, nm) in enumerate(geo) if nm == normal[face] and
                    {f for f in T.FACES if sum(a * b for a, b in zip(normal[f], p)) == cs - 1} == set(faces)]
            assert len(hits) == 1
            return hits[0]

        self.cs, self.S = cs, len(geo)
        corners = T.CORNER_SLOTS_3 if cs == 3 else T.CORNER_SLOTS_2
        edges = T.EDGE_SLOTS_3 if cs == 3 else []
        self.corner = []                                           # per slot: sticker indices, U/D first, then clockwise
        for name in corners:
            ud, a, b = name[0], name[1], name[2]
            assert ud in "UD"
            if cross(normal[ud], normal[a]) != neg(normal[b]):     # a does not follow ud clockwise: b does
                a, b = b, a
            assert cross(normal[ud], normal[a]) == neg(normal[b])
            self.corner.append([sticker(name, f) for f in (ud, a, b)])
        self.edge = [[sticker(name, f) for f in name] for name in edges]
        self.corner, self.edge = np.array(self.corner, np.int64).reshape(-1, 3), np.array(self.edge, np.int64).reshape(-1, 2)
        self.nc, self.ne = len(self.corner), len(self.edge)
        self.solved = np.repeat(np.arange(6, dtype=np.uint8), cs * cs)
        self.ccol, self.ecol = self.solved[self.corner], self.solved[self.edge]
        if cs == 3:
            self.fixed = np.array([9 * f + 4 for f in range(6)])
        else:
            self.fixed = np.array([sticker("DLB", f) for f in "DLB"])
        # colours (c0, c1, c2) -> byte, as a table over base-6 keys
        self.ckey = np.full(216, NONE, np.uint8)
        for p, col in enumerate(self.ccol):
            for o in range(3):
                seen = [col[(k - o) % 3] for k in range(3)]        # position k shows the piece's colour k - o
                self.ckey[seen[0] * 36 + seen[1] * 6 + seen[2]] = 3 * p + o
        self.ekey = np.full(36, NONE, np.uint8)
        for p, col in enumerate(self.ecol):
            self.ekey[col[0] * 6 + col[1]], self.ekey[col[1] * 6 + col[0]] = 2 * p, 2 * p + 1


@functools.lru_cache(maxsize=None)
def rule(cs):
    return Rule(cs)


def _sign(p):
    """Parity (0 even, 1 odd) of every row of p [n, k], rows being permutations of 0..k-1: k minus the number of cycles."""
    n, k = p.shape
    low = np.tile(np.arange(k), (n, 1))
    for _ in range(k):
        low = np.minimum(low, np.take_along_axis(low, p, axis=1))  # the smallest element of the cycle through i
    return (k - (low == np.arange(k)).sum(axis=1)) & 1


def _rank(p):
    """Lexicographic rank of every row of p [n, k] among the permutations of 0..k-1."""
    n, k = p.shape
    r = np.zeros(n, np.int64)
    for q in range(k):
        digit = p[:, q] - (p[:, :q] < p[:, q:q + 1]).sum(axis=1)   # how many unused values are smaller
        r = r * (k - q) + digit
    return r


def cubies(cs, states):
    """[n, S] -> (cubies uint8 [n, SLOTS], status uint8 [n], corner_index uint32 [n], edge_index uint64 [n] | None)."""
    R = rule(cs)
    st = np.asarray(states, np.uint8)
    n = len(st)
    c = st[:, R.corner]                                              # [n, NC, 3]; the keys wrap in uint8 only where `ok` is False
    ok = (c < 6).all(axis=2)
    cc = np.where(ok, R.ckey[np.where(ok, c[..., 0] * np.uint8(36) + c[..., 1] * np.uint8(6) + c[..., 2], 0)], np.uint8(NONE))
    e = st[:, R.edge]
    ok = (e < 6).all(axis=2)
    ee = np.where(ok, R.ekey[np.where(ok, e[..., 0] * np.uint8(6) + e[..., 1], 0)], np.uint8(NONE))
    cub = np.concatenate([cc, ee], axis=1)
    status = np.zeros(n, np.uint8)
    status[(st > 5).any(axis=1)] |= BAD_COLOUR
    status[(st[:, R.fixed] != R.solved[R.fixed]).any(axis=1)] |= BAD_FIXED
    status[(cub == NONE).any(axis=1)] |= BAD_PIECE

    def repeated(part, div):                                       # some piece named by two slots
        piece = np.where(part == NONE, np.uint8(100) + np.arange(part.shape[1], dtype=np.uint8), part // np.uint8(div))
        srt = np.sort(piece, axis=1)
        return (srt[:, 1:] == srt[:, :-1]).any(axis=1)
    status[repeated(cc, 3) | (repeated(ee, 2) if R.ne else False)] |= DUP_PIECE
    good = np.flatnonzero(status == 0)
    cidx = np.full(n, 0xFFFFFFFF, np.uint32)
    eidx = np.full(n, 0xFFFFFFFFFFFFFFFF, np.uint64) if R.ne else None
    cp, co = (cc[good] // np.uint8(3)).astype(np.int64), (cc[good] % np.uint8(3)).astype(np.int64)
    twist = co.sum(axis=1) % 3 != 0
    status[good[twist]] |= TWIST
    if R.ne:
        ep, eo = ee[good].astype(np.int64) // 2, ee[good].astype(np.int64) % 2
        status[good[eo.sum(axis=1) % 2 != 0]] |= FLIP
        status[good[_sign(cp) != _sign(ep)]] |= PARITY
    legal = status[good] == 0
    g = good[legal]
    cidx[g] = (_rank(cp[legal]) * 3 ** (R.nc - 1) + (co[legal][:, :R.nc - 1] * 3 ** np.arange(R.nc - 1)).sum(axis=1)).astype(np.uint32)
    if R.ne:
        eidx[g] = (_rank(ep[legal]) * 2048 + (eo[legal][:, :11] * 2 ** np.arange(11)).sum(axis=1)).astype(np.uint64)
    return cub, status, cidx, eidx


def from_cubies(cs, cub):
    """[n, SLOTS] -> (states [n, S], bad bool [n]): any (piece, ori) per slot as given; a cube with an unnameable byte comes out solved."""
    R = rule(cs)
    cub = np.asarray(cub, np.uint8)
    n = len(cub)
    bad = (cub[:, :R.nc] >= 3 * R.nc).any(axis=1) | (cub[:, R.nc:] >= 2 * R.ne).any(axis=1)
    st = np.tile(R.solved, (n, 1))
    home = np.array([3 * q for q in range(R.nc)] + [2 * q for q in range(R.ne)], np.uint8)
    c = np.where(bad[:, None], home, cub)                            # a flagged cube is assembled from its home bytes: solved
    for q in range(R.nc):
        piece, ori = c[:, q] // np.uint8(3), c[:, q] % np.uint8(3)
        for k in range(3):
            st[:, R.corner[q][k]] = R.ccol[piece, (np.uint8(k + 3) - ori) % np.uint8(3)]      # position k shows the piece's colour k - ori
    for q in range(R.ne):
        piece, ori = c[:, R.nc + q] // np.uint8(2), c[:, R.nc + q] % np.uint8(2)
        for k in range(2):
            st[:, R.edge[q][k]] = R.ecol[piece, (np.uint8(k + 2) - ori) % np.uint8(2)]
    return st, bad


# ------------------------------------------------------------------------------------------------- the cases the tests share
def classes(cs):
    """(t, f, p): twist corner 0 by t, flip edge 0 by f, swap edges 0 and 1 by p.  3x3x3: twelve, eleven of them illegal."""
    return list(itertools.product((0, 1, 2), (0, 1), (0, 1))) if cs == 3 else [(t, 0, 0) for t in (0, 1, 2)]


def class_status(t, f, p):
    return (TWIST if t else 0) | (FLIP if f else 0) | (PARITY if p else 0)


def mutate(cs, cub, t, f, p):
    R = rule(cs)
    c = np.array(cub, np.uint8)
    c[:, 0] = c[:, 0] // 3 * 3 + (c[:, 0] % 3 + t) % 3
    if f:
        c[:, R.nc] ^= 1
    if p:
        c[:, [R.nc, R.nc + 1]] = c[:, [R.nc + 1, R.nc]]
    return c


def low_bit_cases(cs, state):
    """One constructed state for each of the bits 1, 2, 4, 8 (from one legal state) -> [(bit, state)].  Every one also sets no bit above 8."""
    R = rule(cs)
    out = []
    s = state.copy(); s[R.corner[0][0]] = 6; out.append((BAD_COLOUR, s))                                   # (also BAD_PIECE: that slot reads 0xFF)
    s = state.copy(); s[R.fixed[0]] = (s[R.fixed[0]] + 1) % 6; out.append((BAD_FIXED, s))
    s = state.copy(); s[R.corner[1][[1, 2]]] = s[R.corner[1][[2, 1]]]; out.append((BAD_PIECE, s))          # a mirror-image corner
    cub = cubies(cs, state[None])[0]
    cub[0, 1] = cub[0, 0]                                                                                  # slot 1 repeats slot 0's piece
    out.append((DUP_PIECE, from_cubies(cs, cub)[0][0]))
    return out


def walks(oracle, cs, n, depth, seed):
    """[n, S] states after `depth` random oracle moves from solved (the same for every caller of one seed)."""
    rng = np.random.default_rng(seed)
    st = oracle.solved(cs, n)
    for _ in range(depth):
        st = oracle.step(cs, st, rng.integers(0, A_OF[cs], n).astype(np.uint8))[0]
    return st
