"""Cube tables: the single source of truth for the HIP kernels, the C-ABI and the facade.

Nothing here is a transcription of the reference's 12x54 table.  The sticker
permutations are DERIVED from cube geometry given only the reference's sticker
numbering and colour order (docstring of gym-cube/gym_cube/envs/assets/py333.py:3-19:
faces in the order U,R,F,D,L,B, nine stickers per face numbered row-major as seen on
the unfolded net, colour of a face = its index) and the gather convention
``new[i] = old[perm[a][i]]`` (py333.py:220-222).  tests/test_tables.py checks the result
against the reference's own table captured in tests/golden/tables_333.npz.

What cannot be derived is restated as data, citing where it comes from:
  * the order of the 8 corner / 12 edge slots and of the stickers inside each slot
    (py333.py:140-164), written here as face-letter strings;
  * the hash -> (piece, orientation) look-up tables (py333.py:171-198), INCLUDING the
    reference's wrong / missing corner entries: rows never assigned stay (0, 0).
    Reproducing them is required for bit-exact one-hot states.

2x2x2: the reference imports ``assets.py222`` (cube_env.py:8) but does not ship it
 -> PARITY UNPINNED for 2x2x2 values.  We follow the published
algorithm of the public MeepMoop/py222 solver (no version is pinned by the reference):
24 stickers numbered like the 3x3x3 net, the DLB cubie fixed, moves U,U',F,F',R,R'
(cube_env.py:25), 7 piece slots, hash c0+2*c1+10*c2, orientation k = colour triple
rotated right k times.  The six permutations equal the corner-sticker restriction of
the 3x3x3 ones (asserted in tests).
"""
from __future__ import annotations

import functools
import itertools
import math
from dataclasses import dataclass

import numpy as np

FACES = "URFDLB"  # face order == colour order (py333.py:12-19)
_NORMAL = {
    "U": (0, 1, 0), "D": (0, -1, 0),
    "R": (1, 0, 0), "L": (-1, 0, 0),
    "F": (0, 0, 1), "B": (0, 0, -1),
}

# action order of the env API (cube_env.py:24-28, py333.py:41-44)
ACTION_NAMES = {
    2: ["U", "U'", "F", "F'", "R", "R'"],
    3: ["U", "U'", "F", "F'", "R", "R'", "D", "D'", "B", "B'", "L", "L'"],
}
# get_env_config (utils.py:162-186)
STATE_DIM = {2: (7, 21), 3: (20, 24)}
ACTION_DIM = {2: 6, 3: 12}

# slot order and sticker order inside a slot, as face letters (first letter = the
# sticker that is hashed with weight 1).  3x3x3: py333.py:140-164.
CORNER_SLOTS_3 = ["UBL", "ULF", "UFR", "URB", "DLB", "DFL", "DFR", "DBR"]
EDGE_SLOTS_3 = ["UB", "UL", "UF", "UR", "DB", "DL", "DF", "DR", "FL", "FR", "BR", "BL"]
# 2x2x2 (public py222 pieceDefs): DLB is the fixed cubie and has no slot.
CORNER_SLOTS_2 = ["UBL", "ULF", "UFR", "URB", "DFL", "DRF", "DBR"]

CORNER_HASH = (1, 2, 10)  # py333.py:167
EDGE_HASH = (1, 10)  # py333.py:168

# hash -> (piece, orientation), exactly the rows the reference assigns (py333.py:172-180);
# every other row of the 62-row table is (0, 0).
_CORNER_LUT_3 = {
    50: (0, 0), 54: (0, 1), 13: (0, 2), 28: (1, 0), 8: (1, 1), 42: (1, 2),
    14: (2, 0), 5: (2, 1), 12: (2, 2), 52: (3, 0), 11: (3, 1), 15: (3, 2),
    61: (4, 0), 44: (4, 1), 51: (4, 2), 47: (5, 0), 30: (5, 1), 40: (5, 2),
    17: (6, 0), 35: (6, 1), 18: (6, 2), 23: (7, 0), 56: (7, 1), 21: (7, 2),
}
_CORNER_LUT_3_ROWS = 62
# py333.py:184-198 (55-row table)
_EDGE_LUT_3 = {
    50: (0, 0), 5: (0, 1), 40: (1, 0), 4: (1, 1), 20: (2, 0), 2: (2, 1),
    10: (3, 0), 1: (3, 1), 53: (4, 0), 35: (4, 1), 43: (5, 0), 34: (5, 1),
    23: (6, 0), 32: (6, 1), 13: (7, 0), 31: (7, 1), 42: (8, 0), 24: (8, 1),
    12: (9, 0), 21: (9, 1), 15: (10, 0), 51: (10, 1), 45: (11, 0), 54: (11, 1),
}
_EDGE_LUT_3_ROWS = 55
_CORNER_LUT_2_ROWS = 58  # public py222: pieceInds = zeros([58, 2])

LUT_PAD = 72  # device LUTs are padded to 72 bytes (9 groups of 8) ; rows >= table size -> 0


# --------------------------------------------------------------------------- geometry
def _coords(n: int):
    return [2 * k - (n - 1) for k in range(n)]


def _sticker_geometry(n: int):
    """For every sticker index: (cubie position, outward normal), doubled integer coords.

    Row-major numbering of each face as drawn on the net of py333.py:3-11 (U on top,
    L F R B in a row, D below)."""
    v = _coords(n)
    geo = []
    for f in FACES:
        for r in range(n):
            for c in range(n):
                top = v[n - 1 - r]
                if f == "U":
                    p = (v[c], n - 1, v[r])
                elif f == "D":
                    p = (v[c], -(n - 1), v[n - 1 - r])
                elif f == "F":
                    p = (v[c], top, n - 1)
                elif f == "B":
                    p = (v[n - 1 - c], top, -(n - 1))
                elif f == "R":
                    p = (n - 1, top, v[n - 1 - c])
                else:  # L
                    p = (-(n - 1), top, v[c])
                geo.append((p, _NORMAL[f]))
    return geo


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _rot_cw(axis, vec):
    """Quarter turn, clockwise when looking at the face whose outward normal is `axis`
    (= -90 degrees about `axis` by the right-hand rule): v' = n(n.v) - n x v."""
    d = sum(a * b for a, b in zip(axis, vec))
    cr = _cross(axis, vec)
    return tuple(axis[i] * d - cr[i] for i in range(3))


def _face_turn(n: int, face: str) -> np.ndarray:
    geo = _sticker_geometry(n)
    where = {g: i for i, g in enumerate(geo)}
    axis = _NORMAL[face]
    perm = np.arange(len(geo))
    for j, (p, nm) in enumerate(geo):
        if sum(a * b for a, b in zip(axis, p)) == n - 1:  # cubie in the turning layer
            i = where[(_rot_cw(axis, p), _rot_cw(axis, nm))]
            perm[i] = j  # the sticker that was at j is now at i: new[i] = old[j]
    return perm


def _slot_stickers(n: int, slots):
    """Sticker indices of each slot: the cubie shared by the named faces; sticker k lies
    on the face named by letter k."""
    geo = _sticker_geometry(n)
    out = []
    for name in slots:
        row = []
        for letter in name:
            hits = [
                i for i, (p, nm) in enumerate(geo)
                if nm == _NORMAL[letter]
                and {l for l in FACES if sum(a * b for a, b in zip(_NORMAL[l], p)) == n - 1}
                == set(name)
            ]
            assert len(hits) == 1, (name, letter, hits)
            row.append(hits[0])
        out.append(row)
    return np.array(out, dtype=np.uint8)


# ------------------------------------------------------------------------------ tables
@dataclass(frozen=True)
class CubeTables:
    cube_size: int
    n_stickers: int  # S
    n_actions: int  # A
    action_names: tuple
    perm: np.ndarray  # uint8 [A][S]   new[i] = old[perm[a][i]]
    solved: np.ndarray  # uint8 [S]
    corner_defs: np.ndarray  # uint8 [n_corner_slots][3]
    edge_defs: np.ndarray  # uint8 [n_edge_slots][2]  (empty for 2x2x2)
    corner_lut: np.ndarray  # uint8 [rows][2]  (piece, ori), reference layout
    edge_lut: np.ndarray  # uint8 [rows][2]
    corner_code: np.ndarray  # uint8 [LUT_PAD]  piece*3+ori ; 0 beyond the table
    edge_code: np.ndarray  # uint8 [LUT_PAD]  piece*2+ori
    state_dim: tuple  # one-hot shape (R, C)
    n_slots: int  # compact code bytes per cube (20 | 7)

    @property
    def face_size(self):
        return self.cube_size * self.cube_size


def _lut_array(entries, rows):
    t = np.zeros((rows, 2), np.uint8)
    for h, (p, o) in entries.items():
        t[h] = (p, o)
    return t


def _code_array(lut, mult):
    c = np.zeros(LUT_PAD, np.uint8)
    c[: len(lut)] = lut[:, 0] * mult + lut[:, 1]
    return c


@functools.lru_cache(maxsize=None)
def get_tables(cube_size: int) -> CubeTables:
    if cube_size not in (2, 3):
        raise NotImplementedError(f"cube_size {cube_size}")  # cube_env.py:44
    n = cube_size
    names = ACTION_NAMES[n]
    turns = {f: _face_turn(n, f) for f in "UFRDBL"}
    perm = []
    for nm in names:
        p = turns[nm[0]]
        if nm.endswith("'"):
            p = np.argsort(p)  # inverse permutation
        perm.append(p)
    perm = np.array(perm, dtype=np.uint8)
    solved = np.repeat(np.arange(6, dtype=np.uint8), n * n)  # py333.py:211-218
    if n == 3:
        cdefs = _slot_stickers(3, CORNER_SLOTS_3)
        edefs = _slot_stickers(3, EDGE_SLOTS_3)
        clut = _lut_array(_CORNER_LUT_3, _CORNER_LUT_3_ROWS)
        elut = _lut_array(_EDGE_LUT_3, _EDGE_LUT_3_ROWS)
    else:
        cdefs = _slot_stickers(2, CORNER_SLOTS_2)
        edefs = np.zeros((0, 2), np.uint8)
        ent = {}
        for piece, d in enumerate(cdefs):
            col = [int(solved[i]) for i in d]
            for ori in range(3):  # colour triple rotated right `ori` times
                c = col[-ori:] + col[:-ori] if ori else col
                ent[sum(w * x for w, x in zip(CORNER_HASH, c))] = (piece, ori)
        assert len(ent) == 21
        clut = _lut_array(ent, _CORNER_LUT_2_ROWS)
        elut = np.zeros((1, 2), np.uint8)
    for a in range(0, len(names), 2):  # X' undoes X
        assert (perm[a][perm[a + 1]] == np.arange(perm.shape[1])).all()
    return CubeTables(
        cube_size=n, n_stickers=6 * n * n, n_actions=len(names), action_names=tuple(names),
        perm=perm, solved=solved, corner_defs=cdefs, edge_defs=edefs,
        corner_lut=clut, edge_lut=elut,
        corner_code=_code_array(clut, 3), edge_code=_code_array(elut, 2),
        state_dim=STATE_DIM[n], n_slots=len(cdefs) + len(edefs),
    )


# ------------------------------------------------------ pair-indexed code tables (device look-ups)
# sigma id of a reading order (j0, j1, j2) of a corner slot's three stickers, as rc_device.h numbers them
SIGMAS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


@functools.lru_cache(maxsize=None)
def pair_tables(cube_size: int):
    """Code look-ups indexed by TWO colours instead of the hash (the kernels' v_perm tables have 8 entries: a row per second
    colour, the first colour selects inside the row).

    edge_pair[c1][c0] = edge_code[c0 + 10*c1]: the hash is injective in (c0, c1), so this is exact for ANY colouring.
    Corners: on states reachable from the solved cube the first two colours of a slot read in a fixed order determine the
    third (a cubie is a fixed colour triple and a slot reads it in a fixed handedness), so
    corner_pair[table][c1][c0] = corner_code[c0 + 2*c1 + 10*c2(c0, c1)] -- including the reference's missing rows (zeros).
    The handedness depends on the slot and on the reading order: corner_table[q][sigma] names the table of slot q read in
    order SIGMAS[sigma].  Built by enumeration: random walks from the solved cube visit all 24 (21) triples of every slot; the
    generator asserts that (c0, c1) determines c2 and that walks of twice the length find nothing new.
    Returns (edge_pair uint8 [6][8], corner_pair uint8 [K][6][8], corner_table uint8 [NC][6])."""
    t = get_tables(cube_size)
    rng = np.random.default_rng(20260 + cube_size)
    A = t.n_actions
    seen = [set() for _ in t.corner_defs]
    st = np.tile(t.solved, (4096, 1))
    for step in range(60):
        acts = rng.integers(0, A, len(st))
        st = np.stack([s[t.perm[a]] for s, a in zip(st, acts)]) if step == 0 else st[np.arange(len(st))[:, None], t.perm[acts]]
        for q, d in enumerate(t.corner_defs):
            seen[q].update(map(tuple, st[:, d].tolist()))
        if step == 29:
            counts = [len(x) for x in seen]
    assert counts == [len(x) for x in seen] and set(counts) == {3 * (8 if cube_size == 3 else 7)}, counts
    tables, index = [], np.zeros((len(t.corner_defs), 6), np.uint8)
    for q in range(len(t.corner_defs)):
        for sid, sg in enumerate(SIGMAS):
            tab = np.zeros((6, 8), np.uint8)
            third = {}
            for tri in seen[q]:
                c0, c1, c2 = tri[sg[0]], tri[sg[1]], tri[sg[2]]
                assert third.setdefault((c0, c1), c2) == c2          # two colours determine the third
                h = c0 + 2 * c1 + 10 * c2
                tab[c1][c0] = t.corner_code[h] if h < LUT_PAD else 0
            for k, have in enumerate(tables):
                if (have == tab).all():
                    index[q, sid] = k
                    break
            else:
                index[q, sid] = len(tables)
                tables.append(tab)
    epair = np.zeros((6, 8), np.uint8)
    if len(t.edge_defs):
        for c1 in range(6):
            for c0 in range(6):
                epair[c1][c0] = t.edge_code[c0 + 10 * c1]
    return epair, np.stack(tables), index


# ------------------------------------------------------------------------------------------- symmetries
@dataclass(frozen=True)
class CubeSymmetries:
    """The whole-cube symmetries of one cube size (get_symmetries).  image[i] = relabel[s][state[perm[s][i]]]."""
    cube_size: int
    count: int  # K: 48 (3x3x3), 6 (2x2x2: the symmetries that fix the DLB cubie)
    matrix: np.ndarray  # int8 [K][3][3]  signed permutation matrices M
    perm: np.ndarray  # uint8 [K][S]   the sticker j whose (position, normal) M maps onto those of sticker i (a gather, like the moves)
    relabel: np.ndarray  # uint8 [K][6]   the face whose normal is M times the normal of face c
    amap: np.ndarray  # uint8 [K][A+1] T_s(move_a(x)) == move_{amap[s][a]}(T_s(x)); amap[s][A] = A (the no-op)
    det: np.ndarray  # int8 [K]  +1 rotations (first), -1 reflections
    inverse: np.ndarray  # uint8 [K]
    compose: np.ndarray  # uint8 [K][K]  compose[s][u] = apply s, then u

    def apply(self, states, s):
        """[n, S] sticker rows -> their images under symmetry s (an int, or one index per row).  The rule in numpy."""
        st = np.asarray(states, np.uint8)
        s = np.broadcast_to(np.asarray(s, np.int64), (len(st),))
        return self.relabel[s[:, None], np.take_along_axis(st, self.perm[s].astype(np.int64), axis=1)]


@functools.lru_cache(maxsize=None)
def get_symmetries(cube_size: int) -> CubeSymmetries:
    """The symmetries of the cube as a rigid body: every signed permutation matrix M (rotations and reflections of the coordinate
    axes), followed by the recolouring that turns the solved cube's image back into the solved cube.  The 2x2x2 env never moves the
    DLB cubie, so it keeps the M that fix that cubie's position (-1, -1, -1).  Order: permutations of the axes in
    itertools.permutations order, signs in itertools.product((1, -1)) order, M[r][p[r]] = sg[r]; then stably det = +1 first, so the
    identity is index 0 and the first half are the rotations."""
    if cube_size not in (2, 3):
        raise NotImplementedError(f"cube_size {cube_size}")
    n = cube_size
    mats = []
    for p in itertools.permutations(range(3)):
        for sg in itertools.product((1, -1), repeat=3):
            M = np.zeros((3, 3), np.int64)
            for r in range(3):
                M[r, p[r]] = sg[r]
            if n == 2 and tuple(M @ np.array([-1, -1, -1])) != (-1, -1, -1):
                continue
            mats.append(M)
    dets = [int(round(np.linalg.det(M))) for M in mats]
    order = sorted(range(len(mats)), key=lambda k: dets[k] != 1)  # sorted() is stable
    mats, dets = [mats[k] for k in order], [dets[k] for k in order]
    geo = _sticker_geometry(n)
    where = {g: i for i, g in enumerate(geo)}
    face_of = {v: k for k, v in enumerate(_NORMAL[f] for f in FACES)}
    names = ACTION_NAMES[n]
    A = len(names)
    mv = lambda M, v: tuple(int(x) for x in M @ np.array(v))
    perm = np.zeros((len(mats), len(geo)), np.uint8)
    relabel = np.zeros((len(mats), 6), np.uint8)
    amap = np.full((len(mats), A + 1), A, np.uint8)
    for s, M in enumerate(mats):
        for j, (pos, nm) in enumerate(geo):
            perm[s, where[(mv(M, pos), mv(M, nm))]] = j
        for c, f in enumerate(FACES):
            relabel[s, c] = face_of[mv(M, _NORMAL[f])]
        for a, nm in enumerate(names):
            face = FACES[face_of[mv(M, _NORMAL[nm[0]])]]
            prime = nm.endswith("'") != (dets[s] < 0)  # a reflection turns clockwise into counter-clockwise
            amap[s, a] = names.index(face + ("'" if prime else ""))
    index = {M.tobytes(): s for s, M in enumerate(mats)}
    compose = np.array([[index[(Mu @ Ms).tobytes()] for Mu in mats] for Ms in mats], np.uint8)
    inverse = np.array([index[np.ascontiguousarray(M.T).tobytes()] for M in mats], np.uint8)  # orthogonal: the inverse is the transpose
    return CubeSymmetries(cube_size=n, count=len(mats), matrix=np.array(mats, np.int8), perm=perm, relabel=relabel, amap=amap,
                          det=np.array(dets, np.int8), inverse=inverse, compose=compose)


def get_env_config(cube_size: int = 3):
    """([rows, cols] of the one-hot state, number of actions) -- utils.py:162-186."""
    if cube_size not in (2, 3):
        raise NotImplementedError(f"cube_size {cube_size}")
    return list(STATE_DIM[cube_size]), ACTION_DIM[cube_size]


# ------------------------------------------------------------------------------------------- cubie coordinates
# THE RULE (include/rubikhip.h "Cubie coordinates", rcc_*).  Slots and pieces are numbered as CORNER_SLOTS_* / EDGE_SLOTS_3 (corner_defs
# / edge_defs): piece q is the cubie that sits in slot q of the solved cube.  One byte per slot, corner slots first:
#   edge    piece * 2 + ori   ori = 0 when the piece's first colour shows on the slot's first sticker (edge_defs order): RC_FMT_CODE's byte;
#   corner  piece * 3 + ori   ori = clockwise steps, seen from outside the cube looking at the corner, from the slot's U/D sticker to the
#                             sticker that shows the piece's U/D colour.  The handedness of a slot comes from the geometry
#                             (_sticker_geometry), not from the listing order of corner_defs -- so this is NOT RC_FMT_CODE's corner byte;
#   0xFF    the slot's colours are no cubie (equal or opposite colours, a mirror-image corner, a value above 5).
# status (one byte per cube) is 0 exactly when the state can be reached from solved by the env's moves:
RCC_BAD_COLOUR, RCC_BAD_FIXED, RCC_BAD_PIECE, RCC_DUP_PIECE, RCC_TWIST, RCC_FLIP, RCC_PARITY = 1, 2, 4, 8, 16, 32, 64
RCC_NAMES = {RCC_BAD_COLOUR: "RCC_BAD_COLOUR", RCC_BAD_FIXED: "RCC_BAD_FIXED", RCC_BAD_PIECE: "RCC_BAD_PIECE", RCC_DUP_PIECE: "RCC_DUP_PIECE",
             RCC_TWIST: "RCC_TWIST", RCC_FLIP: "RCC_FLIP", RCC_PARITY: "RCC_PARITY"}
#   1 a sticker above 5; 2 a sticker the moves never touch (centres; the DLB cubie of the 2x2x2) differs from solved; 4 a slot reads 0xFF;
#   8 a piece occurs twice (among the slots that name one); and, evaluated only when bits 1..8 are clear: 16 the corner oris do not
#   sum to 0 mod 3; 32 the edge oris sum to an odd number; 64 corner- and edge-permutation parities differ (32, 64: 3x3x3 only).
# corner_index = lehmer(corner pieces) * 3^(NC-1) + sum_{q < NC-1} ori[q] * 3^q, lehmer = sum_q #{r > q: piece[r] < piece[q]} * (NC-1-q)!;
# edge_index = lehmer(edge pieces) * 2^11 + sum_{q < 11} ori[q] * 2^q; both all-ones when status != 0.
RCC_NO_CUBIE = 0xFF
RCC_NO_INDEX32, RCC_NO_INDEX64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def rcc_status_names(status: int):
    return [name for bit, name in RCC_NAMES.items() if status & bit]


@dataclass(frozen=True)
class CubieTables:
    cube_size: int
    nc: int
    ne: int
    corner_cw: np.ndarray  # uint8 [NC][3]  the slot's stickers clockwise seen from outside, the U/D sticker first
    edge_facelets: np.ndarray  # uint8 [NE][2]  = edge_defs
    corner_colours: np.ndarray  # uint8 [NC][3]  colours of piece p in the order of corner_cw[p]
    edge_colours: np.ndarray  # uint8 [NE][2]
    fixed: np.ndarray  # sticker indices no move touches: the 6 centres | the 3 stickers of DLB
    solved: np.ndarray  # uint8 [S]
    # the device look-ups (rc_tables.h): row = second colour, byte = first colour, 0xFF (0x0F for `third`) where no cubie has them
    corner_pair: np.ndarray  # uint8 [6][8]  piece * 4 + ori by the colours at corner_cw positions 0, 1
    corner_third: np.ndarray  # uint8 [6][8]  the colour such a cubie shows at position 2
    edge_pair: np.ndarray  # uint8 [6][8]  piece * 2 + ori by the colours at the slot's two stickers
    corner_sticker: np.ndarray  # uint8 [3][24]  colour at corner_cw position k of a slot whose byte is `code` (0xFF beyond 3 * NC)
    edge_sticker: np.ndarray  # uint8 [2][24]

    @property
    def n_slots(self):
        return self.nc + self.ne

    def cubies(self, states):
        """[n, S] sticker rows -> (cubies uint8 [n, SLOTS], status uint8 [n], corner_index uint32 [n], edge_index uint64 [n] | None)."""
        st = np.asarray(states, np.uint8)
        n, nc, ne = len(st), self.nc, self.ne
        cub = np.full((n, nc + ne), RCC_NO_CUBIE, np.uint8)
        seen = st[:, self.corner_cw.astype(np.int64)]                                    # [n, NC, 3]
        for p in range(nc):
            for o in range(3):
                hit = (seen == np.roll(self.corner_colours[p], o)).all(axis=2)          # colour a_k shows at position (k + o) % 3
                cub[:, :nc][hit] = 3 * p + o
        if ne:
            seen = st[:, self.edge_facelets.astype(np.int64)]
            for p in range(ne):
                for o in range(2):
                    hit = (seen == np.roll(self.edge_colours[p], o)).all(axis=2)
                    cub[:, nc:][hit] = 2 * p + o
        named = cub != RCC_NO_CUBIE
        cp, co = np.where(named[:, :nc], cub[:, :nc] // 3, 0).astype(np.int64), np.where(named[:, :nc], cub[:, :nc] % 3, 0).astype(np.int64)
        ep, eo = np.where(named[:, nc:], cub[:, nc:] // 2, 0).astype(np.int64), np.where(named[:, nc:], cub[:, nc:] % 2, 0).astype(np.int64)

        def twice(piece, ok, count):
            hist = np.zeros((n, count + 1), np.int64)
            np.add.at(hist, (np.arange(n)[:, None], np.where(ok, piece, count)), 1)
            return (hist[:, :count] > 1).any(axis=1)

        def lehmer(piece):                                                               # (value, parity of the permutation)
            k = piece.shape[1]
            cnt = np.stack([(piece[:, q + 1:] < piece[:, q:q + 1]).sum(axis=1) for q in range(k)], axis=1) if k else np.zeros((n, 0), np.int64)
            fact = np.array([int(np.prod(np.arange(1, k - q, dtype=np.int64))) for q in range(k)], np.int64)
            return (cnt * fact).sum(axis=1), cnt.sum(axis=1) & 1

        status = np.zeros(n, np.uint8)
        status |= np.uint8(RCC_BAD_COLOUR) * (st > 5).any(axis=1)
        status |= np.uint8(RCC_BAD_FIXED) * (st[:, self.fixed] != self.solved[self.fixed]).any(axis=1)
        status |= np.uint8(RCC_BAD_PIECE) * (~named).any(axis=1)
        status |= np.uint8(RCC_DUP_PIECE) * (twice(cp, named[:, :nc], nc) | (twice(ep, named[:, nc:], ne) if ne else False))
        clean = status == 0
        clehmer, cpar = lehmer(cp)
        status |= np.uint8(RCC_TWIST) * (clean & (co.sum(axis=1) % 3 != 0))
        cidx = clehmer * 3 ** (nc - 1) + (co[:, :nc - 1] * 3 ** np.arange(nc - 1)).sum(axis=1)
        eidx = None
        if ne:
            elehmer, epar = lehmer(ep)
            status |= np.uint8(RCC_FLIP) * (clean & (eo.sum(axis=1) % 2 != 0))
            status |= np.uint8(RCC_PARITY) * (clean & (cpar != epar))
            eidx = (elehmer * 2 ** (ne - 1) + (eo[:, :ne - 1] << np.arange(ne - 1)).sum(axis=1)).astype(np.uint64)
            eidx[status != 0] = RCC_NO_INDEX64
        cidx = cidx.astype(np.uint32)
        cidx[status != 0] = RCC_NO_INDEX32
        return cub, status, cidx, eidx

    def from_cubies(self, cubies):
        """[n, SLOTS] cubie bytes -> (states uint8 [n, S], bad bool [n]).  Any (piece, ori) per slot is written as given -- a twisted
        corner, a repeated piece; a cube with a byte that names none is written as solved and flagged."""
        cub = np.asarray(cubies, np.uint8)
        n, nc = len(cub), self.nc
        bad = (cub[:, :nc] >= 3 * nc).any(axis=1) | (cub[:, nc:] >= 2 * self.ne).any(axis=1)
        st = np.tile(self.solved, (n, 1))
        home = np.array([3 * q for q in range(nc)] + [2 * q for q in range(self.ne)], np.uint8)      # the solved cube's bytes
        safe = np.where(bad[:, None], home, cub)
        for q in range(nc):
            for k in range(3):
                st[:, self.corner_cw[q][k]] = self.corner_sticker[k][safe[:, q]]
        for q in range(self.ne):
            for k in range(2):
                st[:, self.edge_facelets[q][k]] = self.edge_sticker[k][safe[:, nc + q]]
        return st, bad


@functools.lru_cache(maxsize=None)
def get_cubies(cube_size: int) -> CubieTables:
    """The cubie tables of one cube size and the rule above in numpy (CubieTables.cubies / from_cubies)."""
    t = get_tables(cube_size)
    n = cube_size
    geo = _sticker_geometry(n)
    cw = []
    for d in t.corner_defs:
        n0, n1, n2 = (geo[i][1] for i in d)
        assert n0[1] != 0                                                    # the slot's first sticker is its U/D sticker
        det = sum(a * b for a, b in zip(n0, _cross(n1, n2)))                 # +1: (n0, n1, n2) runs counter-clockwise seen from outside
        cw.append([d[0], d[1], d[2]] if det < 0 else [d[0], d[2], d[1]])
    cw = np.array(cw, np.uint8)
    ccol, ecol = t.solved[cw], (t.solved[t.edge_defs] if len(t.edge_defs) else np.zeros((0, 2), np.uint8))
    moved = np.zeros(t.n_stickers, bool)
    for p in t.perm:
        moved |= p != np.arange(t.n_stickers)
    nc, ne = len(cw), len(t.edge_defs)
    cpair, cthird, epair = np.full((6, 8), 0xFF, np.uint8), np.full((6, 8), 0x0F, np.uint8), np.full((6, 8), 0xFF, np.uint8)
    cstick, estick = np.full((3, 24), 0xFF, np.uint8), np.full((2, 24), 0xFF, np.uint8)
    for p in range(nc):
        for o in range(3):
            c = np.roll(ccol[p], o)
            assert cpair[c[1]][c[0]] == 0xFF
            cpair[c[1]][c[0]], cthird[c[1]][c[0]] = 4 * p + o, c[2]
            cstick[:, 3 * p + o] = c
    for p in range(ne):
        for o in range(2):
            c = np.roll(ecol[p], o)
            assert epair[c[1]][c[0]] == 0xFF
            epair[c[1]][c[0]] = 2 * p + o
            estick[:, 2 * p + o] = c
            assert t.edge_code[c[0] + 10 * c[1]] == 2 * p + o                # the edge byte IS RC_FMT_CODE's
    assert (cpair != 0xFF).sum() == 3 * nc and (epair != 0xFF).sum() == 2 * ne
    return CubieTables(cube_size=n, nc=nc, ne=ne, corner_cw=cw, edge_facelets=t.edge_defs.copy(), corner_colours=ccol, edge_colours=ecol,
                       fixed=np.flatnonzero(~moved).astype(np.uint8), solved=t.solved, corner_pair=cpair, corner_third=cthird, edge_pair=epair,
                       corner_sticker=cstick, edge_sticker=estick)


def get_corner_moves(cube_size: int):
    """(src, twist) uint8 [A][NC]: how a move acts on the corner state (piece[q], ori[q]) of the cubie rule above (include/rubiksearch.h
    "Corner pattern database"): piece'[q] = piece[src[a][q]], ori'[q] = (ori[src[a][q]] + twist[a][q]) mod 3, where 3 * src[a][q] +
    twist[a][q] is the corner byte of slot q after move a on the solved cube (moves gather: state[perm[a]])."""
    t, cb = get_tables(cube_size), get_cubies(cube_size)
    cub = cb.cubies(t.solved[t.perm.astype(np.int64)])[0][:, :cb.nc]
    return (cub // 3).astype(np.uint8), (cub % 3).astype(np.uint8)


def get_edge_moves():
    """(src, flip) uint8 [A][NE] of the 3x3x3: how a move acts on the edge state (piece[q], ori[q]) of the cubie rule above
    (include/rubikhip.h "Edge pattern databases"): piece'[q] = piece[src[a][q]], ori'[q] = ori[src[a][q]] ^ flip[a][q], where
    2 * src[a][q] + flip[a][q] is the edge byte of slot q after move a on the solved cube (moves gather: state[perm[a]]).  The
    2x2x2 has no edges."""
    t, cb = get_tables(3), get_cubies(3)
    cub = cb.cubies(t.solved[t.perm.astype(np.int64)])[0][:, cb.nc:]
    return (cub // 2).astype(np.uint8), (cub % 2).astype(np.uint8)


# ---- the subgroup chain (include/rubikhip.h "Subgroup chain", prefix rct_): <all> > <U,D,R,L,F2,B2> > <U,D,F2,R2,B2,L2> > <half turns> > {solved}
CHAIN_SIZES = (2048, 2187 * 495, 40320 * 70, 96 * 24 ** 3)
CHAIN_NO_ACTION = 0xFF
_CHAIN_QUARTER = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11), (0, 1, 4, 5, 6, 7, 10, 11), (0, 1, 6, 7), ())   # quarter turns of each stage; the other faces turn by halves


@dataclass(frozen=True)
class ChainData:
    sizes: tuple  # N of the four coset tables
    generators: tuple  # per stage uint8 [count][2]: the one or two quarter-turn actions of each generator, in the rule's order (0xFF: none)
    gen_codes: np.ndarray  # uint8 [4][12]  action + 16 * (half turn), 0xFF beyond the stage's count (rc_tables.h chain_gen)
    corner_cosets: np.ndarray  # uint16 [96]  H: lehmer(cp) of the corner permutations half turns reach, ascending


def _lehmer(p):
    n = len(p)
    return sum(sum(p[r] < p[q] for r in range(q + 1, n)) * math.factorial(n - 1 - q) for q in range(n))


@functools.lru_cache(maxsize=None)
def get_chain() -> ChainData:
    """The generated data of the subgroup chain (3x3x3 only): the generator lists and H, the corner permutations reachable from
    solved by half turns, found by closure under get_corner_moves' half turns."""
    gens, codes = [], np.full((4, 12), CHAIN_NO_ACTION, np.uint8)
    for stage, quarter in enumerate(_CHAIN_QUARTER):
        rows = []
        for a in range(12):
            if a in quarter:
                rows.append((a, CHAIN_NO_ACTION))
            elif a % 2 == 0:                                                   # a half turn: the clockwise action twice
                rows.append((a, a))
        gens.append(np.array(rows, np.uint8))
        codes[stage, :len(rows)] = [a + 16 * (b != CHAIN_NO_ACTION) for a, b in rows]
    src = get_corner_moves(3)[0].astype(np.int64)
    half = [src[a][src[a]] for a in range(0, 12, 2)]
    seen, todo = {tuple(range(8))}, [tuple(range(8))]
    while todo:
        p = np.array(todo.pop())
        for h in half:
            q = tuple(int(x) for x in p[h])
            if q not in seen:
                seen.add(q)
                todo.append(q)
    h = np.array(sorted(_lehmer(p) for p in seen), np.uint16)
    assert len(h) == 96
    return ChainData(sizes=CHAIN_SIZES, generators=tuple(gens), gen_codes=codes, corner_cosets=h)
