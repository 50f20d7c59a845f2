"""Plain-Python restatement of the ida_* section (include/rubikhip.h "Iterative-deepening A*"): the reference ida_init / ida_search and
search.ida_search are compared with.  Test infrastructure only.

The cube is moved by what the ORACLE does to the solved cube's cubie bytes (cubie_ref reads them off the stickers): nothing here reads
the package's move tables, the library's ida_canonical or any other ida_* data.  h comes from host copies of the device's own tables
(proved distances elsewhere: tests/test_gpu_pattern.py, tests/test_gpu_edge.py) through edge_ref's index and a corner index that
tests/test_ida_host.py compares with pattern_ref's.

A cube is a tuple of 48 values, three per corner slot and two per edge slot: entry (q, j) of a corner slot that holds piece p with
ori o is 3 p + (o + j) % 3, of an edge slot 2 p + (o ^ j) -- so entry (q, 0) is the slot's cubie byte and a move is a pure
permutation of the 48 entries (one itemgetter call)."""
from __future__ import annotations

import copy
import functools
import operator

import numpy as np

from tests import cubie_ref, edge_ref

A, NOOP, INF = 12, 12, 2 ** 31 - 1
SOLVED, EXHAUSTED, ILLEGAL, BAD_FRAME = 1, 2, 4, 8
MAX_DEPTH = 32
COUNTS = (12, 114, 1068, 10011, 93840, 879624, 8245296)            # canonical sequences of length 1..7 (to 5: OEIS A080601)
CREF = tuple(3 * q for q in range(8))                             # entry (q, 0) of corner slot q
EREF = tuple(24 + 2 * q for q in range(12))
HOME = tuple([3 * q + j for q in range(8) for j in range(3)] + [2 * q + j for q in range(12) for j in range(2)])


class OutOfReach(Exception):
    """the restatement's node cap was reached"""


def skipped(p2, p1, m):
    """THE RULE: may move m NOT follow a path that ends ..., p2, p1 (12: no move)?"""
    if p1 == NOOP:
        return False
    return m == p1 ^ 1 or (m == p1 and m & 1 == 1) or m == p1 == p2 or (m >> 1) + 3 == (p1 >> 1)


def allowed_mask():
    return np.array([[[not skipped(p2, p1, m) for m in range(A)] for p1 in range(13)] for p2 in range(13)])


ALLOWED = [[[m for m in range(A) if not skipped(p2, p1, m)] for p1 in range(13)] for p2 in range(13)]
# FIRST[p2][p1][cursor]: the least allowed move >= cursor, 12 where there is none
FIRST = [[[min([m for m in ALLOWED[p2][p1] if m >= c], default=NOOP) for c in range(13)] for p1 in range(13)] for p2 in range(13)]


def sequences(k, p2=NOOP, p1=NOOP):
    """The canonical sequences of length k after ..., p2, p1, in the search's order."""
    if k == 0:
        yield ()
        return
    for m in ALLOWED[p2][p1]:
        for rest in sequences(k - 1, p1, m):
            yield (m,) + rest


def count(k):
    """How many canonical sequences of length k there are, by dynamic programming over the last two moves."""
    ways = {(NOOP, NOOP): 1}
    for _ in range(k):
        nxt = {}
        for (p2, p1), w in ways.items():
            for m in ALLOWED[p2][p1]:
                nxt[(p1, m)] = nxt.get((p1, m), 0) + w
        ways = nxt
    return sum(ways.values())


@functools.lru_cache(maxsize=None)
def oracle_moves():
    """(csrc [12][8], ctwist, esrc [12][12], eflip) read off the oracle: after move a on the solved cube slot q holds the cubie byte
    3 * csrc + ctwist | 2 * esrc + eflip, because on the solved cube piece p sits in slot p with ori 0."""
    o = edge_ref.oracle()
    csrc, ctw, esrc, efl = [], [], [], []
    for a in range(A):
        cub = cubie_ref.cubies(3, o.step(3, o.solved(3, 1), np.array([a], np.uint8))[0])[0][0].astype(int)
        csrc.append(tuple(cub[:8] // 3)); ctw.append(tuple(cub[:8] % 3))
        esrc.append(tuple(cub[8:] // 2)); efl.append(tuple(cub[8:] % 2))
    return tuple(csrc), tuple(ctw), tuple(esrc), tuple(efl)


@functools.lru_cache(maxsize=None)
def movers():
    """12 itemgetters on the 48 entries: new (q, j) = old (src, (j + twist) % 3) | old (src, j ^ flip)."""
    csrc, ctw, esrc, efl = oracle_moves()
    out = []
    for a in range(A):
        perm = [3 * csrc[a][q] + (j + ctw[a][q]) % 3 for q in range(8) for j in range(3)]
        perm += [24 + 2 * esrc[a][q] + (j ^ efl[a][q]) for q in range(12) for j in range(2)]
        out.append(operator.itemgetter(*perm))
    return tuple(out)


def from_bytes(cub):
    """20 cubie bytes -> the 48 entries; None for a byte >= 24 or a piece twice (IDA_ILLEGAL's rule)."""
    cub = [int(b) for b in cub]
    if max(cub) >= 24 or len({b // 3 for b in cub[:8]}) < 8 or len({b // 2 for b in cub[8:]}) < 12:
        return None
    return tuple([3 * (b // 3) + (b % 3 + j) % 3 for b in cub[:8] for j in range(3)] + [b ^ j for b in cub[8:] for j in range(2)])


def to_bytes(x):
    return [x[i] for i in CREF] + [x[i] for i in EREF]


def corner_index(x):
    """corner_index of the rcc_* section: lehmer(cp) * 3^7 + sum_{q<7} co[q] 3^q."""
    b = [x[i] for i in CREF]
    cp = [v // 3 for v in b]
    lehmer = 0
    for q in range(8):
        lehmer = lehmer * (8 - q) + sum(1 for r in range(q + 1, 8) if cp[r] < cp[q])
    return lehmer * 2187 + sum((b[q] % 3) * 3 ** q for q in range(7))


def edge_index(x, pieces):
    b = [x[i] for i in EREF]
    where = {v >> 1: q for q, v in enumerate(b)}
    pos = [where[t] for t in pieces]
    return edge_ref.rank(pos, [b[p] & 1 for p in pos])


class Heuristic:
    """h = the maximum over host copies of the tables: corner a uint8 array [88 179 840] or None, edges a list of (mask, array)."""

    def __init__(self, corner=None, edges=()):
        self.corner = corner
        self.edges = [(edge_ref.pieces(mask), t) for mask, t in edges]

    def __call__(self, x):
        h = 0
        if self.corner is not None:
            i = corner_index(x)
            h = max(h, int(self.corner[i]) if i < len(self.corner) else 0xFF)
        for pieces, t in self.edges:
            i = edge_index(x, pieces)
            h = max(h, int(t[i]) if i < len(t) else 0xFF)
        return h


class Frame:
    """One cube's frame and the rule's state machine on it, pass by pass."""

    def __init__(self, cub, h, limit, max_depth, prefix=(), floor_given=None):
        self.h, self.max_depth = h, max_depth
        self.floor = len(prefix) if floor_given is None else floor_given
        self.nib = [0] * MAX_DEPTH                                     # the 32 nibbles of the trail; entries from `depth` on are stale
        self.cursor, self.depth, self.bound, self.next, self.nodes, self.status = 0, 0, 0, INF, 0, 0
        self.passes, self.mv = 0, movers()
        self.written, self.deepest, self.word1 = set(), 0, False
        x = from_bytes(cub)
        if x is None:
            self.status |= ILLEGAL
        if not 0 <= self.floor <= max_depth:
            self.status |= BAD_FRAME
        elif not self.status and any(m >= A for m in prefix[:self.floor]):
            self.status |= BAD_FRAME
        if self.status:
            return
        mv = movers()
        for m in prefix[:self.floor]:
            x = mv[m](x)
        self.x, self.depth = x, self.floor
        self.nib[:self.floor] = prefix[:self.floor]
        self.deepest, self.word1 = self.depth, any(self.nib[16:])
        self.lim = min(limit, max_depth)
        h0 = h(x)
        if h0 == 0xFF:
            self.status, self.depth, self.nib = ILLEGAL, 0, [0] * MAX_DEPTH
            return
        self.bound = self.floor + h0
        if x == HOME:
            self.status = SOLVED
        elif self.bound > self.lim:
            self.status, self.next = EXHAUSTED, self.bound

    @classmethod
    def resume(cls, cub, h, limit, max_depth, floor=0, trail=(), depth=0, bound=0, next=INF, cursor=0, nodes=0):
        """A frame the CALLER wrote, as ida_search takes it (the header's "written frame" rule): trail = the nibbles from the root on,
        prefix included (what lies from `depth` on is stale and kept).  A refused frame gets IDA_BAD_FRAME OR-ed into its status and
        keeps every other field as written; depth > bound is NOT refused.  The node is the root moved along trail[0..depth)."""
        f = cls.__new__(cls)
        f.h, f.max_depth, f.floor, f.lim = h, max_depth, floor, min(limit, max_depth)
        f.nib = (list(trail) + [0] * MAX_DEPTH)[:MAX_DEPTH]
        f.cursor, f.depth, f.bound, f.next, f.nodes, f.status = cursor, depth, bound, next, nodes, 0
        f.passes, f.mv = 0, movers()
        f.written, f.deepest, f.word1 = set(), depth, any(f.nib[16:])
        x = from_bytes(cub)
        if x is None:
            f.status |= ILLEGAL
        if not 0 <= floor <= max_depth or depth < floor or depth > max_depth or cursor > A or bound > f.lim:
            f.status |= BAD_FRAME
        elif not f.status and any(m >= A for m in f.nib[:depth]):
            f.status |= BAD_FRAME
        if not f.status:
            for m in f.nib[:depth]:
                x = f.mv[m](x)
            f.x = x
        return f

    def written_frame(self):
        """the keyword arguments of resume() that rewrite this frame"""
        return dict(floor=self.floor, trail=list(self.nib), depth=self.depth, bound=self.bound, next=self.next, cursor=self.cursor,
                    nodes=self.nodes)

    def clone(self):
        """A frame of its own on the same heuristic (a deep copy would copy the tables)."""
        f = copy.copy(self)
        f.nib, f.written = list(self.nib), set(self.written)
        return f

    def step(self):
        """One pass: a child generated, or one level back (at the start node: the iteration ends)."""
        g, t = self.depth, self.nib
        p1, p2 = (t[g - 1] if g >= 1 else NOOP), (t[g - 2] if g >= 2 else NOOP)
        m = FIRST[p2][p1][self.cursor]
        self.passes += 1
        if m != NOOP:
            y = self.mv[m](self.x)
            self.nodes += 1
            h = self.h(y)
            if h == 0xFF:
                self.status = ILLEGAL
            elif g + 1 + h > self.bound:
                self.next, self.cursor = min(self.next, g + 1 + h), m + 1
            else:
                self.x, self.depth, self.cursor = y, g + 1, 0
                t[g] = m
                self.written.add(g)                                          # coverage: which nibbles a run writes, how deep it gets,
                self.deepest = max(self.deepest, g + 1)                      # whether word 1 of the trail was ever nonzero
                self.word1 = self.word1 or (g >= 16 and m != 0)
                if y == HOME:
                    self.status = SOLVED
        elif g > self.floor:
            self.x, self.cursor, self.depth = self.mv[p1 ^ 1](self.x), p1 + 1, g - 1
        elif self.next > self.lim:
            self.status = EXHAUSTED
        else:
            self.bound, self.next, self.cursor = self.next, INF, 0

    def run(self, max_passes=None, max_nodes=200000):
        while not self.status and (max_passes is None or self.passes < max_passes):
            if self.nodes >= max_nodes:
                raise OutOfReach
            self.step()
        return self

    @property
    def length(self):
        return self.depth if self.status == SOLVED else -1

    @property
    def trail(self):
        return self.nib[:self.depth]

    path = trail

    @property
    def words(self):
        """the two uint64 of the frame's trail"""
        return [sum(v << (4 * i) for i, v in enumerate(self.nib[16 * w:16 * w + 16])) for w in range(2)]

    @property
    def lower_bound(self):
        return self.depth if self.status == SOLVED else self.next if self.status == EXHAUSTED else self.bound


def solve(cub, h, limit=20, max_depth=None, **kw):
    return Frame(cub, h, limit, max(1, limit) if max_depth is None else max_depth).run(**kw)


def canonical_walk(rng, length, p2=NOOP, p1=NOOP):
    """A random canonical move sequence of `length` after ..., p2, p1 (uniform over the allowed moves at every step)."""
    out = []
    for _ in range(length):
        m = int(rng.choice(ALLOWED[p2][p1]))
        out.append(m)
        p2, p1 = p1, m
    return out


def undo(x, moves):
    """The cube that `moves` bring to x."""
    for m in reversed(moves):
        x = movers()[m ^ 1](x)
    return x


def replay_bytes(cub, moves):
    """The cubie bytes after `moves` by the oracle-derived movers."""
    x = from_bytes(cub)
    for m in moves:
        x = movers()[m](x)
    return to_bytes(x)


def spheres(depth):
    """[{48-tuple: distance}] breadth-first from solved to `depth`, and the per-level lists in discovery order."""
    dist, levels = {HOME: 0}, [[HOME]]
    for d in range(depth):
        nxt = []
        for x in levels[-1]:
            for mv in movers():
                y = mv(x)
                if y not in dist:
                    dist[y] = d + 1
                    nxt.append(y)
        levels.append(nxt)
    return dist, levels
