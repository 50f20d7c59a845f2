"""Restatement of the edge pattern databases (include/rubikhip.h "Edge pattern databases"): the reference the rce_* kernels and
pattern.EdgeTable / MaxTable are compared with.  Test infrastructure only.

The distances come from a breadth-first search on STICKER arrays moved by the oracle (oracle/rc_oracle.c), deduplicated by an index
computed from the stickers: the edge bytes by tests/cubie_ref.py's rule (the slot's two colours -> piece * 2 + ori), then the index
formula of the header.  Nothing here reads tables.get_edge_moves, the generated header or the library.  rank and unrank are restated
as plain loops; edge_moves() derives the move tables a second way, from where each move carries each edge sticker.

LEVELS below holds the level counts of the two 6-piece tables: they take minutes on a CPU and are no part of any test.  Command, from the
repository root (about four minutes per mask, the oracle on 4 threads):

    python -m tests.edge_ref 0x03f 0xfc0
"""
from __future__ import annotations

import functools
import sys

import numpy as np

from tests import cubie_ref

NE, NC, A = 12, 8, 12
ILLEGAL = 0xFF
MAX_K = 7
SMALL_MASKS = (0x001, 0x800, 0x801, 0x188, 0x452, 0x00F)        # {0}, {11}, {0, 11}, {3, 7, 8}, {1, 4, 6, 10}, {0, 1, 2, 3}
LOW6, HIGH6 = 0x03F, 0xFC0                                      # {0..5}, {6..11}
# patterns per distance, level 0 first: `python -m tests.edge_ref 0x03f 0xfc0` (the sticker search below, on a CPU)
LEVELS = {
    0x03f: (1, 12, 109, 941, 7767, 60751, 439746, 2768420, 12518862, 22465564, 4312983, 2764),
    0xfc0: (1, 10, 93, 832, 6904, 54904, 406895, 2646406, 12435645, 22838844, 4185743, 1643),
}
assert all(sum(v) == 42577920 for v in LEVELS.values())


def pieces(mask):
    return [t for t in range(NE) if mask >> t & 1]


def size(k):
    """N(k) = 12!/(12-k)! * 2^k"""
    n = 1
    for i in range(k):
        n *= 2 * (NE - i)
    return n


assert [size(k) for k in range(1, 8)] == [24, 528, 10560, 190080, 3041280, 42577920, 510935040]


def rank(pos, ori):
    """The index of slots pos[i] and ori bits ori[i] of the k tracked pieces, ascending by piece."""
    k, perm, bits = len(pos), 0, 0
    for i in range(k):
        d = pos[i] - sum(1 for j in range(i) if pos[j] < pos[i])
        perm = perm * (NE - i) + d
        bits += ori[i] << i
    return perm * 2 ** k + bits


def unrank(k, index):
    """(pos, ori) of an index below N(k)."""
    ori = [index >> i & 1 for i in range(k)]
    perm, dig = index >> k, [0] * k
    for i in range(k - 1, -1, -1):
        perm, dig[i] = divmod(perm, NE - i)
    free, pos = list(range(NE)), []
    for i in range(k):
        pos.append(free.pop(dig[i]))
    return pos, ori


def home_index(mask):
    t = pieces(mask)
    return rank(t, [0] * len(t))


def move(esrc, eflip, a, pos, ori):
    """THE RULE's move: a piece in slot s goes to the q with esrc[a][q] == s, its ori XORed with eflip[a][q]."""
    q = [list(esrc[a]).index(s) for s in pos]
    return q, [o ^ int(eflip[a][x]) for o, x in zip(ori, q)]


def index_of_bytes(mask, edge_bytes):
    """uint32 [n]: the index of every row of edge bytes [n, 12] (any byte values); 0xFFFFFFFF for an ILLEGAL row: a byte >= 24, a
    tracked piece absent or twice.  Untracked slots are not looked at beyond the range check."""
    e = np.asarray(edge_bytes, np.uint8)
    n, t = len(e), pieces(mask)
    k = len(t)
    bad = (e >= 24).any(1)
    piece, flip = (e >> 1).astype(np.int64), (e & 1).astype(np.int64)
    pos, ori = np.zeros((n, k), np.int64), np.zeros((n, k), np.int64)
    for i, p in enumerate(t):
        hit = piece == p
        bad |= hit.sum(1) != 1
        pos[:, i] = hit.argmax(1)
        ori[:, i] = flip[np.arange(n), pos[:, i]]
    perm, bits = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(k):
        perm = perm * (NE - i) + pos[:, i] - (pos[:, :i] < pos[:, i:i + 1]).sum(1)
        bits += ori[:, i] << i
    return np.where(bad, 0xFFFFFFFF, perm * 2 ** k + bits).astype(np.uint32)


def edge_bytes_of(states):
    """[n, 12] edge bytes of sticker rows by cubie_ref's rule (0xFF where the two colours are no edge cubie)."""
    R = cubie_ref.rule(3)
    st = np.asarray(states, np.uint8)
    e = st[:, R.edge]
    ok = (e < 6).all(2)
    return np.where(ok, R.ekey[np.where(ok, e[..., 0] * np.uint8(6) + e[..., 1], 0)], np.uint8(0xFF))


def index_of_states(mask, states):
    return index_of_bytes(mask, edge_bytes_of(states))


def unrank_cubies(mask, idx):
    """rce_unrank: cubie rows uint8 [n, 20] and the bool [n] of the indices >= N(k) (those come out solved).  Corners home; tracked
    pieces as the index says; untracked pieces into the free slots, both ascending, ori 0; an odd flip sum flips the edge in the highest
    free slot; then an odd edge permutation makes the edges of the two highest free slots trade places."""
    t = pieces(mask)
    k, N = len(t), size(len(t))
    idx = np.asarray(idx, np.int64)
    cub, bad = np.zeros((len(idx), NC + NE), np.uint8), (idx < 0) | (idx >= N)
    for r, ix in enumerate(idx):
        pos, ori = unrank(k, int(ix)) if not bad[r] else (t, [0] * k)
        piece_at, ori_at = [None] * NE, [0] * NE
        for i in range(k):
            piece_at[pos[i]], ori_at[pos[i]] = t[i], ori[i]
        free = [s for s in range(NE) if piece_at[s] is None]
        for s, p in zip(free, [p for p in range(NE) if p not in t]):
            piece_at[s] = p
        if sum(ori) & 1:
            ori_at[free[-1]] ^= 1
        if sum(1 for x in range(NE) for y in range(x + 1, NE) if piece_at[x] > piece_at[y]) & 1:
            x, y = free[-2], free[-1]
            piece_at[x], piece_at[y] = piece_at[y], piece_at[x]
        cub[r, :NC] = 3 * np.arange(NC)
        cub[r, NC:] = [2 * p + o for p, o in zip(piece_at, ori_at)]
    return cub, bad


def edge_moves(perm):
    """(esrc, eflip) uint8 [A, 12] from sticker positions: the sticker that arrives at position j of slot q under move a (a gather:
    new[i] = old[perm[a][i]]) sat at position (j + f) % 2 of slot src; eflip = f.  perm: the moves as gathers, [A, 54]."""
    R = cubie_ref.rule(3)
    where = {int(R.edge[q][j]): (q, j) for q in range(NE) for j in range(2)}
    esrc, eflip = np.zeros((A, NE), np.uint8), np.zeros((A, NE), np.uint8)
    for a in range(A):
        for q in range(NE):
            frm = [where[int(perm[a][R.edge[q][j]])] for j in range(2)]
            assert frm[0][0] == frm[1][0] and frm[1][1] == 1 - frm[0][1]
            esrc[a, q], eflip[a, q] = frm[0][0], frm[0][1]
    return esrc, eflip


@functools.lru_cache(maxsize=None)
def oracle():
    from oracle.oracle_np import Oracle
    return Oracle()


def bfs(mask, chunk=1 << 18, threads=1, say=None):
    """(table uint8 [N(k)], levels): breadth-first over sticker states moved by the oracle, one representative per pattern."""
    orc = oracle()
    N = size(len(pieces(mask)))
    table = np.full(N, ILLEGAL, np.uint8)
    frontier = orc.solved(3, 1)
    table[index_of_states(mask, frontier)] = 0
    levels, depth = [1], 0
    while len(frontier):
        fresh = []
        for at in range(0, len(frontier), chunk):
            part = frontier[at:at + chunk]
            for a in range(A):
                ch = orc.step(3, part, np.full(len(part), a, np.uint8), threads)[0]
                idx = index_of_states(mask, ch).astype(np.int64)
                new = np.flatnonzero(table[idx] == ILLEGAL)
                uniq, first = np.unique(idx[new], return_index=True)
                table[uniq] = depth + 1
                fresh.append(ch[new[first]])
        frontier = np.concatenate(fresh) if fresh else frontier[:0]
        depth += 1
        if len(frontier):
            levels.append(len(frontier))
        if say:
            say(f"mask {mask:#05x} depth {depth}: {len(frontier)}")
    assert sum(levels) == N and not (table == ILLEGAL).any()
    return table, tuple(levels)


@functools.lru_cache(maxsize=None)
def small(mask):
    """bfs() of one of SMALL_MASKS, once per process."""
    return bfs(mask)


if __name__ == "__main__":
    for arg in sys.argv[1:]:
        m = int(arg, 0)
        print(f"    {m:#05x}: {bfs(m, threads=4, say=lambda s: print(s, file=sys.stderr, flush=True))[1]},", flush=True)
