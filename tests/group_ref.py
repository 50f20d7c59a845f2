"""Facts about the cube groups that neither the oracle nor the reference supplies, and a breadth-first driver that checks a move
implementation against them.  TEST INFRASTRUCTURE ONLY, plain numpy.

Every other test of this suite compares a kernel with a restatement of the same operation.  Here the yardstick is mathematics:
  * the number of states at each quarter-turn distance from solved (OEIS A079762 for the 2x2x2 with one corner fixed, OEIS A080601
    for the 3x3x3), 3 674 160 states of the 2x2x2 in all;
  * the order of a move word w (the smallest k with w^k = identity): the group acts freely on reachable colourings, so EVERY start
    state returns first at exactly k;
  * splitmix64's published test vector and a big-int restatement of DESIGN.md section 5.
From the complete 2x2x2 search a perfect value function (`dist`) and a perfect policy (`nbr`) follow; with them beam search and the
greedy rollout have a known exact answer for every state of the group.

Deduplication here packs the STICKER rows itself (3 bits per sticker, 21 per int64 word); it never looks at the kernels' keys or codes.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

# ------------------------------------------------------------------------------------------------------------------ constants
SPHERES_222 = (1, 6, 27, 120, 534, 2256, 8969, 33058, 114149, 360508, 930588, 1350852, 782536, 90280, 276)   # OEIS A079762, d = 0..14
SPHERES_333 = (1, 12, 114, 1068, 10011, 93840, 878880, 8221632)                                                # OEIS A080601, d = 0..7
GROUP_222 = 3674160                                                     # 7! * 3^6: seven free corners, the last twist is forced
assert sum(SPHERES_222) == GROUP_222

# Distinct 20-byte compact codes per distance on the 3x3x3.  The code is NOT injective there: the reference's corner look-up
# (py333.py:171-180) fills 24 of the 44 reachable corner hashes and leaves zeros = (piece 0, orientation 0) in the other 20, kept bug-compatible;
# two states that differ only in corners whose hash is unfilled get one code.  First collisions at d = 5.  Recorded behaviour.
CODES_333 = (1, 12, 114, 1068, 10011, 93838, 878854, 8221382)

ACTION_NAMES = {2: ("U", "U'", "F", "F'", "R", "R'"), 3: ("U", "U'", "F", "F'", "R", "R'", "D", "D'", "B", "B'", "L", "L'")}
N_STICKERS = {2: 24, 3: 54}
N_ACTIONS = {2: 6, 3: 12}
N_SLOTS = {2: 7, 3: 20}

# word -> (order on the 3x3x3, order on the 2x2x2 or None where the word needs a face the 2x2x2 env does not turn)
WORD_ORDERS = {
    "U": (4, 4),
    "R U": (105, 15),
    "R U'": (63, 9),
    "R F'": (63, 9),
    "R U R' U'": (6, 6),
    "R U R' U": (5, 5),
    "R U F": (80, 10),
    "R U L D": (315, None),
    "R L' U D' F B'": (8, None),
}
COMMUTING_333 = (("U", "D"), ("R", "L"), ("F", "B"))                   # opposite faces share no cubie

SPLITMIX64_SEED = 1234567
SPLITMIX64_VECTOR = (6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821)
RNG_TRIPLES = ((0, 0, 0), (11, 2, 5), (2 ** 63 + 5, 2 ** 40, 10 ** 9))  # (seed, stream, walk)


def word_actions(word, cube_size):
    """'R U' -> [4, 0]: the env's action indices of a move word."""
    names = ACTION_NAMES[cube_size]
    return [names.index(m) for m in word.split()]


def words_for(cube_size):
    """[(word, actions, order)] for the cube size."""
    out = []
    for w, (o3, o2) in WORD_ORDERS.items():
        order = o3 if cube_size == 3 else o2
        if order is not None:
            out.append((w, word_actions(w, cube_size), order))
    return out


# ------------------------------------------------------------------------------------------------------------------ RNG, restated
_M64 = (1 << 64) - 1


def splitmix64(state):
    """One splitmix64 step on Python ints: (new state, output)."""
    state = (state + 0x9E3779B97F4A7C15) & _M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return state, z ^ (z >> 31)


def rng_actions(seed, stream, walk, n, A):
    """DESIGN.md section 5 on Python big ints: the splitmix64 chain seed -> (^ stream) -> (^ walk) -> two state words, then
    xoroshiro128+ (24, 16, 37), action = (hi32(s0 + s1) * A) >> 32."""
    rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & _M64
    _, a = splitmix64(seed & _M64)
    _, b = splitmix64(a ^ (stream & _M64))
    st, s0 = splitmix64(b ^ (walk & _M64))
    _, s1 = splitmix64(st)
    if (s0 | s1) == 0:
        s1 = 0x9E3779B97F4A7C15
    out = []
    for _ in range(n):
        r = (s0 + s1) & _M64
        s1 ^= s0
        s0, s1 = rotl(s0, 24) ^ s1 ^ ((s1 << 16) & _M64), rotl(s1, 37)
        out.append(((r >> 32) * A) >> 32)
    return np.array(out, np.uint8)


# ------------------------------------------------------------------------------------------------------------------ packing
def pack(states):
    """[n, S] uint8 stickers (0..5) -> [n, ceil(S / 21)] int64: 3 bits per sticker, 21 stickers per word (bit 63 stays clear, so the
    signed order is the unsigned one).  Injective on sticker rows; the ONLY identity of a state this module uses."""
    st = np.ascontiguousarray(states, np.uint8)
    assert st.ndim == 2 and (st < 8).all()
    n, S = st.shape
    words = np.zeros((n, -(-S // 21)), np.int64)
    for s in range(S):
        words[:, s // 21] |= st[:, s].astype(np.int64) << (3 * (s % 21))
    return words


def _sorted_groups(words):
    """Lexicographic order of the rows (stable: equal rows keep their input order) and the mask of rows that start a new group."""
    order = np.lexsort(words.T[::-1])
    w = words[order]
    first = np.ones(len(w), bool)
    first[1:] = (w[1:] != w[:-1]).any(axis=1)
    return order, first


def count_distinct(rows):
    """Number of distinct rows of an integer matrix (any width up to what int64 words hold: each column becomes one sort key)."""
    rows = np.ascontiguousarray(rows).astype(np.int64).reshape(len(rows), -1)
    return int(_sorted_groups(rows)[1].sum()) if len(rows) else 0


def pack_code(code, base):
    """[n, SL] codes (< base) -> [n, words] int64 radix words of 8 slots each (24^8, 21^8 < 2^63): injective on code rows."""
    c = np.ascontiguousarray(code).astype(np.int64)
    assert c.ndim == 2 and int(c.max(initial=0)) < base
    n, SL = c.shape
    out = np.zeros((n, -(-SL // 8)), np.int64)
    for s in range(SL):
        out[:, s // 8] = out[:, s // 8] * base + c[:, s]
    return out


# ------------------------------------------------------------------------------------------------------------------ BFS
@dataclass
class Level:
    depth: int
    states: np.ndarray                 # [n, S] uint8, sorted by pack() words
    code: np.ndarray                   # [n, SL] uint8: what the expansion (or `encode`, for the root) gave for the state
    solved: np.ndarray                 # [n] uint8: the expansion's solved flag of the state
    parent: np.ndarray                 # [n] int64: row of the previous level the state was first reached from (-1: root)
    move: np.ndarray                   # [n] int8: the move taken from that parent (-1: root)
    child_code: np.ndarray = None      # [n, A, SL]: the expansion of this level, kept when keep_expansion
    child_solved: np.ndarray = None    # [n, A]
    children_equal_solved: np.ndarray = None   # [n, A] bool: child's stickers == the solved row, by this module's comparison


def bfs(expand, encode, solved_row, max_depth=None, keep_expansion=True):
    """Breadth-first search from `solved_row` over expand(parents [n, S]) -> (children [n, A, S], child_code [n, A, SL], child_solved
    [n, A]); encode(states [n, S]) -> (code, solved) is used for the root only.  Level d + 1 = unique(children of level d) minus level
    d - 1.  A quarter turn flips the parity of the corner permutation, so a child is never at its parent's distance: asserted here on
    every level (no child row equals a row of the parent's level), not assumed.
    Stops after `max_depth` (levels 0..max_depth returned, the last one not expanded) or, with max_depth None, when a level has no new
    state (the last level returned IS expanded: its children are all known)."""
    root = np.ascontiguousarray(solved_row, np.uint8).reshape(1, -1)
    code0, solved0 = encode(root)
    cur = Level(0, root, np.asarray(code0).reshape(1, -1), np.asarray(solved0).reshape(1), np.array([-1], np.int64), np.array([-1], np.int8))
    cur_w, prev_w = pack(root), np.zeros((0, pack(root).shape[1]), np.int64)
    root_w = cur_w.copy()
    levels = []
    while True:
        if max_depth is not None and cur.depth == max_depth:
            levels.append(cur)
            return levels
        ch, cc, cs = expand(cur.states)
        n, A, S = ch.shape
        assert n == len(cur.states) and cc.shape[:2] == (n, A) and cs.shape == (n, A)
        flat = ch.reshape(n * A, S)
        cw = pack(flat)
        if keep_expansion:
            cur.child_code, cur.child_solved = cc, cs
        cur.children_equal_solved = (cw == root_w).all(axis=1).reshape(n, A)
        levels.append(cur)
        # tags: 0 = child, 1 = a state of the parent's level, 2 = a state of the level before; children come first, so the first row of
        # a group is the child with the lowest (parent, move) index
        words = np.concatenate([cw, cur_w, prev_w])
        tag = np.concatenate([np.zeros(len(cw), np.int8), np.ones(len(cur_w), np.int8), np.full(len(prev_w), 2, np.int8)])
        order, first = _sorted_groups(words)
        gid = np.cumsum(first) - 1
        t_sorted = tag[order]
        n_groups = int(gid[-1]) + 1
        has = [np.bincount(gid[t_sorted == t], minlength=n_groups) > 0 for t in (0, 1, 2)]
        assert not (has[0] & has[1]).any(), f"depth {cur.depth}: a child equals a state at its parent's distance"
        fresh = has[0] & ~has[2]
        starts = np.flatnonzero(first)
        pick = order[starts[fresh]]                                   # first (lowest-index) child of every new state, in sorted order
        assert (pick < len(cw)).all()
        if len(pick) == 0:
            assert max_depth is None
            return levels
        nxt = Level(cur.depth + 1, flat[pick], cc.reshape(n * A, -1)[pick], cs.reshape(n * A)[pick], pick // A, (pick % A).astype(np.int8))
        prev_w, cur_w = cur_w, cw[pick]
        cur = nxt


ORACLE_THREADS = 16


def oracle_bfs(oracle, cube_size, max_depth):
    """bfs() driven by the CPU oracle (oracle.oracle_np.Oracle), on at most ORACLE_THREADS threads."""
    thr = min(ORACLE_THREADS, oracle.max_threads())
    return bfs(lambda p: oracle.expand(cube_size, p, threads=thr), lambda s: (oracle.encode(cube_size, s)[0], oracle.is_solved(cube_size, s)),
               oracle.solved(cube_size)[0], max_depth=max_depth)


# ------------------------------------------------------------------------------------------------------------------ 2x2x2 group
RADIX_222 = 21 ** np.arange(7, dtype=np.int64)                         # key = sum_s code_s * 21^s < 21^7 = 1 801 088 541


@dataclass
class Group222:
    keys: np.ndarray        # [N] int64, ascending: radix key of the state's 7-byte code; id = position here
    dist: np.ndarray        # [N] int8: quarter turns to solved
    nbr: np.ndarray         # [N, 6] int32: id of the state after action a
    states: np.ndarray      # [N, 24] uint8 sticker rows (loadable with VecCubeEnv.set_sim_cube)

    def ids(self, code):
        """[n, 7] codes -> ids; asserts every code is one of the group's."""
        k = np.ascontiguousarray(code).astype(np.int64) @ RADIX_222
        i = np.searchsorted(self.keys, k)
        assert (i < len(self.keys)).all() and (self.keys[np.minimum(i, len(self.keys) - 1)] == k).all(), "a code outside the group"
        return i

    def ball(self, radius):
        return np.flatnonzero(self.dist <= radius)


def build_222(levels):
    """The complete 2x2x2 search (bfs(..., keep_expansion=True)) -> Group222.  Needs the code to be injective on the group (asserted)."""
    states = np.concatenate([lv.states for lv in levels])
    code = np.concatenate([lv.code for lv in levels])
    dist = np.concatenate([np.full(len(lv.states), lv.depth, np.int8) for lv in levels])
    child_code = np.concatenate([lv.child_code for lv in levels])
    keys = code.astype(np.int64) @ RADIX_222
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    assert len(keys) == GROUP_222 and (np.diff(keys) > 0).all(), "the 7-byte code is not injective on the group"
    g = Group222(keys, dist[order], None, states[order])
    nbr = g.ids(child_code[order].reshape(-1, 7)).reshape(-1, 6).astype(np.int32)
    g.nbr = nbr
    return g
