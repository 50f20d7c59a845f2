"""Leaves for the lockstep tree search's tests, from the CPU oracle: scrambled roots, the states that no-op padded paths reach from
them, and what the device step reports about those states (leaf code, child codes, solved flags).  The codes are real cube codes,
so transpositions are real, and the child of a child is the parent: the trees have 2-cycles.  TEST INFRASTRUCTURE ONLY."""
import zlib

import numpy as np

GEOMETRY = {3: (12, 20), 2: (6, 7)}           # cube size -> (actions, key bytes)


def scramble_depths(n):
    """Root r is 6, 5, 4, 3, 2, 1, 6, ... moves from solved: a single root is a deep one, every sixth one is solved by its first expansion."""
    return [6 - r % 6 for r in range(n)]


class Cubes:
    def __init__(self, oracle, cube_size, n, seed, depths=None):
        self.orc, self.cs, self.n = oracle, cube_size, n
        self.A, self.SL = GEOMETRY[cube_size]
        self.depths = list(depths) if depths is not None else scramble_depths(n)
        rng = np.random.default_rng([seed, cube_size, n])
        self.scramble = np.full((n, max(self.depths)), self.A, np.uint8)
        for r, k in enumerate(self.depths):
            for d in range(k):                                   # no move undoes the one before it
                a = int(rng.integers(0, self.A))
                while d and a == self.scramble[r, d - 1] ^ 1:
                    a = int(rng.integers(0, self.A))
                self.scramble[r, d] = a
        self.roots, _ = self.move(oracle.solved(cube_size, n), self.scramble, track=False)

    def move(self, states, paths, track=True):
        """(the states `paths` [n, depth] lead to, per row: did the walk see one state twice -- looked at only with `track`)."""
        st = np.ascontiguousarray(states, np.uint8).copy()
        seen = [{s.tobytes()} for s in st] if track else []
        twice = np.zeros(len(st), bool)
        for d in range(paths.shape[1]):
            live = np.flatnonzero(paths[:, d] < self.A)
            if len(live):
                st[live] = self.orc.step(self.cs, st[live], paths[live, d])[0]
                for r in live if track else ():
                    key = st[r].tobytes()
                    twice[r] |= key in seen[r]
                    seen[r].add(key)
        return st, twice

    def leaves(self, paths, track=True):
        """-> (states, leaf code [n, SL], child code [n, A, SL], solved [n, A], repeated-state flags [n]) of the leaves of `paths`."""
        st, twice = self.move(self.roots, np.asarray(paths, np.uint8).reshape(self.n, -1), track)
        code, _ = self.orc.encode(self.cs, st)
        _, cc, cs = self.orc.expand(self.cs, st)
        return st, code, cc, cs, twice

    def replay_solves(self, r, actions):
        st = self.roots[r:r + 1]
        done = [0]
        for a in actions:
            st, _, done, _ = self.orc.step(self.cs, st, np.array([a], np.uint8))
        return bool(done[0])


def code_hash(code):
    return zlib.crc32(bytes(np.asarray(code, np.uint8)))


def plain_row(code, A):
    """Value and policy as a deterministic function of the leaf code: a normal value, a softmax of normal logits."""
    g = np.random.default_rng(code_hash(code))
    v = np.float32(g.normal())
    x = g.normal(size=A).astype(np.float32)
    e = np.exp(x - x.max())
    return v, (e / e.sum()).astype(np.float32)


def adversarial_row(code, A, simple_path, seen):
    """The same, bent towards the decisions the rule fixes: values on a grid of 1/4 (equal W), the two largest policy entries equal or
    1 ulp apart with the larger at the HIGHER index (float32 ties that float64 would break the other way), a one-hot row and a row with
    zeros now and then, and a few NaN / +inf / -inf values.  `seen` counts the kinds handed out.
    +inf is given only to a leaf whose path saw no state twice.  An edge with W = +inf beats every virtual loss, so a descent follows
    the first +inf edge of each node; such a path being simple, the edges it turns to +inf lead to the new leaf and close no loop
    (by induction over the updates), and every descent still ends -- in the rule itself, not only in one implementation of it."""
    h = code_hash(code)
    g = np.random.default_rng(h)
    v = np.float32(np.round(g.normal() * 4) / 4)
    x = g.normal(size=A).astype(np.float32)
    e = np.exp(x - x.max())
    p = (e / e.sum()).astype(np.float32)
    kind = h % 12
    if kind == 0:
        v = np.float32(np.nan)
        seen["nan"] += 1
    elif kind == 1 and simple_path:
        v = np.float32(np.inf)
        seen["+inf"] += 1
    elif kind == 2:
        v = np.float32(-np.inf)
        seen["-inf"] += 1
    lo, hi = sorted(np.argsort(p)[-2:].tolist())
    top = p.max()
    if (h >> 5) & 1:
        p[lo] = p[hi] = top
        seen["equal_top"] += 1
    else:
        p[lo], p[hi] = top, np.nextafter(top, np.float32(np.inf))
        seen["ulp_top"] += 1
    shape = (h >> 7) % 12
    if shape == 0:
        p[:] = 0
        p[(h >> 12) % A] = 1
        seen["one_hot"] += 1
    elif shape == 1:
        p[(h >> 12) % 2::2] = 0
        seen["zeros"] += 1
    return v, p


KINDS = ("nan", "+inf", "-inf", "equal_top", "ulp_top", "one_hot", "zeros")


class Rows:
    """Value [n] and policy [n, A] rows for leaf codes; one row per distinct code, kept so that every tree is fed the same bytes."""

    def __init__(self, A, adversarial):
        self.A, self.adversarial, self.memo = A, adversarial, {}
        self.seen = dict.fromkeys(KINDS, 0)

    def __call__(self, leaf_code, twice):
        n = len(leaf_code)
        value, policy = np.zeros(n, np.float32), np.zeros((n, self.A), np.float32)
        for r in range(n):
            key = (leaf_code[r].tobytes(), bool(twice[r]))
            if key not in self.memo:
                self.memo[key] = adversarial_row(leaf_code[r], self.A, not twice[r], self.seen) if self.adversarial else plain_row(leaf_code[r], self.A)
            value[r], policy[r] = self.memo[key]
        return value, policy
