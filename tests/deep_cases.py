"""The DEEP sets of the three budgeted depth-first kernels (ida_search, tp_phase1_search, tp_phase2_search): inputs whose searches run
in the upper half of the trail (nibbles 16..31, word 1) and in the upper rows of path (to row 31, and to row 47 in phase 2), built
so that the plain-Python restatements (tests/ida_ref.py, tests/twophase_ref.py) follow each of them to its final status within
PASS_CAP passes.  Test infrastructure only; every seed is fixed, and tests/test_ida_host.py and tests/test_twophase_host.py assert
the pass cap and what the sets cover, so that the GPU tests need not assume either.

Every case walks a random canonical sequence W away from home and searches the way back:
  IDA*     the root is home moved by W's inverse, the prefix W[:f] goes into path with floor f: the start node is d = len(W) - f
           moves from home, on a trail f deep.
  phase 2  W = k generators after a prefix of f actions; the frame is WRITTEN at trail = W[:k0], g = f + cost(W[:k0]),
           bound = min(f + cost(W), lim), cursor 0: a search that tp_phase2_init has not started.
  phase 1  W = L actions, the last no U or D turn, so that W ends in G1; the frame is written at trail = W[:d0], depth d0, bound L."""
from __future__ import annotations

import numpy as np

from tests import ida_ref, twophase_ref as T

PASS_CAP = 30000
NOOP = ida_ref.NOOP


# ---------------------------------------------------------------------------------------------------------------------- IDA*
class IdaCase:
    """limit 32 everywhere; want = the status the construction predicts (W[f:] is canonical, so the start node is exactly d moves
    from home: SOLVED at f + d where that fits min(limit, max_depth), else EXHAUSTED with next = f + d)."""

    def __init__(self, f, d, max_depth=32, seed=0):
        self.f, self.d, self.max_depth, self.limit = f, d, max_depth, 32
        rng = np.random.default_rng(1000 * f + 10 * d + seed)
        self.W = ida_ref.canonical_walk(rng, f + d)
        self.root = ida_ref.to_bytes(ida_ref.undo(ida_ref.HOME, self.W))
        self.column = self.W[:f] + [NOOP] * (max_depth - f)                  # the path column at ida_init: rows f and up hold the no-op
        self.want = ida_ref.SOLVED if f + d <= max_depth else ida_ref.EXHAUSTED
        self.name = f"f={f} d={d} max_depth={max_depth}"

    def frame(self, h):
        return ida_ref.Frame(self.root, h, self.limit, self.max_depth, prefix=tuple(self.column), floor_given=self.f)


def ida_cases(max_depth=32):
    """The table of the issue at max_depth 32 (f = 16 is the floor at the word boundary: rows 16 and up of its column hold the no-op);
    at max_depth 20 the one case whose cap is max_depth."""
    if max_depth == 20:
        return [IdaCase(17, 3, 20)]
    pairs = [(13, 3), (14, 3), (15, 3), (16, 3), (17, 3), (28, 3), (29, 3), (30, 2), (31, 1), (32, 0), (29, 4), (30, 3)]
    return [IdaCase(f, d) for f, d in pairs]


# ------------------------------------------------------------------------------------------------------------------- phase 2
def generator_walk(rng, k, prefix, cost=None, quarter=1):
    """k phase-2 generators, canonical after the actions of `prefix` (a generator is allowed iff its first action is); with `cost`
    given, the first draw whose costs sum to it.  quarter: the weight of a quarter turn against a half turn's 1."""
    while True:
        acts, out = [NOOP, NOOP] + list(prefix), []
        for _ in range(k):
            ok = [j for j in range(8) if not ida_ref.skipped(acts[-2], acts[-1], T.GENERATORS[2][j][0])]
            w = np.array([quarter if T.COST[2][j] == 1 else 1 for j in ok], float)
            j = int(rng.choice(ok, p=w / w.sum()))
            out.append(j)
            acts += T.GENERATORS[2][j]
        if cost is None or gen_cost(out) == cost:
            return out


def gen_cost(gens):
    return sum(T.COST[2][j] for j in gens)


class Phase2Case:
    def __init__(self, f, k, k0, limit=48, max_depth=48, cost=None, seed=0, quarter=1, why=""):
        self.f, self.k, self.k0, self.limit, self.max_depth, self.why = f, k, k0, limit, max_depth, why
        rng = np.random.default_rng(100000 + 1000 * f + 10 * k + seed)
        self.prefix = ida_ref.canonical_walk(rng, f)
        self.W = generator_walk(rng, k, self.prefix, cost, quarter)
        x = ida_ref.HOME
        for j in reversed(self.W):                                           # a half turn is its own inverse; U, U', D, D' pair by ^ 1
            x = T.apply(x, T.GENERATORS[2][j ^ 1] if T.COST[2][j] == 1 else T.GENERATORS[2][j])
        self.root = ida_ref.to_bytes(x)
        self.lim = min(limit, max_depth, f + T.MAX_TRAIL)
        self.total = f + gen_cost(self.W)
        self.written = dict(trail=self.W[:k0], depth=f + gen_cost(self.W[:k0]), bound=min(self.total, self.lim), cursor=0)
        # W itself answers wherever its length fits the cap; a cap below it ends EXHAUSTED unless a shorter answer exists
        self.want = (T.SOLVED,) if self.total <= self.lim else (T.SOLVED, T.EXHAUSTED)
        self.name = f"f={f} k={k} k0={k0} limit={limit} max_depth={max_depth}"

    def frame(self, h):
        return T.Phase2.resume(self.root, h, self.limit, prefix=tuple(self.prefix), max_depth=self.max_depth, **self.written)


def phase2_cases(max_depth=48):
    if max_depth == 24:
        return [Phase2Case(4, 18, 10, max_depth=24, why="max_depth binds below the limit")]
    return [Phase2Case(0, 20, 15, cost=30, why="k0 = 15"), Phase2Case(3, 20, 16, cost=30, why="k0 = 16"), Phase2Case(5, 22, 17, cost=31, why="k0 = 17"),
            Phase2Case(6, 24, 21, cost=31, quarter=3, why="k >= 24"), Phase2Case(16, 18, 15, cost=28, why="f >= 16"),
            Phase2Case(20, 19, 17, cost=28, why="f + cost(W) = 48 = max_depth"),
            Phase2Case(10, 24, 20, cost=34, seed=4, why="floor + 32 = 42 is the cap, below f + cost(W) = 44")]


# ------------------------------------------------------------------------------------------------------------------- phase 1
class Phase1Case:
    """limit = L: the written iteration is the last one.  W itself is a candidate of the iteration's length, so K = 1 ends FULL."""

    def __init__(self, L, d0, K, seed=0):
        self.L, self.d0, self.K, self.limit = L, d0, K, L
        rng = np.random.default_rng(200000 + 100 * L + d0 + seed)
        while True:
            self.W = ida_ref.canonical_walk(rng, L)
            if self.W[-1] >> 1 not in (0, 3):
                break
        self.root = ida_ref.to_bytes(ida_ref.undo(ida_ref.HOME, self.W))
        self.written = dict(trail=self.W[:d0], depth=d0, bound=L, cursor=0)
        self.name = f"L={L} d0={d0} K={K}"

    def frame(self, h):
        return T.Phase1.resume(self.root, h, self.K, self.limit, **self.written)


def phase1_cases():
    return [Phase1Case(L, d0, K, seed) for K in (1, 8) for L, d0, seed in ((18, 15, 8), (20, 17, 0), (32, 29, 0), (32, 30, 0))]
