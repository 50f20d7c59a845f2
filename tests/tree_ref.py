"""The lockstep tree search's host rule, restated once in plain Python / numpy from the header comment of include/rubiktree.h.
TEST INFRASTRUCTURE ONLY: it imports neither mcts_batched nor _tree, so the two product trees (librubiktree.so and the Python
tree of BatchedMCTS) are each compared with a third statement of the rule, never only with each other.

The rule (include/rubiktree.h):
  * one dict per root, keyed by the code bytes of a state; the root node is stored under ROOT and, once expanded, also under its
    own code, so a descent that returns to the root state re-enters the root node;
  * a descent starts at ROOT and walks until the next key is not in the dict.  At a node whose visit counts are all zero it
    draws `randint(0, A - 1)` from the root's generator (or from ONE shared generator, the roots taking their turns in index
    order); otherwise it takes the first maximum of the PUCT score evaluated in these float32 steps:
        float32(c) * P_a  ->  times float32(sqrt(sum N) / (1 + N_a))  ->  plus float32(W_a)  ->  minus float32(L_a)
    (P is float32; W, L and the quotient are doubles that become float32 at use).  Every edge walked gains L += virtual_loss;
  * the leaf is inserted with W = value_min, N = 0, L = 0 on every edge; on the way up W = max(W, v) (W stays on ties and on a NaN
    v), then L -= 150 -- the literal, whatever virtual_loss is -- then N += 1;
  * a root is finished by the first expanded leaf that has a solved child: solution = path + [lowest solved action].  Finished
    roots make no descent (their row of `select()` is all no-op) and keep their `sims_used`.

The occurrence counters (`TreeRef.count`) let a test assert that the case it exists for really happened.
"""
import math
import random

import numpy as np

ROOT = b"root"

COUNTERS = (
    "transposition",     # a descent step found its child already in the tree, inserted under another parent
    "root_reentry",      # a descent came back to the root under the root's own code
    "cycle",             # a descent visited one node twice
    "draw_below_root",   # a random draw at a node other than the root
    "rejection",         # a randint draw threw bits away (k-bit value >= A)
    "equal_maxima",      # a PUCT decision with two or more exactly equal maximal scores
    "f64_differs",       # a PUCT decision where the same formula in float64 picks another action
    "residual",          # a back-propagation left L != 0 on an edge
    "finished_early",    # a finished root sat out a simulation in which another root made a descent
)


class Node:
    __slots__ = ("children", "done", "P", "W", "N", "L", "total", "parent", "cP32", "cP64")

    def __init__(self, children, done, policy, value_min, parent, c):
        a = len(children)
        self.children, self.done = children, done
        self.P = np.array(policy, np.float32)
        self.W = np.full(a, value_min, np.float64)
        self.N = np.zeros(a, np.int64)
        self.L = np.zeros(a, np.float64)
        self.total = 0                # sum of N
        self.parent = parent          # the node whose edge inserted this one (None: the root)
        self.cP32 = np.float32(c) * self.P                    # the first float32 step: the same product at every decision
        self.cP64 = c * self.P.astype(np.float64)
        assert self.cP32.dtype == np.float32


def puct_scores(node):
    """(float32 scores in the header's steps, the same formula in float64), as lists."""
    q = math.sqrt(node.total) / (1.0 + node.N)                            # the double quotient
    s32 = node.cP32 * q.astype(np.float32)
    s32 = s32 + node.W.astype(np.float32)
    s32 = s32 - node.L.astype(np.float32)
    s64 = node.cP64 * q + node.W - node.L
    return s32.tolist(), s64.tolist()


def first_max(s):
    return s.index(max(s))            # max() keeps the first of equal items; no score is ever NaN (W, L and P are never NaN)


class DescentTooLong(Exception):
    """A descent passed `limit` steps.  With virtual_loss < 150 every visit leaves L = virtual_loss - 150 < 0 behind, which makes
    a visited edge MORE attractive; once both edges of a 2-cycle are favourites a descent circles until the virtual loss has
    paid the residuals off, about (150 - virtual_loss) / virtual_loss passes per earlier visit, and every pass is an earlier visit
    of the next descent: the lengths grow geometrically.  That is the rule, not a fault of an implementation (virtual_loss = 0 is
    the limit: no descent through a 2-cycle ends).  The trees are left in the middle of a simulation."""


class TreeRef:
    def __init__(self, n_roots, n_actions, cpuct, virtual_loss, value_min, rngs=None, shared=random, limit=4096):
        """rngs: one random.Random per root, or None: ONE generator `shared` (the `random` module or a random.Random)."""
        self.limit = limit
        assert virtual_loss != 0          # a real 2-cycle never ends a descent without it (a property of the rule)
        self.n, self.A = int(n_roots), int(n_actions)
        self.c, self.vl, self.vmin = float(cpuct), float(virtual_loss), float(value_min)
        self.rngs, self.shared = rngs, shared
        assert rngs is None or len(rngs) == self.n
        self.trees = [dict() for _ in range(self.n)]
        self._solution = [None] * self.n
        self._sims = [0] * self.n
        self._trail = [None] * self.n          # (leaf key, parent node, [(node, action)]) of the last descent
        self.count = dict.fromkeys(COUNTERS, 0)

    # ------------------------------------------------------------------ random.randint(0, A - 1), watched
    def _draw(self, gen):
        state = gen.getstate()
        a = gen.randint(0, self.A - 1)
        twin = random.Random()                 # the same draw spelled out: k = A.bit_length() bits, rejection
        twin.setstate(state)
        k = self.A.bit_length()
        r = twin.getrandbits(k)
        while r >= self.A:
            self.count["rejection"] += 1
            r = twin.getrandbits(k)
        assert r == a and twin.getstate()[1] == gen.getstate()[1]
        return a

    # ------------------------------------------------------------------ one simulation, first half
    def select(self):
        """One descent per unfinished root -> uint8 [n, depth] paths padded with the no-op A."""
        paths = []
        running = sum(s is None for s in self._solution)
        for r in range(self.n):
            if self._solution[r] is not None:
                self._trail[r] = None
                paths.append([])
                self.count["finished_early"] += running > 0
                continue
            self._sims[r] += 1
            gen = self.rngs[r] if self.rngs is not None else self.shared
            tree, key, parent, trail, seen, cycled = self.trees[r], ROOT, None, [], set(), False
            while key in tree:
                node = tree[key]
                if trail:
                    if node is tree[ROOT]:
                        self.count["root_reentry"] += 1
                    elif node.parent is not parent:
                        self.count["transposition"] += 1
                if id(node) in seen:
                    cycled = True
                seen.add(id(node))
                if node.total == 0:
                    a = self._draw(gen)
                    self.count["draw_below_root"] += int(bool(trail))
                else:
                    s32, s64 = puct_scores(node)
                    a = first_max(s32)
                    self.count["equal_maxima"] += s32.count(s32[a]) > 1
                    self.count["f64_differs"] += first_max(s64) != a
                node.L[a] += self.vl
                trail.append((node, a))
                if len(trail) > self.limit:
                    self.count["cycle"] += 1                      # more steps than nodes
                    raise DescentTooLong(r, self._sims[r])
                parent, key = node, node.children[a]
            self.count["cycle"] += cycled
            self._trail[r] = (key, parent, trail)
            paths.append([a for _, a in trail])
        depth = max((len(p) for p in paths), default=0)
        out = np.full((self.n, depth), self.A, np.uint8)
        for r, p in enumerate(paths):
            out[r, :len(p)] = p
        return out

    # ------------------------------------------------------------------ second half
    def update(self, leaf_code, child_code, solved, value, policy):
        """Row r describes the leaf root r's last descent ended on.  Returns the number of finished roots."""
        for r in range(self.n):
            if self._trail[r] is None:
                continue
            key, parent, trail = self._trail[r]
            self._trail[r] = None
            tree = self.trees[r]
            own = bytes(np.asarray(leaf_code[r], np.uint8))
            assert key == ROOT or key == own                       # the key a parent stored IS the leaf's code
            kids = [bytes(np.asarray(child_code[r, a], np.uint8)) for a in range(self.A)]
            done = [bool(x) for x in solved[r]]
            node = Node(kids, done, policy[r], self.vmin, parent, self.c)
            assert key not in tree
            tree[key] = node
            if key == ROOT:
                tree[own] = node
            v = np.float32(value[r])
            for nd, a in reversed(trail):
                if float(v) > nd.W[a]:                               # max(W, v): W stays on ties and on NaN
                    nd.W[a] = float(v)
                nd.L[a] -= 150.0
                nd.N[a] += 1
                nd.total += 1
            self.count["residual"] += any(nd.L[a] != 0.0 for nd, a in trail)
            if any(done):
                self._solution[r] = [a for _, a in trail] + [done.index(True)]
        return sum(s is not None for s in self._solution)

    # ------------------------------------------------------------------ results
    def solution(self, r):
        return self._solution[r]

    def sims_used(self):
        return list(self._sims)

    def nodes(self, r):
        return len(self.trees[r]) - (ROOT in self.trees[r])       # the root is stored twice

    def root_stats(self, r):
        """(visit counts, values, node count) of root r; zeros and -1 while the root is not expanded (rc_tree_root_stats)."""
        root = self.trees[r].get(ROOT)
        if root is None:
            return [0] * self.A, [-1.0] * self.A, 0
        return root.N.tolist(), root.W.tolist(), self.nodes(r)

    def dump(self, r):
        """{key: (W, N, L)} of every node of root r, as lists."""
        return {k: (v.W.tolist(), v.N.tolist(), v.L.tolist()) for k, v in self.trees[r].items()}

    def finished(self):
        return sum(s is not None for s in self._solution)
