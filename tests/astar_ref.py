"""numpy restatement of the batch-weighted A* rule (include/rubiksearch.h "Batch-weighted A*", DESIGN.md "A* search") over the
oracle's tables: the reference the rca_* kernels are compared with, buffer by buffer.  Test infrastructure only.

AStar holds the arrays the device holds, in the device's layout (node n of problem p at p * C + n; beam slot i of problem p at
p * B + i), and changes them only where the rule says so: an element the rule does not name keeps what it held."""
from __future__ import annotations

import numpy as np

from tests.beam_ref import Cube, rank_order

OPEN, CLOSED, NEW = 1, 2, 8


def prio_of(score, weight, g):
    """score - weight * g in float32: the product rounded, then the difference rounded (no fma)."""
    with np.errstate(all="ignore"):
        prod = np.float32(weight) * np.asarray(g).astype(np.float32)
        return (np.asarray(score, np.float32) - prod).astype(np.float32)


def best_open(prio, nodes, batch, tie="higher"):
    """The min(batch, len) best of `nodes` (ascending node indices, prio their priorities): prio descending, NaN lowest, -0 == +0,
    then the HIGHER node index (tie="lower": the lower one, the flipped rule of the tie test).  Returned in ascending node index."""
    order = rank_order(prio, -nodes if tie == "higher" else nodes)
    return np.sort(nodes[order[:batch]])


class AStar:
    def __init__(self, cube: Cube, roots, batch, capacity, weight=1.0, tie="higher"):
        self.cube, self.B, self.C, self.weight, self.tie = cube, int(batch), int(capacity), float(weight), tie
        self.P = P = len(roots)
        n, S, A = P * self.C, cube.S, cube.A
        self.KW = 3 if cube.cs == 3 else 2
        self.stickers = np.zeros((n, S), np.uint8)
        self.keys = np.zeros((self.KW, n), np.uint64)
        self.parent, self.g = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.action, self.state = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.score, self.prio = np.zeros(n, np.float32), np.zeros(n, np.float32)
        self.count, self.overflow = np.zeros(P, np.int32), np.zeros(P, np.uint8)
        self.live, self.active = np.zeros(P, np.int32), np.zeros(P, np.uint8)
        self.length, self.ended = np.zeros(P, np.int32), np.zeros(P, np.int32)
        self.solution = np.zeros((P, 2), np.int32)
        self.pop_node = np.zeros(P * self.B, np.int32)
        self.beam = np.zeros((P * self.B, S), np.uint8)
        self.last_action = np.zeros(P * self.B, np.uint8)
        self.iteration = 1
        self.known = [dict() for _ in range(P)]             # key bytes -> node, every node ever made
        self.cand = {}
        # init
        roots = np.asarray(roots, np.uint8)
        g0 = np.arange(P) * self.C
        self.stickers[g0] = roots
        self.keys[:, g0] = cube.keys(roots)
        self.parent[g0], self.action[g0], self.g[g0], self.score[g0] = -1, A, 0, 0.0
        self.prio[g0], self.state[g0] = np.inf, OPEN
        self.count[:] = 1
        solved = cube.is_solved(roots)
        self.active[:] = ~solved
        self.length[:] = np.where(solved, 0, -1)
        self.solution[:] = (-1, A)
        for p in range(P):
            self.known[p][self.keys[:, g0[p]].tobytes()] = 0

    # ------------------------------------------------------------------ the stages
    def pop(self):
        for p in np.flatnonzero(self.active):
            g0 = p * self.C
            nodes = np.flatnonzero(self.state[g0:g0 + self.count[p]] == OPEN)
            if len(nodes) == 0:
                self.active[p], self.live[p], self.ended[p] = 0, 0, self.iteration
                continue
            kept = best_open(self.prio[g0 + nodes], nodes, self.B, self.tie)
            k, b0 = len(kept), p * self.B
            self.state[g0 + kept] = CLOSED
            self.pop_node[b0:b0 + k] = kept
            self.last_action[b0:b0 + k] = self.action[g0 + kept]
            self.beam[b0:b0 + k] = self.stickers[g0 + kept]
            self.live[p] = k

    def expand(self):
        """cand[p] of every active problem, arrays over c = i * A + a ascending: children, valid, solved, keys [KW, M]."""
        cube, A = self.cube, self.cube.A
        self.cand = {}
        for p in np.flatnonzero(self.active):
            live, b0 = int(self.live[p]), p * self.B
            i, a = np.repeat(np.arange(live), A), np.tile(np.arange(A), live)
            children = cube.move(self.beam[b0 + i], a)
            valid = a != (self.last_action[b0 + i].astype(np.int64) ^ 1)
            self.cand[int(p)] = dict(i=i, a=a, children=children, valid=valid, solved=cube.is_solved(children), keys=cube.keys(children))

    def merge(self, scores):
        """scores[p]: float32 over c.  Returns {p: bool mask over c of the NEW candidates} (empty mask for a problem that ended)."""
        new_masks = {}
        for p, cd in self.cand.items():
            g0, b0 = p * self.C, p * self.B
            par = self.pop_node[b0 + cd["i"]]
            hit = np.flatnonzero(cd["valid"] & cd["solved"])
            new = np.zeros(len(cd["i"]), bool)
            new_masks[p] = new
            if len(hit):
                gl = self.g[g0 + par[hit]] + 1
                c = hit[np.lexsort((hit, gl))[0]]
                self.length[p], self.solution[p] = self.g[g0 + par[c]] + 1, (par[c], cd["a"][c])
                self.active[p], self.ended[p] = 0, self.iteration
                continue
            seen = set()
            for c in np.flatnonzero(cd["valid"]):
                k = cd["keys"][:, c].tobytes()
                if k not in self.known[p] and k not in seen:
                    new[c] = True
                seen.add(k)
            fresh = np.flatnonzero(new)
            room = self.C - int(self.count[p])
            if len(fresh) > room:
                self.overflow[p] = 1
            sc = np.asarray(scores[p], np.float32)
            for r, c in enumerate(fresh[:room]):
                n = int(self.count[p]) + r
                gid = g0 + n
                self.stickers[gid], self.keys[:, gid] = cd["children"][c], cd["keys"][:, c]
                self.parent[gid], self.action[gid], self.g[gid] = par[c], cd["a"][c], self.g[g0 + par[c]] + 1
                self.score[gid] = sc[c]
                self.prio[gid] = prio_of(sc[c], self.weight, self.g[gid])
                self.state[gid] = OPEN
                self.known[p][cd["keys"][:, c].tobytes()] = n
            self.count[p] += min(len(fresh), room)
        self.iteration += 1
        return new_masks

    def backtrack(self, max_length=None):
        """actions [L, P], L = max(1, length.max()) unless given: the solution's moves by the parent links, then the no-op."""
        A = self.cube.A
        L = max(1, int(self.length.max())) if max_length is None else int(max_length)
        actions = np.full((L, self.P), A, np.uint8)
        for p in np.flatnonzero((self.length >= 1) & (self.length <= L)):
            n, g0 = int(self.solution[p, 0]), p * self.C
            actions[self.length[p] - 1, p] = self.solution[p, 1]
            for t in range(int(self.length[p]) - 1, 0, -1):
                actions[t - 1, p] = self.action[g0 + n]
                n = int(self.parent[g0 + n])
        return actions


def astar_search(cube, roots, batch, max_iterations, score_fn, weight=1.0, capacity=None, tie="higher"):
    """roots [P, S] -> dict(solved, length, actions, iterations, nodes, overflow, capacity).  score_fn(states uint8 [m, S]) -> float32 [m],
    called once per iteration on every candidate of the problems that have not ended."""
    if capacity is None:
        capacity = 1 + batch * (cube.A - 1) * max_iterations
    st = AStar(cube, roots, batch, capacity, weight, tie)
    ran = 0
    for _ in range(max_iterations):
        if not st.active.any():
            break
        st.pop()
        st.expand()
        ps = list(st.cand)
        scores = {}
        if ps:
            sc = np.asarray(score_fn(np.concatenate([st.cand[p]["children"] for p in ps])), np.float32)
            at = 0
            for p in ps:
                m = len(st.cand[p]["i"])
                scores[p] = sc[at:at + m]
                at += m
        st.merge(scores)
        ran += 1
    iterations = np.where(st.active != 0, ran, st.ended).astype(np.int32)
    return {"solved": st.length >= 0, "length": st.length.copy(), "actions": st.backtrack(), "iterations": iterations,
            "nodes": st.count.copy(), "overflow": st.overflow != 0, "capacity": capacity, "state": st}


def replay(cube, roots, actions):
    """[L + 1, P] bool: is the cube solved after 0, 1, .. L of its column's moves (the no-op leaves it as it is)."""
    st = np.asarray(roots, np.uint8).copy()
    out = [cube.is_solved(st)]
    for row in np.asarray(actions):
        live = row < cube.A
        st[live] = cube.move(st[live], row[live])
        out.append(cube.is_solved(st))
    return np.stack(out)
