"""numpy restatement of the corner pattern database (include/rubiksearch.h "Corner pattern database"): the reference the rcp_* kernels
and pattern.CornerTable are compared with.  Test infrastructure only.

The distances come from a breadth-first search on STICKER arrays with tables.get_tables(cs).perm, deduplicated by
tables.get_cubies(cs).cubies(...)[2] (the corner index): nothing here reads the corner move tables the kernels walk the index space
with.  corner_moves() derives those tables a second way, from where a move carries each corner sticker."""
from __future__ import annotations

import collections
import functools

import numpy as np

from rubiks_cube_solver_amd.tables import get_cubies, get_tables

from tests import group_ref

# States per distance of the corner group under the env's quarter turns.  3x3x3: computed on the CPU by a separate C program (a
# breadth-first search over the 88 179 840 indices with the package's tables); the sum is 88 179 840, the deepest level is 14, and from
# depth 10 on each count is 24 x the 2x2x2's (group_ref.SPHERES_222, OEIS A079762).  bfs(3, 6) below reproduces the first seven.
LEVELS_333 = (1, 12, 114, 924, 6539, 39528, 199926, 806136, 2761740, 8656152, 22334112, 32420448, 18780864, 2166720, 6624)
LEVELS = {2: group_ref.SPHERES_222, 3: LEVELS_333}
SIZE = {2: 3674160, 3: 88179840}
ILLEGAL = 0xFF
assert sum(LEVELS_333) == SIZE[3] and sum(group_ref.SPHERES_222) == SIZE[2]
assert all(a == 24 * b for a, b in zip(LEVELS_333[10:], group_ref.SPHERES_222[10:]))


def corner_moves(cs):
    """(src, twist) uint8 [A, NC] from sticker positions: the sticker that arrives at position j of slot q under move a (a gather:
    new[i] = old[perm[a][i]]) sat at position (j + s) % 3 of slot src.  A piece whose U/D colour showed at position o of src shows it
    at position (o - s) % 3 of q: twist = -s mod 3."""
    t, cb = get_tables(cs), get_cubies(cs)
    cw = cb.corner_cw.astype(np.int64)
    where = {int(cw[q][k]): (q, k) for q in range(cb.nc) for k in range(3)}
    src, twist = np.zeros((t.n_actions, cb.nc), np.uint8), np.zeros((t.n_actions, cb.nc), np.uint8)
    for a in range(t.n_actions):
        for q in range(cb.nc):
            frm = [where[int(t.perm[a][cw[q][j]])] for j in range(3)]
            assert len({f[0] for f in frm}) == 1
            s = frm[0][1]
            assert [f[1] for f in frm] == [(j + s) % 3 for j in range(3)]
            src[a, q], twist[a, q] = frm[0][0], (-s) % 3
    return src, twist


def coords(cs, states):
    """(piece, ori) int64 [n, NC] of legal corner states, and the corner index."""
    cb = get_cubies(cs)
    cub, _, idx, _ = cb.cubies(states)
    c = cub[:, :cb.nc].astype(np.int64)
    return c // 3, c % 3, idx


def move_coords(piece, ori, src, twist, a):
    """THE RULE's move on (piece, ori) [n, NC]; a: one action."""
    s = src[a].astype(np.int64)
    return piece[:, s], (ori[:, s] + twist[a]) % 3


def rank(piece, ori):
    """corner_index of (piece, ori) [n, NC] (include/rubikhip.h "Cubie coordinates")."""
    n, nc = piece.shape
    lehmer = np.zeros(n, np.int64)
    for q in range(nc):
        lehmer = lehmer * (nc - q) + (piece[:, q + 1:] < piece[:, q:q + 1]).sum(1)
    return lehmer * 3 ** (nc - 1) + (ori[:, :nc - 1] * 3 ** np.arange(nc - 1)).sum(1)


def unrank(cs, idx):
    """rcp_unrank: cubie rows uint8 [n, SLOTS] of corner indices < N (any other comes out solved), and the bool [n] of those others.
    3x3x3: the edges are home, the last two trade places under an odd corner permutation."""
    cb = get_cubies(cs)
    nc, ne = cb.nc, cb.ne
    idx = np.asarray(idx, np.int64)
    bad = (idx < 0) | (idx >= SIZE[cs])
    idx = np.where(bad, 0, idx)
    n = len(idx)
    oris, lehmer = idx % 3 ** (nc - 1), idx // 3 ** (nc - 1)
    ori, dig, piece = (np.zeros((n, nc), np.int64) for _ in range(3))
    for q in range(nc - 1):
        ori[:, q], oris = oris % 3, oris // 3
    ori[:, nc - 1] = (-ori.sum(1)) % 3
    for q in range(nc - 1, -1, -1):
        dig[:, q], lehmer = lehmer % (nc - q), lehmer // (nc - q)
    avail = np.ones((n, nc), bool)
    for q in range(nc):                                                      # the dig[q]-th smallest piece not used yet
        piece[:, q] = np.argmax((np.cumsum(avail, 1) == dig[:, q:q + 1] + 1) & avail, 1)
        avail[np.arange(n), piece[:, q]] = False
    cub = np.zeros((n, nc + ne), np.uint8)
    cub[:, :nc] = piece * 3 + ori
    if ne:
        cub[:, nc:] = 2 * np.arange(ne)
        odd = (dig.sum(1) & 1).astype(bool)
        cub[odd, nc + ne - 2], cub[odd, nc + ne - 1] = 2 * (ne - 1), 2 * (ne - 2)
    return cub, bad


def corner_index(cs, states):
    """uint32 corner index per sticker row, 0xFFFFFFFF where the CORNER state is not legal -- the edges and centres of a 3x3x3 are
    not looked at: they are replaced by the solved cube's before the cubie rule is asked."""
    cb, t = get_cubies(cs), get_tables(cs)
    st = np.asarray(states, np.uint8)
    if cs == 3:
        corner = np.zeros(t.n_stickers, bool)
        corner[cb.corner_cw.reshape(-1)] = True
        st = np.where(corner[None, :], st, t.solved[None, :])
        bad_colour = (st > 5).any(1)
        cub, status, _, _ = cb.cubies(st)
        c = cub[:, :cb.nc].astype(np.int64)
        named = (c != 0xFF).all(1)
        piece, ori = np.where(c != 0xFF, c // 3, 0), np.where(c != 0xFF, c % 3, 0)
        ok = ~bad_colour & named & (np.sort(piece, 1) == np.arange(cb.nc)).all(1) & (ori.sum(1) % 3 == 0)
        idx = rank(piece, ori)
        return np.where(ok, idx, 0xFFFFFFFF).astype(np.uint32)
    return cb.cubies(st)[2]


@functools.lru_cache(maxsize=None)
def bfs(cs, max_depth=None):
    """(dist uint8 [N] with 0xFF where not reached within max_depth, level counts) by breadth-first search on stickers."""
    t, cb = get_tables(cs), get_cubies(cs)
    perm = t.perm.astype(np.int64)
    dist = np.full(SIZE[cs], ILLEGAL, np.uint8)
    frontier = t.solved[None, :].copy()
    dist[cb.cubies(frontier)[2]] = 0
    levels, d = [1], 0
    while len(frontier) and (max_depth is None or d < max_depth):
        nxt = []
        for a in range(t.n_actions):
            child = frontier[:, perm[a]]
            idx = cb.cubies(child)[2].astype(np.int64)
            idx, first = np.unique(idx, return_index=True)
            new = dist[idx] == ILLEGAL
            dist[idx[new]] = d + 1
            nxt.append(child[first[new]])
        frontier = np.concatenate(nxt)
        d += 1
        if len(frontier):
            levels.append(len(frontier))
    dist.setflags(write=False)
    return dist, tuple(levels)


def score_of_keys(cs, keys, dist):
    """-(float)dist[corner index] per key column (uint64 [KW, m]), -255 for a key that names no legal corner state."""
    t = get_tables(cs)
    idx = [k for k in range(t.n_stickers) if not (cs == 3 and k % 9 == 4)]
    st = np.tile(t.solved, (keys.shape[1], 1))
    for n, k in enumerate(idx):
        st[:, k] = (keys[n // 16] >> np.uint64(3 * (n % 16))) & np.uint64(7)
    ci = corner_index(cs, st)
    d = np.where(ci < SIZE[cs], dist[np.minimum(ci, SIZE[cs] - 1)], ILLEGAL)
    return -d.astype(np.float32)


# ---------------------------------------------------------------------------------------------- A* with rcp_relax
COUNTERS = ("relaxed", "contested", "tie_g", "diff_g", "winner_not_lowest_c", "across_strides", "win_c256", "fma_differs")
LANES = 256                                                                  # the relax workgroup: candidate c is lane c % 256's, stride c // 256


def prio_rounded_once(score, weight, g):
    """float32(score - weight * g) with ONE rounding, as an fma gives it: float64 holds the product of two float32 exactly, and its
    difference with a float32 to far below half a float32 ulp."""
    with np.errstate(all="ignore"):
        return np.float32(np.float64(np.float32(score)) - np.float64(np.float32(weight)) * np.float64(np.float32(g)))


def relaxed_class():
    """tests/astar_ref.py's AStar with include/rubiksearch.h's rcp_relax as a stage of its own, relax(new_masks), to run after every
    merge.  An OFFER is a VALID candidate that is not NEW, whose key names an OPEN node and whose g(parent) + 1 is below that node's g.
    Counters over the run (COUNTERS): relaxed = nodes lowered; contested = nodes with >= 2 offers in one iteration; of those, tie_g:
    >= 2 offers share the least g, diff_g: the offers differ in g, winner_not_lowest_c: the winner is not the lowest c among them,
    across_strides: the offers lie in different c // 256; win_c256: relaxed nodes won by a c >= 256; fma_differs: relaxed nodes whose
    prio would have other bits had score - weight * g been rounded once."""
    from tests import astar_ref

    class Relaxed(astar_ref.AStar):
        relaxed = contested = tie_g = diff_g = winner_not_lowest_c = across_strides = win_c256 = fma_differs = 0

        def counters(self):
            return {k: getattr(self, k) for k in COUNTERS}

        def relax(self, new_masks):
            """After merge(scores) -> new_masks of the same iteration.  The winner of a node: the least g, then the least c."""
            for p, cd in self.cand.items():
                if not self.active[p]:
                    continue
                g0, b0 = p * self.C, p * self.B
                par = self.pop_node[b0 + cd["i"]]
                offers = {}                                                  # node -> [(g, c)] in ascending c
                for c in np.flatnonzero(cd["valid"] & ~new_masks[p]):
                    n = self.known[p].get(cd["keys"][:, c].tobytes())
                    if n is None or self.state[g0 + n] != astar_ref.OPEN:
                        continue
                    g = int(self.g[g0 + par[c]]) + 1
                    if g < self.g[g0 + n]:
                        offers.setdefault(n, []).append((g, int(c)))
                for n, offs in offers.items():
                    g, c = min(offs)
                    if len(offs) > 1:
                        gs, cs_ = [o[0] for o in offs], [o[1] for o in offs]
                        self.contested += 1
                        self.tie_g += gs.count(g) > 1
                        self.diff_g += len(set(gs)) > 1
                        self.winner_not_lowest_c += c != min(cs_)
                        self.across_strides += len({x // LANES for x in cs_}) > 1
                    self.g[g0 + n], self.parent[g0 + n], self.action[g0 + n] = g, par[c], cd["a"][c]
                    self.prio[g0 + n] = astar_ref.prio_of(self.score[g0 + n], self.weight, g)
                    self.relaxed += 1
                    self.win_c256 += c >= LANES
                    once = prio_rounded_once(self.score[g0 + n], self.weight, g)
                    self.fma_differs += int(once.view(np.uint32) != self.prio[g0 + n:g0 + n + 1].view(np.uint32)[0])

    return Relaxed


def relaxed_step(st, score_fn):
    """One iteration of a Relaxed state: pop, expand, the scores, merge, relax (astar_ref.astar_search's loop body + relax)."""
    st.pop()
    st.expand()
    ps = list(st.cand)
    scores = {}
    if ps:
        sc = np.asarray(score_fn(np.concatenate([st.cand[p]["children"] for p in ps])), np.float32)
        at = 0
        for p in ps:
            m = len(st.cand[p]["i"])
            scores[p], at = sc[at:at + m], at + m
    st.relax(st.merge(scores))


def relaxed_astar(cube, roots, batch, max_iterations, score_fn, weight=1.0, capacity=None):
    """What search.astar_search runs for front="table", restated.  -> astar_ref.astar_search's dict."""
    if capacity is None:
        capacity = 1 + batch * (cube.A - 1) * max_iterations
    st = relaxed_class()(cube, roots, batch, capacity, weight)
    ran = 0
    for _ in range(max_iterations):
        if not st.active.any():
            break
        relaxed_step(st, score_fn)
        ran += 1
    iterations = np.where(st.active != 0, ran, st.ended).astype(np.int32)
    return {"solved": st.length >= 0, "length": st.length.copy(), "actions": st.backtrack(), "iterations": iterations,
            "nodes": st.count.copy(), "overflow": st.overflow != 0, "capacity": capacity, "state": st}


# ---------------------------------------------------------------------------- the built scenario of the relax stage tests
# "Flood, lift, re-open".  A search by itself does not offer two candidates to one OPEN node (54 configurations of written scores
# gave no relaxation at all), so the tests build the state in which nearly every candidate is an offer.  Zero scores flood the pool
# level by level for `pre` iterations; then every OPEN node's g is raised by 1 + n % 3 (lift) and the nodes of the last pop go back
# to OPEN with the best priority there is, their g raised by n % 2 (re-open with JITTER: the offers to a node differ in g; without it,
# the TIE form, they all tie and c alone decides).  The next pop takes those nodes again: their children are known, OPEN and lifted.
# Two iterations follow.  All of it is written to the numpy arrays of a Relaxed state; a GPU test copies the same arrays to the device.
#
# The cube group looks the same from every state, so the flood from any root that is not solved on the way numbers its nodes alike:
# seed, depth and P do not change what one problem contributes to the counters, only B, `pre`, C, the weight and the scores do.
DEPTHS = (0, 1, 9, 2, 11, 3, 14)                                             # as test_gpu_astar.mixed_scrambles: some problems end during `pre`
SEEDS = {3: 7, 2: 8}                                                         # 2x2x2: seed 7's 9-move roots lie within 6 moves of solved and end in the flood
REOPENED = np.float32(3e38)
# The pool overflows in the last iteration of `pre` at B = 64 (3x3x3: 127 nodes + 64 x ~9 new, 2x2x2: 154 + 64 x ~4.4), and the
# iterations after hold dropped NEW candidates, duplicates of them AND winners at c >= 256.  (C = 200 gave no such winner.)
SMALL_CAPACITY = 400
# weight, score mode of beam_ref.hard_scores for the OPEN nodes.  fma_differs needs an inexact weight * g at the g of the offers: 3 | 4
# on the 3x3x3, where float32(0.6) * 3 and * 4 are exact, so 0.7 (24 significant bits times 3 needs 26) is added there; 4 | 5 on the 2x2x2.
WEIGHTED = {2: ((0.6, 2), (2.5, 1), (0.0, 2)), 3: ((0.6, 2), (2.5, 1), (0.0, 2), (0.7, 2))}
FMA_WEIGHT = {2: 0.6, 3: 0.7}

Case = collections.namedtuple("Case", "cs P B C weight mode jitter")


def scenario_cases(max_P=40):
    """Every point the relax stage test runs; tests/test_pattern_host.py runs the ones with P <= 5 on the restatement alone."""
    out = []
    for cs in (2, 3):
        A = 12 if cs == 3 else 6
        full = lambda B: 1 + B * (A - 1) * 8                                 # noqa: E731
        for jitter in (True, False):
            out += [Case(cs, P, B, full(B), 1.0, None, jitter) for P in (1, 3, 40) for B in (1, 4, 64)]
            # the ragged last stride, M = 264 | 258.  3x3x3: at weight 1 no node is contested across strides, at weight 0 some are
            out.append(Case(3, 3, 22, full(22), 0.0, 2, jitter) if cs == 3 else Case(2, 3, 43, full(43), 1.0, None, jitter))
            out.append(Case(cs, 5, 256, full(256), 1.0, None, jitter))       # 12 | 6 full strides
            out.append(Case(cs, 3, 64, SMALL_CAPACITY, 1.0, None, jitter))
        for w, mode in WEIGHTED[cs]:
            out += [Case(cs, 3, 64, full(64), w, mode, True), Case(cs, 3, 4, full(4), w, mode, False)]
    return [c for c in out if c.P <= max_P]


def case_id(c):
    return f"{c.cs}-P{c.P}-B{c.B}-C{c.C}-w{c.weight}-{'jitter' if c.jitter else 'tie'}"


def scenario_depths(P):
    return [DEPTHS[i % 7] for i in range(P)] if P >= 3 else [9] * P


def scenario_pre(cs, B):
    """3 | 4 at B = 64, 6 below.  B = 256 floods one level further: only then does a pop take 256 nodes (the levels hold 1, 12,
    114, 924 and 1, 6, 27, 120, 534 nodes), and every stride is full."""
    return (3 if cs == 3 else 4) + (B >= 256) if B >= 64 else 6


def zero_scores(st):
    return {p: np.zeros(len(cd["i"]), np.float32) for p, cd in st.cand.items()}


def doctor(st, jitter=True, score_mode=None, seed=0):
    """Lift, re-open and (score_mode 1 | 2: beam_ref.hard_scores, values a few ulps apart) new scores for the OPEN nodes, of every
    problem, ended ones too.  Changes g, state, prio and score and nothing else."""
    from tests import astar_ref, beam_ref
    rng = np.random.default_rng(seed)
    for p in range(st.P):
        g0, b0 = p * st.C, p * st.B
        n = np.flatnonzero(st.state[g0:g0 + st.count[p]] == astar_ref.OPEN)
        st.g[g0 + n] += 1 + n % 3
        back = st.pop_node[b0:b0 + max(int(st.live[p]), 0)]
        st.state[g0 + back], st.prio[g0 + back] = astar_ref.OPEN, REOPENED
        if jitter:
            st.g[g0 + back] += back % 2
        if score_mode is not None:
            n = np.flatnonzero(st.state[g0:g0 + st.count[p]] == astar_ref.OPEN)
            st.score[g0 + n] = beam_ref.hard_scores(rng, len(n), st.B, score_mode)


def dropped_and_duplicated(st, new_masks):
    """Over the candidates of the iteration just merged: (NEW candidates that found no room in the pool, VALID candidates that are
    not NEW and carry the key of one of those)."""
    dropped = dups = 0
    for p, cd in st.cand.items():
        lost = {cd["keys"][:, c].tobytes() for c in np.flatnonzero(new_masks[p])} - set(st.known[p])
        dropped += len(lost)
        dups += sum(cd["keys"][:, c].tobytes() in lost for c in np.flatnonzero(cd["valid"] & ~new_masks[p]))
    return dropped, dups


def end_one(st):
    """Between merge and relax of the first iteration after the doctoring: where two or more problems run, the last of them is made
    to have ended (active = 0, what a solved child does in merge).  Its candidates are VALID and nearly all of them offers, and relax
    must not touch it.  (A search does not end there by itself: that iteration repeats the candidates of the one before the
    doctoring; and expand clears the VALID flags of problems that ended earlier, so those have nothing to offer.)  -> p or None."""
    run = np.flatnonzero(st.active)
    if len(run) < 2:
        return None
    st.active[run[-1]] = 0
    return int(run[-1])


def run_scenario(case, roots):
    """The scenario on the restatement alone -> the Relaxed state after the two iterations, .dropped / .duplicated of the first."""
    from tests import beam_ref
    st = relaxed_class()(beam_ref.Cube(case.cs), roots, case.B, case.C, case.weight)
    for it in range(scenario_pre(case.cs, case.B) + 2):
        if it == scenario_pre(case.cs, case.B):
            st.overflowed = st.overflow.copy()
            doctor(st, case.jitter, case.mode)
        st.pop(), st.expand()
        new = st.merge(zero_scores(st))
        if it == scenario_pre(case.cs, case.B):
            st.dropped, st.duplicated = dropped_and_duplicated(st, new)
            st.ended_by_hand = end_one(st)
        st.relax(new)
    return st


def check_reached(case, st):
    """The conditions a case exists for, on the restatement's counters; st.overflowed: overflow before the doctoring, st.dropped and
    st.duplicated: dropped_and_duplicated() of the first iteration after it."""
    n, M = st.counters(), case.B * (12 if case.cs == 3 else 6)
    assert n["relaxed"] > 0, n
    assert (st.active != 0).any() and ((st.active == 0).any() or case.P < 3), "some problems ended, some run"
    assert (st.ended_by_hand is not None) == (case.P >= 5)
    if case.B >= 4 and case.P >= 3:
        assert (n["diff_g"] > 0 and n["winner_not_lowest_c"] > 0) if case.jitter else n["tie_g"] > 0, n
    if M > LANES:
        # M = 258, tie form: the ragged stride holds c = 256 and 257 alone.  One of them ties with stride 0 for a node and must lose;
        # that the other wins a node in the same run occurred in none of 1188 inputs (pre 2..10, six capacities, eight weight and
        # score modes, three score seeds), so that form asserts the contest only.  The jitter form has both.
        assert n["across_strides"] > 0 and (n["win_c256"] > 0 or (M == 258 and not case.jitter)), n
    if case.C == SMALL_CAPACITY:
        assert st.overflowed[st.active != 0].all() and st.dropped > 0 and st.duplicated > 0, (st.overflowed, st.dropped, st.duplicated)
    else:
        assert not st.overflow.any()
    if case.weight == FMA_WEIGHT[case.cs] and case.B == 64:                  # at B = 4 the 2x2x2's offers have g = 2 | 3: 0.6 * g is exact
        assert n["fma_differs"] > 0, n


