"""Batch-weighted A* on the GPU (search.AStarPlan / astar_search, the rca_* entry points of librubiksearch.so): every stage against the
numpy restatement (tests/astar_ref.py) buffer by buffer, whole searches against the cube group's own numbers (sphere counts, exact
distances), graph / eager / sync_every equalities, argument errors, minimum alignment, and the shipped 2x2x2 checkpoint.  GPU only."""
import os

import numpy as np
import pytest
import torch

from tests import astar_ref as R
from tests import beam_ref
from tests.test_gpu_search import DeepCube, Stub, _random_deepcube, env_of, scrambles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0xEE                 # every byte the rule does not name keeps this (pool, pop_node); beam stickers / last_action keep BEAM_FILL
BEAM_FILL = 0x03            # a sticker colour: rc_search_expand reads dead slots too and looks their stickers up


def search_mod():
    from rubiks_cube_solver_amd import search
    return search


def aos(t):
    """tiled [tiles, S, pitch] -> [tiles * pitch, S] numpy"""
    return t.permute(0, 2, 1).reshape(-1, t.shape[1]).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Pair:
    """An AStarPlan and the restatement on the same roots, every buffer pre-filled with the same bytes on both sides."""

    def __init__(self, cs, scr, B, C, weight=1.0, model=None, front="dense", dtype=torch.float32, relax=False):
        """relax: the restatement is tests/pattern_ref.py's Relaxed and iterate() runs rcp_relax as a fourth stage after merge."""
        S = search_mod()
        self.cube = cube = beam_ref.Cube(cs)
        self.cs, self.P, self.B, self.C, self.model, self.relax = cs, len(scr), B, C, model, relax
        self.env = env_of(cs, scr)
        hidden = None
        if front == "codes":
            from rubiks_cube_solver_amd.codenet import CodeNet
            self.model = CodeNet(model, cs)
            hidden = self.model.hidden
        self.plan = plan = S.AStarPlan(self.P, cs, B, C, DEV, dtype=dtype, front=front, hidden=hidden, weight=weight)
        for t in (plan.stickers, plan.keys, plan.parent, plan.action, plan.g, plan.node_score, plan.prio, plan.state, plan.count, plan.overflow,
                  plan.ended, plan.solution, plan.pop_node, plan.beam.live, plan.beam.active, plan.beam.length):
            t.view(torch.uint8).fill_(FILL)
        plan.beam.beams[0].fill_(BEAM_FILL)
        plan.beam.last_action.fill_(BEAM_FILL)
        roots = cube.scramble(scr)
        if relax:
            from tests import pattern_ref
        self.ref = ref = (pattern_ref.relaxed_class() if relax else R.AStar)(cube, roots, B, C, weight)
        for name in ("pop_node",):
            getattr(ref, name).view(np.uint8)[:] = FILL
        ref.beam[:], ref.last_action[:] = BEAM_FILL, BEAM_FILL
        # the restatement's constructor IS init: everything it did not write gets the fill
        g0 = np.arange(self.P) * C
        rest = np.ones(self.P * C, bool)
        rest[g0] = False
        for a in (ref.parent, ref.action, ref.g, ref.score, ref.prio, ref.state):
            a.view(np.uint8).reshape(self.P * C, -1)[rest] = FILL
        ref.stickers[rest] = FILL
        ref.keys.view(np.uint8).reshape(ref.KW, self.P * C, 8)[:, rest] = FILL
        plan.init(self.env.stickers, self.env.stickers.shape[-1])
        self.compare("init")

    # every array of the device against the restatement's, whole
    def compare(self, stage):
        plan, ref, P, B, C = self.plan, self.ref, self.P, self.B, self.C
        torch.cuda.synchronize()
        n, nb = P * C, P * B
        st = aos(plan.stickers)
        assert (st[:n] == ref.stickers).all() and (st[n:] == FILL).all(), stage
        assert (plan.keys.cpu().numpy().view(np.uint64) == ref.keys).all(), stage
        for name in ("parent", "action", "g", "state", "count", "overflow", "ended", "solution", "pop_node"):
            assert (getattr(plan, name).cpu().numpy() == getattr(ref, name)).all(), (stage, name)
        assert (bits(plan.node_score.cpu().numpy()) == bits(ref.score)).all(), stage
        prio = plan.prio.cpu().numpy()                                      # bit for bit; a NaN's payload is not part of the rule
        assert ((bits(prio) == bits(ref.prio)) | (np.isnan(prio) & np.isnan(ref.prio))).all(), stage
        for name in ("live", "active", "length"):
            assert (getattr(plan.beam, name).cpu().numpy() == getattr(ref, name)).all(), (stage, name)
        bm, la = aos(plan.beam.beams[0]), plan.beam.last_action.cpu().numpy()
        assert (bm[:nb] == ref.beam).all() and (bm[nb:] == BEAM_FILL).all(), stage
        assert (la[:nb] == ref.last_action).all() and (la[nb:] == BEAM_FILL).all(), stage

    def device_scores(self):
        """{p: the device's scores over c} of the restatement's candidates."""
        sc = self.plan.beam.scores.cpu().numpy()
        return {p: sc[:, p * self.B:p * self.B + int(self.ref.live[p])].T.reshape(-1).copy() for p in self.ref.cand}

    def cand_flags(self):
        """{p: flags over c} of the restatement's candidates, and the whole flag array."""
        fl = self.plan.beam.flags.cpu().numpy()
        return {p: fl[:, p * self.B:p * self.B + int(self.ref.live[p])].T.reshape(-1).copy() for p in self.ref.cand}, fl

    def iterate(self, write_scores=None, before_relax=None):
        """One iteration on both sides, compared after every stage.  write_scores(pair) overwrites plan.beam.scores instead of the model;
        before_relax(pair) runs between merge and relax."""
        plan, ref = self.plan, self.ref
        plan.pop()
        ref.pop()
        self.compare("pop")
        plan.expand()
        ref.expand()
        torch.cuda.synchronize()
        keys = plan.beam.keys.cpu().numpy().view(np.uint64)
        flags, _ = self.cand_flags()
        for p, cd in ref.cand.items():
            assert (flags[p] == (cd["valid"].astype(np.uint8) | (cd["solved"].astype(np.uint8) << 1))).all(), p
            k = keys[:, :, p * self.B:p * self.B + int(ref.live[p])].transpose(0, 2, 1).reshape(ref.KW, -1)
            assert (k == cd["keys"]).all(), p
        if write_scores is not None:
            write_scores(self)
        else:
            plan.score(self.model)
        scores = self.device_scores()
        _, before = self.cand_flags()
        plan.merge()
        new = ref.merge(scores)
        self.compare("merge")
        flags, after = self.cand_flags()
        want = before.copy()
        for p, mask in new.items():                                         # RCA_NEW on the new candidates, no other flag byte changes
            live = len(mask) // self.cube.A
            blk = want[:, p * self.B:p * self.B + live]
            blk |= (mask.reshape(live, self.cube.A).T.astype(np.uint8) * R.NEW)
        assert (after == want).all()
        self.new_masks = new
        if self.relax:                                                      # the fourth stage: what it may not write keeps its bytes
            if before_relax is not None:
                before_relax(self)
            held = {k: getattr(plan.beam, k).clone() for k in ("flags", "keys", "scores")} | {"table": plan.table.clone()}
            plan.relax()
            ref.relax(new)
            self.compare("relax")
            for k, was in held.items():
                now = plan.table if k == "table" else getattr(plan.beam, k)
                assert torch.equal(now.view(torch.uint8), was.view(torch.uint8)), ("relax wrote", k)
        plan.iteration.add_(1)

    def finish(self):
        L = max(1, int(self.ref.length.max()))
        got = self.plan.backtrack(L).cpu().numpy()
        want = self.ref.backtrack(L)
        assert (got == want).all()
        solved = R.replay(self.cube, self.ref.stickers[np.arange(self.P) * self.C], want)
        for p in np.flatnonzero(self.ref.length >= 0):
            assert solved[self.ref.length[p], p] and not solved[:self.ref.length[p], p].any()
        self.compare("backtrack")                                           # backtrack writes nothing but actions


def hard_writer(mode, seed):
    """Scores written by the test: beam_ref.hard_scores modes 0..4 (random bit patterns, values a few ulps apart, +-0 blocks, +-inf,
    NaN, +-FLT_MAX); mode 5: score = weight * g(child), so EVERY node of a problem has priority 0 across different g."""
    rng = np.random.default_rng(seed)

    def write(pair):
        sc = pair.plan.beam.scores
        if mode < 5:
            vals = beam_ref.hard_scores(rng, sc.numel(), pair.B, mode)
        else:
            vals = np.zeros(sc.shape, np.float32)
            for p in pair.ref.cand:
                b0, live = p * pair.B, int(pair.ref.live[p])
                g = pair.ref.g[p * pair.C + pair.ref.pop_node[b0:b0 + live]] + 1
                vals[:, b0:b0 + live] = (np.float32(pair.ref.weight) * g.astype(np.float32))[None, :]
        sc.copy_(torch.from_numpy(vals.reshape(sc.shape)).to(DEV))
    return write


def mixed_scrambles(cs, P, seed):
    """depth 0 (solved root), 1 (solved at iteration 1), 2, 3 and deeper, cycling: problems end while others run."""
    return scrambles(cs, [(0, 1, 9, 2, 11, 3, 14)[i % 7] for i in range(P)] if P > 1 else [9], seed=seed)


# ------------------------------------------------------------------------------------- stage by stage
@pytest.mark.parametrize("B", [1, 4, 64])
@pytest.mark.parametrize("P", [1, 3, 40])
@pytest.mark.parametrize("cs", [2, 3])
def test_stages_match_restatement_with_written_scores(cs, P, B):
    """Every pool array, pop_node, live, active, length, solution, count, overflow, the beam and the bytes around them after init, every
    pop, every merge and backtrack; C large, and C in {1, 5, 32}: a full pool at init, overflow mid-list, exhaustion."""
    A = 12 if cs == 3 else 6
    for ci, C in enumerate((1 + B * (A - 1) * 6, 1, 5, 32)):
        pair = Pair(cs, mixed_scrambles(cs, P, seed=P + B), B, C, weight=(1.0, 0.6, 0.0, 2.5)[ci])
        write = hard_writer((4, 3, 0, 1)[ci], seed=ci)
        for _ in range(7):
            pair.iterate(write)
        pair.finish()
        if C <= 5 and P >= 3:                                               # the deep roots overflowed and then ran out of open nodes
            deep = np.flatnonzero(pair.ref.length < 0)
            assert len(deep) and pair.ref.overflow[deep].all() and (pair.ref.active[deep] == 0).all() and (pair.ref.ended[deep] > 0).all()


@pytest.mark.parametrize("mode", range(6))
def test_written_score_modes(mode):
    """Equal priorities across different g (mode 5: the node index alone decides), NaN, +-0, +-inf, lowest mantissa bits."""
    for cs, P, B, C in ((2, 3, 4, 400), (3, 40, 64, 700)):
        pair = Pair(cs, scrambles(cs, [9 + (i % 3) for i in range(P)], seed=2), B, C, weight=0.5)   # every root further than 3 moves
        for _ in range(4):
            pair.iterate(hard_writer(mode, seed=10 + mode))
        pair.finish()
        assert (pair.ref.count > B).all()                                   # the radix select had more open nodes than B to choose from


@pytest.mark.parametrize("cs", [2, 3])
def test_merge_priority_is_two_roundings(cs):
    """prio = score - weight * g with the product rounded before the difference.  Weight 0.7 (its product with 3 needs 26 bits) and
    scores a few ulps below -3: for many of the new nodes ONE rounding gives other bits -- counted here in float64, which holds the
    product of two float32 exactly -- so a multiply-subtract that k_astar_merge's compiler contracted into an fma shows."""
    from tests.pattern_ref import prio_rounded_once
    pair = Pair(cs, scrambles(cs, [9, 10, 11], seed=2), 16, 800, weight=0.7)    # B >= 12: the third iteration makes nodes at g = 3
    for _ in range(4):
        pair.iterate(hard_writer(2, seed=cs))
    ref = pair.ref
    made = (np.arange(ref.C)[None, :] < ref.count[:, None]).reshape(-1) & (ref.parent >= 0)      # every node but the roots
    once = prio_rounded_once(ref.score[made], 0.7, ref.g[made])
    assert (ref.g[made] >= 3).any() and (bits(once) != bits(ref.prio[made])).any()


@pytest.mark.parametrize("cs,B", [(2, 1), (2, 4), (3, 1), (3, 64)])
def test_exhaustion_with_every_child_known(cs, B):
    """A cube runs out of open nodes with room left in its pool: after iteration 1 the root is set back to open and its children to
    closed, on the device and in the restatement.  Iteration 2 pops the root again; every child's key is in the persistent table, so
    merge marks nothing new, appends nothing and leaves count and overflow as they are.  Iteration 3's pop finds no open node: the cube
    is exhausted with overflow still 0.  Every buffer is compared after every stage."""
    A = 12 if cs == 3 else 6
    P = 3
    pair = Pair(cs, scrambles(cs, [9, 10, 11], seed=2), B, 4 * A, weight=0.5)     # every root further than 3 moves: nothing is solved
    write = hard_writer(4, seed=cs + B)
    pair.iterate(write)
    assert (pair.ref.count == 1 + A).all() and (pair.ref.active == 1).all()
    state = pair.ref.state.reshape(P, -1)
    state[:, 0], state[:, 1:1 + A] = R.OPEN, R.CLOSED
    pair.plan.state.copy_(torch.from_numpy(pair.ref.state).to(DEV))
    pair.compare("reopened root")
    pair.iterate(write)                                                     # compares after pop and after merge, the NEW flags included
    assert (pair.ref.live == 1).all() and (pair.ref.count == 1 + A).all() and (pair.ref.overflow == 0).all()
    assert (pair.ref.state.reshape(P, -1)[:, :1 + A] == R.CLOSED).all() and (pair.ref.active == 1).all()
    assert (pair.plan.beam.flags.cpu().numpy() & R.NEW == 0).all()
    pair.iterate(write)                                                     # pop: exhausted; expand and merge find nothing active
    assert (pair.ref.active == 0).all() and (pair.ref.ended == 3).all() and (pair.ref.length == -1).all()
    assert (pair.ref.overflow == 0).all() and (pair.ref.live == 0).all() and (pair.ref.count == 1 + A).all()
    pair.finish()


@pytest.mark.parametrize("cs,front,dtype", [(3, "dense", torch.float32), (3, "dense", torch.bfloat16), (3, "codes", torch.float32),
                                            (2, "codes", torch.bfloat16), (2, "dense", torch.float32)])
def test_stages_with_a_random_deepcube(cs, front, dtype):
    model = DeepCube(_random_deepcube(cs)).to(DEV).to(dtype).eval()
    pair = Pair(cs, mixed_scrambles(cs, 40, seed=3), 4, 300, weight=0.25, model=model, front=front, dtype=dtype)
    with torch.no_grad():
        for _ in range(6):
            pair.iterate()
    pair.finish()


# ------------------------------------------------------------------------------------- mathematics
@pytest.mark.parametrize("cs,B,want,far", [(2, 1024, (7, 34, 154, 688, 2944), 6), (3, 128, (13, 127, 1195), 4)])
def test_level_flooding_counts_the_spheres(cs, B, want, far):
    """B >= the sphere size: iteration t pops exactly the nodes at depth t - 1, whatever the weight and the scores, so `nodes` is the
    cumulative sphere count of the cube group: the persistent dedup, exactly."""
    S = search_mod()
    cube = beam_ref.Cube(cs)
    dist, _ = beam_ref.bfs_distances(cube, far - 1)
    rng = np.random.default_rng(5)
    scr = []
    while len(scr) < 3:
        s = rng.integers(0, cube.A, (1, 14)).astype(np.uint8)
        if cube.scramble(s)[0].tobytes() not in dist:                       # at distance >= far: no child is solved while we count
            scr.append(s[0])
    scr = np.stack(scr)
    model = DeepCube(_random_deepcube(cs)).to(DEV).eval()
    plan = S.AStarPlan(len(scr), cs, B, want[-1] + 1, DEV, weight=0.3)
    env = env_of(cs, scr)
    plan.init(env.stickers, env.stickers.shape[-1])
    seen = [1]                                                              # sphere sizes: what the next pop takes
    with torch.no_grad():
        for t, total in enumerate(want):
            plan.step(model)
            count, g = plan.count.cpu().numpy(), plan.g.view(len(scr), -1).cpu().numpy()
            assert (count == total).all(), (t, count)
            assert (plan.beam.live.cpu().numpy() == seen[-1]).all()         # popped: the whole previous sphere
            assert (g[:, want[t - 1] if t else 1:total] == t + 1).all()     # appended: the next one
            seen.append(total - (want[t - 1] if t else 1))
    assert not plan.overflow.any() and bool(plan.beam.active.all())


RADIUS = 7


@pytest.fixture(scope="module")
def ball():
    cube = beam_ref.Cube(2)
    dist, counts = beam_ref.bfs_distances(cube, RADIUS)
    states = np.frombuffer(b"".join(dist), np.uint8).reshape(-1, cube.S)
    d = np.array(list(dist.values()))
    return cube, states, d


class BallValue(torch.nn.Module):
    """No parameters: value = -min(distance, RADIUS + 1) of the 2x2x2 state the dense one-hot names (row = piece, column =
    slot * 3 + orientation), by a sorted table of the ball's codes."""

    def __init__(self, cube, states, d):
        super().__init__()
        radix = 21 ** np.arange(7, dtype=np.int64)
        keys = cube.codes(states).astype(np.int64) @ radix
        order = np.argsort(keys)
        self.register_buffer("keys", torch.from_numpy(keys[order]))
        self.register_buffer("dist", torch.from_numpy(d[order].astype(np.float32)))
        self.register_buffer("radix", torch.from_numpy(radix))

    def forward(self, x):
        code = x.reshape(-1, 7, 7, 3).permute(0, 2, 1, 3).reshape(-1, 7, 21).argmax(-1)      # [m, slot] = piece * 3 + orientation
        k = (code * self.radix).sum(1)
        i = torch.searchsorted(self.keys, k).clamp_(max=len(self.keys) - 1)
        v = -torch.where(self.keys[i] == k, self.dist[i], torch.full_like(self.dist[i], RADIUS + 1.0))
        return v[:, None], v[:, None]


def test_exact_heuristic(ball):
    """2944 roots (every 2x2x2 state within RADIUS - 2) in one call.  B = 1, weight = 1: length == dist and iterations == dist.
    B = 4: length >= dist of the same parity.  Every solution replays on the oracle's moves to solved at exactly its length."""
    S = search_mod()
    cube, states, d = ball
    keep = d <= RADIUS - 2
    roots, d = states[keep], d[keep]
    assert len(roots) == 2944
    env = env_of(2, np.full((len(roots), 1), cube.A, np.uint8))
    env.set_sim_cube(torch.from_numpy(roots).to(DEV))
    before = env.stickers.clone()
    model = BallValue(cube, states, ball[2]).to(DEV)
    for B in (1, 4):
        res = S.astar_search(model, env, B, RADIUS, weight=1.0)
        length, act = res["length"].cpu().numpy(), res["actions"].cpu().numpy()
        assert torch.equal(env.stickers, before)
        assert res["solved"].all() and not res["overflow"].any()
        if B == 1:
            assert (length == d).all() and (res["iterations"].cpu().numpy() == d).all()
        else:
            assert (length >= d).all() and ((length - d) % 2 == 0).all()
        assert act.shape == (max(1, length.max()), len(roots))
        solved = R.replay(cube, roots, act)
        first = np.argmax(solved, axis=0)                                    # the first step at which the cube is solved
        assert (first == length).all() and solved[length, np.arange(len(roots))].all()
        assert ((act < cube.A) == (np.arange(act.shape[0])[:, None] < length[None, :])).all()


# ------------------------------------------------------------------------------------- equalities
def test_graph_eager_and_sync_every_agree_and_env_is_unchanged():
    S = search_mod()
    scr = scrambles(3, [k for k in range(0, 9) for _ in range(7)], seed=4)
    for dtype, front in ((torch.float32, "dense"), (torch.bfloat16, "codes")):
        model = DeepCube(_random_deepcube(3)).to(DEV).to(dtype).eval()
        env = env_of(3, scr)
        before = env.stickers.clone()
        runs = [S.astar_search(model, env, 8, 10, weight=0.5, front=front, dense_budget_bytes=1 << 20, **kw)
                for kw in (dict(sync_every=1), dict(sync_every=4), dict(graph=True), dict(graph=True, sync_every=1))]
        assert torch.equal(env.stickers, before)
        for k in ("solved", "length", "actions", "iterations", "nodes", "overflow"):   # iterations too: an early stop means every cube ended
            for r in runs[1:]:
                assert torch.equal(runs[0][k], r[k]), k
        assert runs[0]["capacity"] == 1 + 8 * 11 * 10 and bool(runs[0]["solved"][:14].all())
        cube = beam_ref.Cube(3)
        length, solved = runs[0]["length"].cpu().numpy(), R.replay(cube, cube.scramble(scr), runs[0]["actions"].cpu().numpy())
        for p in np.flatnonzero(length >= 0):
            assert solved[length[p], p] and not solved[:length[p], p].any()


def test_astar_solve_percentage():
    S = search_mod()
    rates = S.astar_solve_percentage(Stub(2).to(DEV), 2, 4, 10, 1024, 5, weight=0.0)
    assert rates == [100.0] * 4                                             # B >= every sphere within 4: level flooding, exhaustive


# ------------------------------------------------------------------------------------- ABI: errors, alignment
NAMES = {
    "rca_init": "roots n root_pitch cs C ppitch stickers keys parent action g score prio state count overflow live active length solution "
                "ended table table_bytes stream",
    "rca_pop": "n cs B C ppitch stickers action prio state count iteration beam pitch last_action live active ended pop_node stream",
    "rca_merge": "n cs B pitch C ppitch weight flags bkeys scores live active length solution ended iteration pop_node stickers keys parent "
                 "action g score prio state count overflow table table_bytes scratch scratch_bytes stream",
    "rca_backtrack": "n cs C parent action length solution actions max_length stream",
}
SCALARS = {"n", "root_pitch", "cs", "C", "ppitch", "B", "pitch", "weight", "table_bytes", "scratch_bytes", "max_length", "stream"}


def plan_values(plan, roots, actions):
    from rubiks_cube_solver_amd._lib import stream_ptr
    b = plan.beam
    t = dict(roots=roots, stickers=plan.stickers, keys=plan.keys, parent=plan.parent, action=plan.action, g=plan.g, score=plan.node_score,
             prio=plan.prio, state=plan.state, count=plan.count, overflow=plan.overflow, live=b.live, active=b.active, length=b.length,
             solution=plan.solution, ended=plan.ended, table=plan.table, iteration=plan.iteration, beam=b.beams[0],
             last_action=b.last_action, pop_node=plan.pop_node, flags=b.flags, bkeys=b.keys, scores=b.scores, scratch=b.workspace,
             actions=actions)
    v = {k: x.data_ptr() for k, x in t.items()}
    v.update(n=plan.P, root_pitch=roots.shape[-1], cs=plan.cs, C=plan.C, ppitch=plan.ppitch, B=plan.B, pitch=b.pitch, weight=plan.weight,
             table_bytes=plan.table.numel(), scratch_bytes=b.workspace.numel(), max_length=actions.shape[0], stream=stream_ptr(plan.dev))
    return v, t


def test_argument_errors_write_nothing():
    """Every violated limit, null pointer, pointer off 16-byte alignment or pitch that is not a power of two: -1 with a message, and
    not one byte of any buffer changes."""
    from rubiks_cube_solver_amd._astar_lib import astar_lib
    S = search_mod()
    L = astar_lib()
    env = env_of(3, scrambles(3, [3, 4, 5], seed=1))
    plan = S.AStarPlan(3, 3, 4, 50, DEV, weight=1.0)
    plan.init(env.stickers, env.stickers.shape[-1])
    plan.pop(), plan.expand()
    plan.beam.scores.normal_()
    actions = torch.zeros((4, 3), dtype=torch.uint8, device=DEV)
    values, tensors = plan_values(plan, env.stickers, actions)
    torch.cuda.synchronize()
    snap = {k: t.clone() for k, t in tensors.items()}
    bad_scalar = {"n": (0, -1, 1 << 31), "cs": (4, 0), "C": (0, -5, 1 << 31, ((1 << 31) + 2) // 3), "ppitch": (256, 768, 0, 1 << 27),
                  "B": (0, 65537, -1), "pitch": (256, 1536, 0, 1 << 27), "weight": (float("nan"), -1.0, float("inf")),
                  "table_bytes": (plan.table.numel() - 8, 0), "scratch_bytes": (plan.beam.workspace.numel() - 8, 0), "max_length": (0, -3),
                  "root_pitch": (0, 24, -512)}
    tried = 0
    for fn, names in NAMES.items():
        names = names.split()
        call = lambda v: getattr(L, fn)(*[v[k] for k in names])                # noqa: E731
        for k in names:
            if k == "stream":
                continue
            bads = bad_scalar[k] if k in SCALARS else (None, values[k] + 8, values[k] + 4)
            for bad in bads:
                assert call({**values, k: bad}) == -1, (fn, k, bad)
                assert L.rc_search_last_error() != b"", (fn, k, bad)
                tried += 1
    torch.cuda.synchronize()
    assert tried > 200
    for k, t in tensors.items():
        assert torch.equal(t.view(torch.uint8), snap[k].view(torch.uint8)), k
    # and the good calls still pass afterwards
    for fn in ("rca_merge", "rca_backtrack"):
        assert getattr(L, fn)(*[values[k] for k in NAMES[fn].split()]) == 0
    torch.cuda.synchronize()


def carve_like(t):
    """A copy of t whose data pointer is 16 bytes past a 32-byte boundary."""
    size = t.numel() * t.element_size()
    raw = torch.zeros(size + 96, dtype=torch.uint8, device=t.device)
    off = (16 - raw.data_ptr()) % 32
    view = raw[off:off + size].view(t.dtype).reshape(t.shape)
    assert view.data_ptr() % 32 == 16 and view.is_contiguous()
    view.copy_(t)
    return view


@pytest.mark.parametrize("cs", [2, 3])
def test_every_pointer_at_minimum_alignment(cs):
    S = search_mod()
    scr = mixed_scrambles(cs, 40, seed=8)
    model = Stub(cs).to(DEV)
    out = []
    for carved in (False, True):
        env = env_of(cs, scr)
        plan = S.AStarPlan(40, cs, 4, 60, DEV, weight=0.5)
        roots = env.stickers
        if carved:
            for obj, names in ((plan, "stickers keys parent action g node_score prio state count overflow ended solution pop_node iteration table"),
                               (plan.beam, "last_action live active length code flags keys scores workspace")):
                for name in names.split():
                    setattr(obj, name, carve_like(getattr(obj, name)))
            plan.beam.beams[0] = carve_like(plan.beam.beams[0])
            roots = carve_like(roots)
        plan.init(roots, roots.shape[-1])
        with torch.no_grad():
            for _ in range(5):
                plan.step(model)
        acts = plan.backtrack(5)
        if carved:
            plan.actions = None
            acts2 = carve_like(torch.zeros_like(acts))
            from rubiks_cube_solver_amd._astar_lib import astar_lib
            from rubiks_cube_solver_amd._lib import stream_ptr
            assert astar_lib().rca_backtrack(40, cs, 60, plan.parent.data_ptr(), plan.action.data_ptr(), plan.beam.length.data_ptr(),
                                             plan.solution.data_ptr(), acts2.data_ptr(), 5, stream_ptr(plan.dev)) == 0
            assert torch.equal(acts, acts2)
        torch.cuda.synchronize()
        out.append({k: getattr(plan, k).clone() for k in "stickers keys parent action g node_score prio state count overflow ended solution pop_node".split()}
                   | {"b_" + k: getattr(plan.beam, k).clone() for k in "last_action live active length flags keys scores".split()}
                   | {"beam": plan.beam.beams[0].clone(), "actions": acts.clone()})
    for k in out[0]:
        assert torch.equal(out[0][k].view(torch.uint8), out[1][k].view(torch.uint8)), k
    assert bool((out[0]["count"] > 1).any()) and bool((out[0]["b_length"] >= 0).any())


# ------------------------------------------------------------------------------------- checkpoint
def test_shipped_checkpoint_solves_what_greedy_solves():
    """The authors' 2x2x2 checkpoint, B = 16, weight = 1: every fixture scramble the greedy rollout solved (tests/golden/
    crosscheck_222.npz) is solved, and each solution replays on the HIP 2x2x2 path (a VecCubeEnv)."""
    S = search_mod()
    g = np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222.npz"))
    with np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222_weights.npz")) as z:
        sd = {k: z[k] for k in z.files}
    scr = g["scramble"].astype(np.uint8)
    greedy = g["done"].astype(bool).any(1)
    assert 200 < greedy.sum() < len(scr)
    res = S.astar_search(DeepCube(sd).to(DEV).eval(), env_of(2, scr), 16, 200, weight=1.0)
    solved, length, act = res["solved"].cpu().numpy(), res["length"].cpu().numpy(), res["actions"].cpu().numpy()
    assert solved[greedy].all(), np.flatnonzero(greedy & ~solved)
    env = env_of(2, np.concatenate([scr, act.T], 1))                        # scramble, then the returned moves, on the device
    assert env.done.cpu().numpy().astype(bool)[solved].all()
    assert ((act < 6) == (np.arange(act.shape[0])[:, None] < length[None, :])).all()
