"""The HIP kernels against the cube group itself (tests/group_ref.py), on complete, structured sets of states.  GPU only.

  a. rc_expand_children drives a breadth-first search: 2x2x2 complete (3 674 160 states), 3x3x3 to depth 7 (the last step expands
     878 880 parents into 10.5 M children): sphere sizes = OEIS A079762 / A080601, levels = the oracle's byte for byte, code counts.
  b. rc_search_expand on every complete sphere: equal keys <=> equal sticker vectors, VALID / SOLVED by their definitions.
  c. beam search under a PERFECT value function (the 2x2x2 distance table) from all 3 674 160 roots: length == distance.
  d. greedy rollout under a PERFECT policy from every non-solved state: solve_step == distance.
  e. orders of move words on every step route (VecCubeEnv.step in each obs mode, ops.apply_moves in every variant, the batch-1 facade).
  f. device random walks (reset, reset(seeds), ADI parents) against the distance table: dist <= k and dist = k (mod 2).
The oracle is used only in (a), where the levels are compared with it.  All comparisons are exact."""
import numpy as np
import pytest
import torch

from tests import group_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEP_VARIANTS = (0, 1, 2, 11, 12, 21, 22, 31, 32, 41, 42)          # the RC_VARIANT_STEP_* values tests/test_gpu_dispatch.py enumerates


@pytest.fixture(scope="module")
def ops():
    from rubiks_cube_solver_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from rubiks_cube_solver_amd import _lib
    return _lib


def dev_expand(ops, cs, variant=0):
    A = G.N_ACTIONS[cs]

    def expand(parents):
        n = len(parents)
        src = ops.from_aos(parents, DEV)
        out = ops.expand_buffers(n, cs, DEV, children=True, codes=True)
        ops.expand_children(src, n, cs, out["children"], out["child_solved"], out["child_code"], pitch=out["children"].shape[-1], variant=variant)
        ch = torch.stack([ops.to_aos(out["children"][a], n) for a in range(A)], 1).cpu().numpy()
        cc = torch.stack([ops.to_aos(out["child_code"][a], n) for a in range(A)], 1).cpu().numpy()
        return ch, cc, out["child_solved"][:, :n].t().contiguous().cpu().numpy()
    return expand


def dev_encode(ops, L, cs):
    def encode(states):
        n = len(states)
        st = ops.from_aos(states, DEV)
        code = ops.alloc_code(n, cs, DEV)
        done = torch.empty(n, dtype=torch.uint8, device=DEV)
        ops.encode(st, n, cs, code, L.FMT_CODE)
        ops.is_solved(st, n, cs, done)
        return ops.to_aos(code, n).cpu().numpy(), done.cpu().numpy()
    return encode


def dev_bfs(ops, L, cs, max_depth, variant=0):
    solved = np.repeat(np.arange(6, dtype=np.uint8), G.N_STICKERS[cs] // 6)
    return G.bfs(dev_expand(ops, cs, variant), dev_encode(ops, L, cs), solved, max_depth=max_depth)


def same_levels(got, want, spheres, codes, base):
    """Per level: the count is the constant, the sorted new states are the oracle's byte for byte, the child codes of every parent
    are the oracle's, the solved flags sit exactly on the children equal to the solved row; the distinct-code counts are `codes`."""
    assert tuple(len(lv.states) for lv in got) == tuple(spheres)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.states.shape == w.states.shape and (g.states == w.states).all(), g.depth
        assert (g.code == w.code).all() and (g.solved == w.solved).all() and int(g.solved.sum()) == (g.depth == 0), g.depth
        assert (g.parent == w.parent).all() and (g.move == w.move).all(), g.depth
        assert (g.child_code is None) == (w.child_code is None), g.depth
        if g.child_code is not None:
            assert (g.child_code == w.child_code).all(), g.depth
            assert ((g.child_solved != 0) == g.children_equal_solved).all() and (g.child_solved <= 1).all(), g.depth
    assert tuple(G.count_distinct(G.pack_code(lv.code, base)) for lv in got) == tuple(codes)


@pytest.fixture(scope="module")
def levels_222(ops, L):
    """The complete 2x2x2 search, every expansion by rc_expand_children at its default dispatch."""
    return dev_bfs(ops, L, 2, None)


@pytest.fixture(scope="module")
def oracle_222(oracle):
    return G.oracle_bfs(oracle, 2, None)


@pytest.fixture(scope="module")
def levels_333(ops, L):
    return dev_bfs(ops, L, 3, 7)


@pytest.fixture(scope="module")
def group(levels_222):
    """The 2x2x2 tables (keys, dist, nbr, states), built once per module from the DEVICE's search."""
    return G.build_222(levels_222)


class Tables:
    """The 2x2x2 tables on the device + the look-up the perfect models share."""

    def __init__(self, g):
        from rubiks_cube_solver_amd import codenet
        self.keys = torch.from_numpy(g.keys).to(DEV)
        self.dist = torch.from_numpy(g.dist.astype(np.int64)).to(DEV)
        self.nbr = torch.from_numpy(g.nbr.astype(np.int64)).to(DEV)
        self.radix = torch.from_numpy(G.RADIX_222).to(DEV)
        # dense [7, 21] one-hot -> radix key by ONE float64 product: the 1 of slot s holding code c sits at onehot_index[s, c], weight c * 21^s
        idx = codenet.onehot_index(2)
        w = np.zeros(147, np.float64)
        for s in range(7):
            w[idx[s]] = np.arange(21) * float(21 ** s)
        assert len(np.unique(idx)) == 147
        self.w = torch.from_numpy(w).to(DEV)

    def lookup_dense(self, x):
        """[m, 7, 21] -> (id [m] clamped, found [m])."""
        key = (x.reshape(x.shape[0], 147).double() @ self.w).round().long()
        i = torch.searchsorted(self.keys, key).clamp_(max=len(self.keys) - 1)
        return i, self.keys[i] == key

    def ids_of_code(self, code_aos):
        """[m, 7] uint8 device codes -> ids; every code must be one of the group's."""
        key = (code_aos.long() * self.radix).sum(1)
        i = torch.searchsorted(self.keys, key).clamp_(max=len(self.keys) - 1)
        assert bool((self.keys[i] == key).all()), "a code outside the group"
        return i


@pytest.fixture(scope="module")
def tables(group):
    return Tables(group)


class PerfectValue(torch.nn.Module):
    """No parameters: value = -distance of the state the one-hot names, -inf for a one-hot that names no state of the group (dead
    slots hold garbage)."""

    def __init__(self, t):
        super().__init__()
        self.t = t

    def forward(self, x):
        i, found = self.t.lookup_dense(x)
        v = torch.where(found, -self.t.dist[i].float(), torch.full((), float("-inf"), device=x.device))
        return v[:, None], v[:, None]


class PerfectPolicy(torch.nn.Module):
    """No parameters: policy logits = -distance of each neighbour."""

    def __init__(self, t):
        super().__init__()
        self.t = t

    def forward(self, x):
        i, _ = self.t.lookup_dense(x)
        return torch.zeros((x.shape[0], 1), device=x.device), -self.t.dist[self.t.nbr[i]].float()


def env_of(cs, states, obs=None, **kw):
    from rubiks_cube_solver_amd import VecCubeEnv
    env = VecCubeEnv(len(states), DEV, cs, obs=obs, **kw)
    env.set_sim_cube(states)
    return env


def replay_done_at(cs, states, actions, length):
    """Replay actions [T, n] (no-op padded) on an env loaded with `states`: done comes at exactly step length[i] and not before."""
    env = env_of(cs, states)
    for t in range(actions.shape[0]):
        _, _, done, _ = env.step(actions[t].contiguous())
        assert torch.equal(done != 0, length <= t + 1), t
    env.check_actions()


# ------------------------------------------------------------------------------------------------------------------ a. spheres
def test_222_spheres_default_dispatch(levels_222, oracle_222):
    same_levels(levels_222, oracle_222, G.SPHERES_222, G.SPHERES_222, 21)
    assert sum(len(lv.states) for lv in levels_222) == G.GROUP_222 and levels_222[-1].child_code is not None     # depth 15 is empty


@pytest.mark.parametrize("v", [1, 2])
def test_222_spheres_pack_variants(ops, L, oracle_222, v):
    same_levels(dev_bfs(ops, L, 2, None, variant=v), oracle_222, G.SPHERES_222, G.SPHERES_222, 21)


def test_333_spheres_to_depth_7(levels_333, oracle):
    same_levels(levels_333, G.oracle_bfs(oracle, 3, 7), G.SPHERES_333, G.CODES_333, 24)


def test_222_is_solved_encode_and_onehot_on_the_whole_group(ops, L, group, tables):
    from rubiks_cube_solver_amd import codenet
    n = G.GROUP_222
    st = ops.from_aos(group.states, DEV)
    done = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    rew = torch.zeros(n, dtype=torch.float32, device=DEV)
    ops.is_solved(st, n, 2, done, rew)
    assert int(done.sum()) == 1 and int(done.max()) == 1 and int(done.argmax()) == int(np.flatnonzero(group.dist == 0)[0])
    assert torch.equal(rew, done.float() * 2 - 1)
    code = ops.alloc_code(n, 2, DEV)
    ops.encode(st, n, 2, code, L.FMT_CODE)
    aos = ops.to_aos(code, n)
    assert torch.equal(tables.ids_of_code(aos), torch.arange(n, device=DEV))          # rc_encode's code = the expansion's, state by state
    want = torch.from_numpy(codenet.onehot_index(2)).to(DEV)[torch.arange(7, device=DEV)[None, :], aos.long()]      # [n, 7] flat positions
    assert bool((want.sort(1).values[:, 1:] > want.sort(1).values[:, :-1]).all())                                   # seven different positions
    for how in ("encode", "from_code"):
        oh = torch.full((n, 7, 21), 3.0, dtype=torch.float32, device=DEV)
        ops.encode(st, n, 2, oh, L.FMT_F32) if how == "encode" else ops.onehot_from_code(code, n, 2, oh)
        flat = oh.view(n, 147)
        assert bool((flat.gather(1, want) == 1).all()), how
        assert bool(((flat == 0) | (flat == 1)).all()) and bool((flat.sum(1) == 7).all()), how
    assert L.read_status() == 0


# ------------------------------------------------------------------------------------------------------------------ b. search keys
def pack_t(aos):
    """group_ref.pack on the device: [m, S] uint8 -> [m, words] int64, 3 bits per sticker, 21 per word."""
    m, S = aos.shape
    out = torch.zeros((m, -(-S // 21)), dtype=torch.int64, device=aos.device)
    for s in range(S):
        out[:, s // 21] |= aos[:, s].long() << (3 * (s % 21))
    return out


def distinct(rows):
    return int(torch.unique(rows, dim=0).shape[0]) if len(rows) else 0


def check_search_keys(ops, cs, levels):
    from rubiks_cube_solver_amd import _search_lib as SL, search      # SL.VALID / SOLVED / SURVIVOR: the RC_SEARCH_* bits of the header
    A = G.N_ACTIONS[cs]
    solved_w = pack_t(torch.from_numpy(levels[0].states).to(DEV))
    for lv in levels:
        n = len(lv.states)
        env = env_of(cs, lv.states)
        plan = search.BeamPlan(n, cs, 1, 1, DEV)
        plan.init(env.stickers, env.stickers.shape[-1])
        plan.flags.fill_(0xFF)
        plan.keys.fill_(-1)
        plan.expand(0)
        out = ops.expand_buffers(n, cs, DEV, children=True, codes=False)
        ops.expand_children(env.stickers, n, cs, out["children"], out["child_solved"], None, pitch=out["children"].shape[-1])
        packs = torch.stack([pack_t(ops.to_aos(out["children"][a], n)) for a in range(A)])       # [A, n, words], the test's own identity
        keys = plan.keys[:, :, :n].permute(1, 2, 0)                                                # [A, n, KW]
        flags = plan.flags[:, :n]
        # VALID: a live slot of an active problem and the move does not undo the last one: every child of a non-solved root, none of a solved one
        active = torch.from_numpy(lv.solved == 0).to(DEV)
        assert torch.equal((flags & SL.VALID) != 0, active[None, :].expand(A, n)), lv.depth
        assert torch.equal((flags & SL.SOLVED) != 0, (packs == solved_w[0]).all(-1)), lv.depth
        assert int((flags & (0xFF ^ SL.VALID ^ SL.SOLVED)).max()) == 0                   # expand sets nothing else
        if lv.depth == 0:
            continue
        k, p = keys.reshape(A * n, -1), packs.reshape(A * n, -1)
        nk, npk, both = distinct(k), distinct(p), distinct(torch.cat([k, p], 1))
        assert nk == npk == both, (lv.depth, nk, npk, both)                                       # one partition: equal keys <=> equal stickers
        assert npk < A * n                                                                        # and it is not the trivial one
        del plan, env, out, packs, keys
        torch.cuda.empty_cache()


def test_search_keys_partition_222(ops, levels_222):
    check_search_keys(ops, 2, levels_222)


def test_search_keys_partition_333(ops, levels_333):
    check_search_keys(ops, 3, levels_333[:7])                        # parents up to depth 6: 10.5 M candidates in the last step


# ------------------------------------------------------------------------------------------------------------------ c. perfect value
@pytest.fixture(scope="module")
def beam_width_1(group, tables):
    from rubiks_cube_solver_amd import search
    env = env_of(2, group.states)
    res = search.beam_search(PerfectValue(tables), env, width=1, max_depth=14, front="dense", dense_budget_bytes=4 << 30)
    assert torch.equal(env.sim_cube.cpu(), torch.from_numpy(group.states))                        # the env is left unchanged
    return {k: v.clone() for k, v in res.items()}


def test_beam_search_perfect_value_width_1(group, tables, beam_width_1):
    """Every state of the group as a root: under the exact distance the beam of width 1 walks a geodesic, so length == dist for every
    cube (0 for the solved root), nothing is left out, and the returned moves replay to solved at exactly that step."""
    res = beam_width_1
    assert res["length"].shape == (G.GROUP_222,) and bool(res["solved"].all())
    assert torch.equal(res["length"].long(), tables.dist)
    assert int((res["length"] == 0).sum()) == 1
    assert res["actions"].shape == (14, G.GROUP_222)
    replay_done_at(2, group.states, res["actions"], res["length"])


def test_beam_search_perfect_value_width_4(group, tables, beam_width_1):
    from rubiks_cube_solver_amd import search
    env = env_of(2, group.states)
    res = search.beam_search(PerfectValue(tables), env, width=4, max_depth=14, front="dense", dense_budget_bytes=4 << 30)
    assert bool(res["solved"].all()) and torch.equal(res["length"], beam_width_1["length"]) and torch.equal(res["length"].long(), tables.dist)
    replay_done_at(2, group.states, res["actions"], res["length"])


# ------------------------------------------------------------------------------------------------------------------ d. perfect policy
@pytest.mark.parametrize("mask,graph", [(False, False), (True, False), (False, True)])
def test_greedy_rollout_perfect_policy(group, tables, mask, graph):
    """Every non-solved state: the arg-max of -dist[neighbour] goes down one step at a time (and never undoes the last move, so the
    mask changes nothing): solve_step == dist, and the moves taken replay to solved at exactly that step."""
    from rubiks_cube_solver_amd.rollout import greedy_rollout
    keep = np.flatnonzero(group.dist > 0)
    assert len(keep) == G.GROUP_222 - 1
    states = group.states[keep]
    env = env_of(2, states, obs="onehot", onehot_dtype=torch.float32)
    res = greedy_rollout(PerfectPolicy(tables), env, max_timesteps=14, mask=mask, graph=graph)
    want = tables.dist[torch.from_numpy(keep).to(DEV)]
    assert bool(res["solved"].all()) and torch.equal(res["solve_step"].long(), want)
    assert res["actions"].shape[0] == 14
    replay_done_at(2, states, res["actions"], res["solve_step"])


# ------------------------------------------------------------------------------------------------------------------ e. word orders
def start_states(ops, cs, levels):
    ball = np.concatenate([lv.states for lv in levels[:5]])
    assert len(ball) == (11206 if cs == 3 else 688)
    n = 4096
    st = ops.alloc_states(n, cs, DEV)
    ops.fill_solved(st, n, cs)
    ops.scramble(st, n, cs, 30, seed=41, stream_id=cs)
    return np.concatenate([ball, ops.to_aos(st, n).cpu().numpy()])


def per_cube_equal(ops, a, b, n):
    """[tiles, rows, pitch] buffers -> bool [n]: cube i has the same rows in both."""
    return (a == b).all(dim=1).reshape(-1)[:n]


def colour_counts(st, n):
    return torch.stack([(st == c).sum(dim=1).reshape(-1)[:n] for c in range(6)])


@pytest.mark.parametrize("cs", [3, 2])
@pytest.mark.parametrize("obs", [None, "code", "onehot"])
def test_word_orders_vec_env_step(ops, L, levels_222, levels_333, cs, obs):
    """Each word through VecCubeEnv.step: every cube is back at its start first after exactly `order` applications; the observation
    the step returns then equals the start's (encoded on its own by rc_encode); colour counts never change."""
    start = start_states(ops, cs, levels_333 if cs == 3 else levels_222)
    n, A = len(start), G.N_ACTIONS[cs]
    env = env_of(cs, start, obs=obs, **({"onehot_dtype": torch.float32} if obs == "onehot" else {}))
    first = env.stickers.clone()
    counts = colour_counts(first, n)
    obs0 = None
    if obs == "code":
        obs0 = ops.alloc_code(n, cs, DEV)
        ops.encode(first, n, cs, obs0, L.FMT_CODE)
    elif obs == "onehot":
        obs0 = torch.empty((n, *env.state_dim), dtype=torch.float32, device=DEV)
        ops.encode(first, n, cs, obs0, L.FMT_F32)
    act = lambda a: torch.full((n,), a, dtype=torch.uint8, device=DEV)
    for word, acts, order in G.words_for(cs):
        for k in range(1, order + 1):
            for a in acts:
                o, rew, done, _ = env.step(act(a))
            same = per_cube_equal(ops, env.stickers, first, n)
            assert bool(same.all()) if k == order else not bool(same.any()), (word, k)
            assert torch.equal(colour_counts(env.stickers, n), counts), (word, k)
        if obs == "code":
            assert bool(per_cube_equal(ops, o, obs0, n).all()), word
        elif obs == "onehot":
            assert torch.equal(o, obs0), word
    # commuting faces (3x3x3), a then a ^ 1, on the same batch
    def moved(*names):
        env.set_sim_cube(start)
        for m in names:
            env.step(act(G.ACTION_NAMES[cs].index(m)))
        return env.stickers.clone()
    if cs == 3:
        for x, y in G.COMMUTING_333:
            assert torch.equal(moved(x, y), moved(y, x)) and torch.equal(moved(x, y + "'"), moved(y + "'", x)), (x, y)
    assert not bool(per_cube_equal(ops, moved("U", "R"), moved("R", "U"), n).any())
    for a in range(A):
        env.set_sim_cube(start)
        env.step(act(a))
        assert not bool(per_cube_equal(ops, env.stickers, first, n).any()), a
        env.step(act(a ^ 1))
        assert torch.equal(env.stickers, first), a
    env.check_actions()


@pytest.mark.parametrize("cs", [3, 2])
def test_word_orders_apply_moves_every_variant(ops, L, levels_222, levels_333, cs):
    """The same through ops.apply_moves out of place (ping-pong) in every RC_VARIANT_STEP_* the dispatch tests enumerate, with the
    fused compact code: back at the start first at exactly `order`, and the code written by that step is the start's."""
    start = start_states(ops, cs, levels_333 if cs == 3 else levels_222)
    n = len(start)
    first = ops.from_aos(start, DEV)
    code0 = ops.alloc_code(n, cs, DEV)
    ops.encode(first, n, cs, code0, L.FMT_CODE)
    act = {a: torch.full((n,), a, dtype=torch.uint8, device=DEV) for a in range(G.N_ACTIONS[cs])}
    done = torch.empty(n, dtype=torch.uint8, device=DEV)
    counts = colour_counts(first, n)
    for variant in STEP_VARIANTS:
        for word, acts, order in G.words_for(cs):
            a_buf, b_buf = first.clone(), torch.zeros_like(first)
            code = torch.zeros_like(code0)
            for k in range(1, order + 1):
                for a in acts:
                    ops.apply_moves(a_buf, b_buf, act[a], n, cs, None, done, code, L.FMT_CODE, variant=variant)
                    a_buf, b_buf = b_buf, a_buf
                same = per_cube_equal(ops, a_buf, first, n)
                assert bool(same.all()) if k == order else not bool(same.any()), (variant, word, k)
                assert torch.equal(colour_counts(a_buf, n), counts), (variant, word, k)
            assert bool(per_cube_equal(ops, code, code0, n).all()), (variant, word)
    assert L.read_status() == 0


@pytest.mark.parametrize("cs", [3, 2])
def test_word_orders_batch_1_facade(cs):
    """From solved through the batch-1 CubeEnv: one rc_facade_step per move, and one rc_facade_steps launch per word: done comes first
    after exactly `order` applications, and the one-hot returned then is the solved cube's."""
    from rubiks_cube_solver_amd import CubeEnv
    env = CubeEnv(device=torch.device("cpu"), cube_size=cs)
    for word, acts, order in G.words_for(cs):
        for route in ("step", "step_many"):
            env.init_state()
            home = np.array(env.cube)
            for k in range(1, order + 1):
                if route == "step":
                    for a in acts:
                        state, reward, done, _ = env.step(a)
                else:
                    state, reward, done, _ = env.step_many(acts)
                assert done == (k == order) and reward == (1.0 if k == order else -1.0), (word, route, k)
                assert (np.asarray(state) == home).all() == (k == order), (word, route, k)
            assert (env.sim_cube == np.repeat(np.arange(6), G.N_STICKERS[cs] // 6)).all(), (word, route)
    env.close()


# ------------------------------------------------------------------------------------------------------------------ f. walks
def check_walk(tables, code_aos, k):
    d = tables.dist[tables.ids_of_code(code_aos)]
    assert int(d.max()) <= k and bool(((d - k) % 2 == 0).all()), k
    return d


def test_222_device_walks_against_distances(ops, L, tables):
    """k random quarter turns from solved end at distance <= k of k's parity: VecCubeEnv.reset with the device RNG and with per-env
    legacy seeds, k = 1..20 over 2^20 cubes."""
    from rubiks_cube_solver_amd import VecCubeEnv
    n = 1 << 20
    env = VecCubeEnv(n, DEV, 2, obs="code", seed=5, stream_id=1)
    seeds = torch.arange(n, dtype=torch.int64) * 2654435761 % (1 << 32)
    seen = 0
    for k in range(1, 21):
        d = check_walk(tables, ops.to_aos(env.reset(scramble_count=k), n), k)
        seen = max(seen, int(d.max()))
        check_walk(tables, ops.to_aos(env.reset(seeds=(seeds + k) % (1 << 32), scramble_count=k), n), k)
    assert seen >= 11                                  # the walks do leave the neighbourhood of solved (276 of 3.7 M states are at 14)
    assert L.read_status() == 0


def test_222_adi_parents_against_distances(ops, L, tables):
    W, D = 100_000, 14
    pt, bufs = ops.adi_buffers(W, D, 2, DEV, parents=True, parent_code=True, child_code=True)
    ops.adi_generate(W, D, 2, pt, DEV, seed=19, stream_id=3, **bufs)
    for d in range(D):
        check_walk(tables, ops.to_aos(bufs["parent_code"][d], W), d + 1)
    assert L.read_status() == 0


@pytest.mark.parametrize("cs", [3, 2])
@pytest.mark.parametrize("triple", G.RNG_TRIPLES)
def test_adi_action_streams_equal_python_restatement(ops, L, cs, triple):
    """The kernel's action draws for three (seed, stream, walk_offset) triples, also beyond 2^32 and 2^63, against DESIGN.md section 5
    restated on Python big ints (tests/group_ref.py) -- not against the C oracle."""
    seed, stream, walk0 = triple
    W, D, A = 5, 30, G.N_ACTIONS[cs]
    pt, bufs = ops.adi_buffers(W, D, cs, DEV, parents=True, children=True)
    ops.adi_generate(W, D, cs, pt, DEV, seed=seed, stream_id=stream, walk_offset=walk0, **bufs)
    got = bufs["actions_out"][:, :W].cpu().numpy()
    for w in range(W):
        assert (got[:, w] == G.rng_actions(seed, stream, walk0 + w, D, A)).all(), w
    assert L.read_status() == 0
