"""The corner pattern database on the GPU (pattern.CornerTable, the rcp_* entry points of librubiksearch.so, front="table" of search.py):
the built tables against the committed level counts and the numpy restatement (tests/pattern_ref.py), rank / unrank through the cubie
kernels, the table proved to be the distance through the existing move kernels, look-ups and scores in every layout, whole
searches whose lengths must be the exact distances, and the table against the symmetry kernel (an image is as far from solved as
its state).  All comparisons are exact.  GPU only."""
import ctypes

import numpy as np
import pytest
import torch

from tests import astar_ref, beam_ref, group_ref
from tests import layout_cases as LC
from tests import pattern_ref as R
from tests.test_gpu_cubies import FILL, Arena, rows_arena
from tests.test_gpu_search import DeepCube, _random_deepcube, env_of, scrambles

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
CHUNK = 1 << 20
COUNTS = (1, 3, 513, 2565)


def mods():
    from rubiks_cube_solver_amd import _lib, _pattern_lib, ops, pattern, search
    return _lib, _pattern_lib, ops, pattern, search


def stream():
    from rubiks_cube_solver_amd import _lib
    return _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def dense_run(cs):
    """One dense-front A* and one beam search with a random DeepCube: the results as bytes."""
    _, _, _, _, S = mods()
    torch.manual_seed(0)
    model = DeepCube(_random_deepcube(cs)).to(DEV).eval()
    env = env_of(cs, scrambles(cs, [1 + i % 6 for i in range(40)], seed=5))
    a = S.astar_search(model, env, 4, 12, weight=0.5, front="dense")
    b = S.beam_search(model, env, 8, 6, front="dense")
    torch.cuda.synchronize()
    return [a[k].cpu().numpy().tobytes() for k in ("length", "actions", "iterations", "nodes")] + [b[k].cpu().numpy().tobytes() for k in ("length", "actions")]


@pytest.fixture(scope="session")
def dense_before():
    """The net fronts' results BEFORE any table object exists in the process (the `tables` fixture depends on this one)."""
    return {cs: dense_run(cs) for cs in (2, 3)}


@pytest.fixture(scope="session")
def tables(dense_before):
    _, _, _, pattern, _ = mods()
    return {cs: pattern.CornerTable.build(cs, DEV) for cs in (2, 3)}


@pytest.fixture(scope="session")
def host_tables(tables):
    return {cs: tables[cs].table.cpu().numpy() for cs in (2, 3)}


@pytest.fixture(scope="session")
def ref222():
    """The restatement's distances of the whole 2x2x2 group: the sticker search, once."""
    return R.bfs(2)


def covered(cs):
    """The indices the exhaustive tests walk: every 2x2x2 index; on the 3x3x3 i = 5 (mod 16) plus 0 and the last."""
    n = R.SIZE[cs]
    return np.arange(n, dtype=np.int64) if cs == 2 else np.concatenate([[0], np.arange(5, n, 16, dtype=np.int64), [n - 1]])


# ---------------------------------------------------------------------------------------------------------------- 1. build
def test_build_levels_and_the_restatement(tables, host_tables, ref222):
    _, _, _, pattern, _ = mods()
    for cs in (2, 3):
        t, h = tables[cs], host_tables[cs]
        assert t.levels == R.LEVELS[cs] and t.depth == 14
        assert h.dtype == np.uint8 and len(h) == R.SIZE[cs] and h[0] == 0 and not (h == 0xFF).any()
        assert tuple(np.bincount(h)) == R.LEVELS[cs]
        again = pattern.CornerTable.build(cs, DEV)                           # building twice gives identical bytes
        assert again.levels == t.levels and torch.equal(again.table, t.table)
    dist, levels = ref222
    assert levels == group_ref.SPHERES_222 and (host_tables[2] == dist).all()
    wrapped = pattern.CornerTable(tables[2].table.clone(), 2)                # a table loaded from disk
    assert wrapped.levels is None and torch.equal(wrapped.distance(tables[2].states([0, 1, 3674159]), 3), tables[2].table[[0, 1, 3674159]])
    broken = tables[2].table.clone()
    broken[0] = 1
    with pytest.raises(ValueError):
        pattern.CornerTable(broken, 2)


def _level_builders():
    """(name, N, begin(table), level(table, depth, count)) of the users of the one level kernel: the 2x2x2 corner space, the edge
    spaces of mask 0x3 (528 entries; its home index is 0) and of mask 0x6 (528 entries, home index 48: the goal is not entry 0) and
    chain stage 3 (the LDS prologue, entries no cube has)."""
    from rubiks_cube_solver_amd import _chain_lib, _edge_lib, _search_lib
    _lib, P, _, _, _ = mods()
    ptr, st = _lib.ptr, stream()
    Lp, Le, Lc = P.pattern_lib(), _edge_lib.edge_lib(), _chain_lib.chain_lib()
    assert _edge_lib.home_index(0x6) != 0

    def edge(mask):
        return (f"edge mask {mask:#x}", _edge_lib.table_bytes(mask), lambda t: _lib.check(Le.rce_build_begin(ptr(t), t.numel(), mask, st)),
                lambda t, d, c: _lib.check(Le.rce_build_level(ptr(t), t.numel(), mask, d, ptr(c), st)))
    return (("corner 2x2x2", P.table_bytes(2), lambda t: _search_lib.check(Lp.rcp_build_begin(ptr(t), t.numel(), 2, st)),
             lambda t, d, c: _search_lib.check(Lp.rcp_build_level(ptr(t), t.numel(), 2, d, ptr(c), st))),
            edge(0x3), edge(0x6),
            ("chain stage 3", _chain_lib.table_bytes(3), lambda t: _lib.check(Lc.rct_build_begin(ptr(t), t.numel(), 3, st)),
             lambda t, d, c: _lib.check(Lc.rct_build_level(ptr(t), t.numel(), 3, d, ptr(c), st))))


def test_every_level_of_the_shared_level_kernel():
    """One level kernel, three index spaces: after EVERY level of each build the returned count is the number of entries that hold
    depth + 1, nothing but 0xFF lies above depth + 1, and what earlier levels set is unchanged."""
    _lib, _, _, pattern, _ = mods()
    _lib.init(torch.device(DEV, torch.cuda.current_device()))
    for name, n, begin, level in _level_builders():
        assert n in (3674160, 528, 1327104)
        table = torch.empty(n, dtype=torch.uint8, device=DEV)
        count = torch.zeros(4, dtype=torch.int32, device=DEV)
        begin(table)
        assert int((table == 0).sum()) >= 1 and bool(((table == 0) | (table == 0xFF)).all()), name
        for depth in range(pattern.MAX_LEVELS + 1):
            before = table.clone()
            level(table, depth, count)
            c, was_set = int(count[0]), before != 0xFF
            assert c == int((table == depth + 1).sum()), (name, depth)
            assert not bool(((table > depth + 1) & (table != 0xFF)).any()), (name, depth)
            assert torch.equal(table[was_set], before[was_set]), (name, depth)
            if c == 0:
                break
        else:
            raise AssertionError(f"{name}: no empty level within {pattern.MAX_LEVELS + 1}")
        assert depth >= 1, name


# --------------------------------------------------------------------------------------------------------- 2. rank / unrank
@pytest.mark.parametrize("cs", (2, 3))
def test_unrank_then_rank_is_the_identity(tables, cs):
    _, _, ops, _, _ = mods()
    idx = covered(cs)
    for at in range(0, len(idx), CHUNK):
        part = idx[at:at + CHUNK]
        st = tables[cs].states(torch.from_numpy(part))
        out = ops.cubies(st, len(part), cs, cubies=False, index=True)
        assert not bool(out["status"].any())
        assert torch.equal(out["corner_index"].cpu().long() & 0xFFFFFFFF, torch.from_numpy(part))


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("cs", (2, 3))
def test_unrank_in_every_layout_carved_with_bad_indices(tables, cs, n):
    """rcp_unrank with every operand 16 bytes past a 32-byte boundary, in each of the four layouts: the rows equal the restatement's,
    an index >= N is written solved and flagged, guards and pad columns keep their bytes."""
    _, P, _, _, _ = mods()
    L, SL, N = P.pattern_lib(), LC.SL_OF[cs], R.SIZE[cs]
    rng = np.random.default_rng(n + cs)
    idx = rng.integers(0, N, n).astype(np.uint32)
    idx[0] = N - 1
    for flagged in (False, True):
        if flagged:
            idx[n - 1] = N                                                   # the first index outside, in the ragged last pack
            if n > 600:
                idx[[7, 600]] = 0xFFFFFFFF, N + 12345
        want, bad = R.unrank(cs, idx.astype(np.int64))
        assert bad.any() == flagged
        for lay in LC.LAYOUTS:
            offs = LC.carve_offsets(3)
            ind = Arena(4 * n, offs[0])
            ind.expect(idx)
            ind.upload()
            cub = rows_arena(None, n, SL, lay, offs[1]).upload()
            flag = Arena(16, offs[2])
            flag.host[flag.start] = 0
            flag.upload()
            assert L.rcp_unrank(ind.ptr(), n, cs, cub.ptr(), cub.pitch, flag.ptr(), stream()) == 0, L.rc_search_last_error()
            cub.expect_rows(want, cub.pitch)
            flag.host[flag.start] = int(flagged)
            for a, what in ((ind, "index"), (cub, "cubies"), (flag, "bad")):
                a.check(f"rcp_unrank cs={cs} n={n} {lay} flagged={flagged}: {what}")
    with pytest.raises(IndexError):
        tables[cs].cubies([0, N])


# --------------------------------------------------------------------------- 3. the table is the distance (the device's own moves)
@pytest.mark.parametrize("cs", (2, 3))
def test_table_is_the_distance_through_the_move_kernels(tables, cs):
    """For every covered index: states(i) -> rc_expand_children -> rcp_lookup on parent and children.  |h(child) - h(parent)| = 1 (a
    quarter turn flips the corner parity), h > 0 => some child has h - 1, h == 0 <=> the corners are home.  A byte array with these
    properties and h(solved) = 0 IS the distance."""
    _, _, ops, _, _ = mods()
    t, A, idx = tables[cs], LC.A_OF[cs], covered(cs)
    for at in range(0, len(idx), CHUNK):
        part = torch.from_numpy(idx[at:at + CHUNK])
        n = len(part)
        st = t.states(part)
        h = t.distance(st, n).int()
        assert torch.equal(h, t.table[part.to(DEV)].int())
        out = ops.expand_buffers(n, cs, DEV, st.shape[-1], children=True, codes=False)
        ops.expand_children(st, n, cs, out["children"], out["child_solved"], None, pitch=st.shape[-1])
        down = torch.zeros(n, dtype=torch.bool, device=DEV)
        for a in range(A):
            hc = t.distance(out["children"][a], n).int()
            assert bool(((hc - h).abs() == 1).all()), a
            down |= hc == h - 1
        assert bool((down == (h > 0)).all())
        home = part.to(DEV) == 0                                             # corner_index 0 <=> every corner home and untwisted
        assert bool(((h == 0) == home).all())


# --------------------------------------------------------------------------------------------------------------- 4. look-up
def illegal_cubes(cs, st):
    """st [n >= 8, S] legal -> a copy whose cubes 0..: a twisted corner, a repeated corner piece, a corner sticker above 5 (6, 7, 0xFF)."""
    from rubiks_cube_solver_amd.tables import get_cubies
    cb = get_cubies(cs)
    bad = st.copy()
    bad[0, cb.corner_cw[0]] = bad[0, np.roll(cb.corner_cw[0], 1)]
    bad[1, cb.corner_cw[2]] = bad[1, cb.corner_cw[5]]
    bad[2, cb.corner_cw[1][1]], bad[3, cb.corner_cw[3][2]], bad[4, cb.corner_cw[6][0]] = 6, 7, 0xFF
    return bad, 5


@pytest.mark.parametrize("cs", (2, 3))
def test_lookup_on_device_walks(tables, host_tables, cs):
    """2^18 + 5 walks of k = 0..20 moves made by the env: h <= k, h = k (mod 2), h = table[numpy corner index]."""
    _, _, ops, _, _ = mods()
    n = (1 << 18) + 5
    k = np.arange(n) % 21
    env = env_of(cs, scrambles(cs, list(k), seed=11))
    h = env.corner_distance(tables[cs]).cpu().numpy().astype(np.int64)
    assert (h <= k).all() and ((h - k) % 2 == 0).all() and (h[k == 0] == 0).all()
    st = ops.to_aos(env.stickers, n).cpu().numpy()
    ci = R.corner_index(cs, st)
    assert (ci < R.SIZE[cs]).all() and (h == host_tables[cs][ci]).all()


@pytest.mark.parametrize("n", (513, 2565))
@pytest.mark.parametrize("cs", (2, 3))
def test_lookup_in_every_layout_pair(tables, host_tables, oracle, cs, n):
    """unrank into layout X, rcc_from_cubies X -> Y, rcp_lookup from Y: every ordered pair, operands carved, some cubes made illegal
    (0xFF, nothing read) and, on the 3x3x3, an edge flipped or miscoloured (the corner distance all the same)."""
    _lib, P, _, _, _ = mods()
    from rubiks_cube_solver_amd import _cubie_lib
    from rubiks_cube_solver_amd.tables import get_cubies
    L, LH, S, SL, N = P.pattern_lib(), _cubie_lib.cubie_lib(), LC.S_OF[cs], LC.SL_OF[cs], R.SIZE[cs]
    t = tables[cs]
    idx = np.random.default_rng(n * cs).integers(0, N, n).astype(np.uint32)
    cub_rows, _ = R.unrank(cs, idx.astype(np.int64))
    legal = get_cubies(cs).from_cubies(cub_rows)[0]
    states, n_bad = illegal_cubes(cs, legal)
    if cs == 3:
        cb = get_cubies(3)
        states[10, cb.edge_facelets[3]] = states[10, cb.edge_facelets[3][::-1]]     # only a flipped edge
        states[11, cb.edge_facelets[0][0]] = 6                                      # an edge sticker that is no colour
        states[12, 4] = 2                                                           # a wrong centre
    want = host_tables[cs][idx].copy()
    want[:n_bad] = 0xFF
    assert (R.corner_index(cs, states)[:n_bad] == 0xFFFFFFFF).all() and (R.corner_index(cs, states)[n_bad:] == idx[n_bad:]).all()
    for lay_c, lay_st in LC.PAIRS:
        offs = LC.carve_offsets(5)
        ind = Arena(4 * n, offs[0])
        ind.expect(idx)
        ind.upload()
        cub = rows_arena(None, n, SL, lay_c, offs[1]).upload()
        st = rows_arena(None, n, S, lay_st, offs[2]).upload()
        flag = Arena(16, offs[3])
        flag.host[flag.start] = 0
        flag.upload()
        dist = Arena(n, offs[4]).upload()
        assert L.rcp_unrank(ind.ptr(), n, cs, cub.ptr(), cub.pitch, flag.ptr(), stream()) == 0
        assert LH.rcc_from_cubies(cub.ptr(), n, cub.pitch, cs, st.ptr(), st.pitch, flag.ptr(), stream()) == 0
        assert L.rcp_lookup(st.ptr(), n, st.pitch, cs, ctypes.c_void_p(t.table.data_ptr()), N, dist.ptr(), stream()) == 0
        cub.expect_rows(cub_rows, cub.pitch)
        st.expect_rows(legal, st.pitch)
        dist.expect(host_tables[cs][idx])
        for a, what in ((ind, "index"), (cub, "cubies"), (st, "st"), (flag, "bad"), (dist, "dist")):
            a.check(f"cs={cs} n={n} {lay_c}->{lay_st}: {what}")
        # the same layout with the doctored cubes
        st2 = rows_arena(states, n, S, lay_st, offs[2]).upload()
        dist2 = Arena(n, offs[4]).upload()
        assert L.rcp_lookup(st2.ptr(), n, st2.pitch, cs, ctypes.c_void_p(t.table.data_ptr()), N, dist2.ptr(), stream()) == 0
        dist2.expect(want)
        st2.check("doctored st")
        dist2.check(f"cs={cs} n={n} {lay_st}: doctored dist")


@pytest.mark.parametrize("cs", (2, 3))
def test_lookup_argument_errors_write_nothing(tables, cs):
    _, P, _, _, _ = mods()
    L, S, N, n = P.pattern_lib(), LC.S_OF[cs], R.SIZE[cs], 513
    st = rows_arena(None, n, S, "tight", 0).upload()
    dist = Arena(n + 16, 0).upload()
    tb = tables[cs].table
    before = tb.clone()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    good = dict(st=st.ptr(), n=n, pitch=st.pitch, cs=cs, table=p(tb), bytes=N, dist=dist.ptr())
    call = lambda **kw: (lambda a: L.rcp_lookup(a["st"], a["n"], a["pitch"], a["cs"], a["table"], a["bytes"], a["dist"], stream()))({**good, **kw})
    for word, kw in [("st", dict(st=None)), ("st", dict(st=p(st.view, 8))), ("n_cubes", dict(n=-1)), ("pitch", dict(pitch=st.pitch - 8)),
                     ("pitch", dict(pitch=256)), ("cube_size", dict(cs=4)), ("table", dict(table=None)), ("table", dict(table=p(tb, 4))),
                     ("bytes", dict(bytes=N - 1)), ("bytes", dict(bytes=0)), ("dist", dict(dist=None)), ("dist", dict(dist=p(dist.view, 4)))]:
        assert call(**kw) == EINVAL, (word, kw)
        assert word in L.rc_search_last_error().decode(), (word, L.rc_search_last_error())
    assert call(n=0) == 0
    # the build's and unrank's refusals
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    flag = torch.zeros(16, dtype=torch.uint8, device=DEV)
    ind = torch.zeros(16, dtype=torch.int32, device=DEV)
    cub = torch.full((LC.SL_OF[cs], 16), FILL, dtype=torch.uint8, device=DEV)
    for rc in (L.rcp_build_begin(None, N, cs, stream()), L.rcp_build_begin(p(tb, 8), N, cs, stream()), L.rcp_build_begin(p(tb), N - 1, cs, stream()),
               L.rcp_build_begin(p(tb), N, 5, stream()), L.rcp_build_level(p(tb), N - 1, cs, 0, p(cnt), stream()),
               L.rcp_build_level(p(tb), N, cs, -1, p(cnt), stream()), L.rcp_build_level(p(tb), N, cs, 254, p(cnt), stream()),
               L.rcp_build_level(p(tb), N, cs, 0, None, stream()), L.rcp_build_level(p(tb), N, cs, 0, p(cnt, 4), stream()),
               L.rcp_build_level(None, N, cs, 0, p(cnt), stream()), L.rcp_build_level(p(tb), N, 1, 0, p(cnt), stream()),
               L.rcp_unrank(None, 3, cs, p(cub), 16, p(flag), stream()), L.rcp_unrank(p(ind, 4), 3, cs, p(cub), 16, p(flag), stream()),
               L.rcp_unrank(p(ind), 3, cs, None, 16, p(flag), stream()), L.rcp_unrank(p(ind), 3, cs, p(cub, 8), 16, p(flag), stream()),
               L.rcp_unrank(p(ind), 3, cs, p(cub), 8, p(flag), stream()), L.rcp_unrank(p(ind), 17, cs, p(cub), 16, p(flag), stream()),
               L.rcp_unrank(p(ind), 3, cs, p(cub), 16, None, stream()), L.rcp_unrank(p(ind), -1, cs, p(cub), 16, p(flag), stream()),
               L.rcp_unrank(p(ind), 3, 0, p(cub), 16, p(flag), stream())):
        assert rc == EINVAL
    assert L.rcp_unrank(p(ind), 0, cs, p(cub), 16, p(flag), stream()) == 0
    torch.cuda.synchronize()
    st.check("st")
    dist.check("dist after the refused calls")
    assert torch.equal(tb, before) and not bool(flag.any()) and not bool(cnt.any()) and bool((cub == FILL).all())


# ---------------------------------------------------------------------------------------------------------------- 5. scores
def all_scores(cs, keys, host_table):
    """The restatement over every slot of a key array [KW, A, NBp]."""
    kw, A, nbp = keys.shape
    return R.score_of_keys(cs, keys.reshape(kw, A * nbp), host_table).reshape(A, nbp)


@pytest.mark.parametrize("W", (1, 4, 64))
@pytest.mark.parametrize("P", (1, 3, 40))
@pytest.mark.parametrize("cs", (2, 3))
def test_scores_of_every_candidate_slot(tables, host_tables, cs, P, W):
    """rc_search_init + rc_search_expand, then BeamPlan.score: every slot's score equals the restatement on the unpacked key -- the
    live candidates, the dead slots expand wrote, and (a second call on a key array of random 64-bit words) arbitrary bits."""
    _, _, _, _, S = mods()
    t = tables[cs]
    plan = S.BeamPlan(P, cs, W, 1, DEV, front="table")
    assert not hasattr(plan, "dense") and not hasattr(plan, "hidden")
    env = env_of(cs, scrambles(cs, [1 + i % 9 for i in range(P)], seed=P + W))
    rnd = torch.from_numpy(np.random.default_rng(P * W + cs).integers(-1 << 63, (1 << 63) - 1, plan.keys.numel(), dtype=np.int64)).view(plan.keys.shape)
    plan.keys.copy_(rnd)                                                     # slots past `live` hold arbitrary 64-bit words beforehand
    plan.scores.fill_(float("nan"))
    plan.init(env.stickers, env.stickers.shape[-1])
    plan.expand(0)
    plan.score(t)
    torch.cuda.synchronize()
    keys = plan.keys.cpu().numpy().view(np.uint64)
    got = plan.scores.cpu().numpy()
    want = all_scores(cs, keys, host_tables[cs])
    assert got.dtype == np.float32 and (got == want).all()
    live = plan.flags.cpu().numpy()[:, :P * W:W] & 1                        # slot 0 of every problem: the root's children
    roots = env.corner_distance(t).cpu().numpy().astype(np.float32)
    assert (np.abs(-got[:, :P * W:W] - roots[None, :]) == 1).all() and live.any()
    assert ((got == -255) | ((got <= 0) & (got >= -14))).all()
    # arbitrary bits in every slot
    plan.keys.copy_(rnd)
    plan.scores.fill_(float("nan"))
    t.score_keys(plan.keys, P, W, plan.pitch, plan.scores)
    got = plan.scores.cpu().numpy()
    assert (got == all_scores(cs, plan.keys.cpu().numpy().view(np.uint64), host_tables[cs])).all()
    assert ((got == -255) | ((got <= 0) & (got >= -14))).all() and (got == -255).mean() > 0.99


@pytest.mark.parametrize("cs", (2, 3))
def test_score_argument_errors_write_nothing(tables, cs):
    _, P, _, _, S = mods()
    L, N = P.pattern_lib(), R.SIZE[cs]
    plan = S.BeamPlan(3, cs, 4, 1, DEV, front="table")
    plan.scores.fill_(7.0)
    tb = tables[cs].table
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    good = dict(keys=p(plan.keys), n=3, w=4, pitch=plan.pitch, cs=cs, table=p(tb), bytes=N, scores=p(plan.scores))
    call = lambda **kw: (lambda a: L.rcp_score_keys(a["keys"], a["n"], a["w"], a["pitch"], a["cs"], a["table"], a["bytes"], a["scores"], stream()))({**good, **kw})
    for kw in (dict(keys=None), dict(keys=p(plan.keys, 8)), dict(n=0), dict(w=0), dict(w=65537), dict(pitch=500), dict(pitch=256), dict(cs=4),
               dict(table=None), dict(table=p(tb, 1)), dict(bytes=N - 1), dict(scores=None), dict(scores=p(plan.scores, 4))):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert bool((plan.scores == 7.0).all())
    assert call() == 0
    other = tables[5 - cs]
    for bad in (object(), None, other):
        with pytest.raises(ValueError):
            plan.score(bad)


# ---------------------------------------------------------------------------------------------------------------- 6. search
def env_from_states(cs, st, n):
    from rubiks_cube_solver_amd import VecCubeEnv
    env = VecCubeEnv(n, DEV, cs, obs=None)
    assert env.stickers.shape == st.shape
    env.stickers.copy_(st)
    return env


def check_solutions(cs, env, res, want_length):
    """Every cube solved with the wanted length, and the moves replay to solved on the oracle's tables."""
    _, _, ops, _, _ = mods()
    cube = beam_ref.Cube(cs)
    n = env.num_envs
    length = res["length"].cpu().numpy()
    assert bool(res["solved"].all()) and (length == want_length).all()
    roots = ops.to_aos(env.stickers, n).cpu().numpy()
    act = res["actions"].cpu().numpy()
    rep = astar_ref.replay(cube, roots, act)
    assert rep[np.minimum(length, len(act)), np.arange(n)].all()
    assert ((act < cube.A).sum(0) == length).all()


@pytest.fixture(scope="module")
def roots222(tables, host_tables):
    """All 2944 states within 5 moves and 2000 states drawn from 14-move walks, as one env; their distances."""
    _, _, ops, _, _ = mods()
    near = np.flatnonzero(host_tables[2] <= 5)
    assert len(near) == sum(group_ref.SPHERES_222[:6]) == 2944
    far = env_of(2, scrambles(2, [14] * 2000, seed=222))
    far_idx = ops.cubies(far.stickers, 2000, 2, cubies=False, status=False, index=True)["corner_index"].cpu().numpy().astype(np.int64)
    idx = np.concatenate([near, far_idx])
    env = env_from_states(2, tables[2].states(torch.from_numpy(idx)), len(idx))
    return env, host_tables[2][idx].astype(np.int32)


def test_weight_one_astar_is_optimal_on_the_222(tables, roots222):
    """B = 1, weight = 1 under the exact heuristic: length == distance == iterations (one geodesic, no detour), every solution
    replays; graph replay equals eager."""
    _, _, _, _, S = mods()
    env, dist = roots222
    res = S.astar_search(tables[2], env, 1, 16, weight=1.0, front="table")
    check_solutions(2, env, res, dist)
    assert (res["iterations"].cpu().numpy() == dist).all() and not bool(res["overflow"].any())
    assert (res["nodes"].cpu().numpy() <= 1 + 5 * dist + (dist > 0)).all()
    g = S.astar_search(tables[2], env, 1, 16, weight=1.0, front="table", graph=True)
    for k in ("solved", "length", "actions", "iterations", "nodes", "overflow"):
        assert torch.equal(res[k], g[k]), k


def test_beam_of_width_one_is_optimal_on_the_222(tables, roots222):
    _, _, _, _, S = mods()
    env, dist = roots222
    res = S.beam_search(tables[2], env, 1, 14, front="table")
    check_solutions(2, env, res, dist)
    g = S.beam_search(tables[2], env, 1, 14, front="table", graph=True)
    for k in ("solved", "length", "actions"):
        assert torch.equal(res[k], g[k]), k
    sym = S.beam_search_symmetric(tables[2], env, 1, 14, symmetries=[0], front="table")
    assert torch.equal(sym["length"], res["length"])
    assert S.beam_solve_percentage(tables[2], 2, 3, 4, 1, 14, front="table") == [100.0] * 3
    assert S.astar_solve_percentage(tables[2], 2, 3, 4, 1, 14, front="table") == [100.0] * 3


# 3x3x3, B = 1, weight 1: iterations and pool nodes the numpy restatement (tests/astar_ref.py with rcp_relax after every merge:
# pattern_ref.relaxed_astar, scored from pattern_ref.bfs(3, 6) with the unknown entries read as 7: every node it pops before the end
# has g + h <= 7, so it never orders by an unknown one) needs to solve EVERY root of walks333() without overflow, found on the CPU;
# the limits below leave room above them.  (Without rcp_relax the same restatement needs 30 624 iterations and 308 740 nodes and
# returns length 9 for three of the 7-move roots: the rule of the rca_* section never lowers a known state's g.)
NEED_333 = {3: (7, 66), 5: (200, 1987), 7: (4230, 41982)}
LIMITS_333 = {3: (16, 128), 5: (256, 2560), 7: (4608, 45056)}


def walks333(k):
    """The 500 walks of k moves: rows of ONE draw of 1500 scrambles (3, 5 and 7 moves, in this order)."""
    scr = scrambles(3, [3] * 500 + [5] * 500 + [7] * 500, seed=333)
    at = {3: 0, 5: 500, 7: 1000}[k]
    return scr[at:at + 500]


@pytest.fixture(scope="module")
def ball5():
    return beam_ref.bfs_distances(beam_ref.Cube(3), 5)[0]


@pytest.mark.parametrize("k", sorted(LIMITS_333))
def test_astar_with_the_corner_bound_on_the_333(tables, ball5, k):
    """500 walks of k moves: every cube solved, h(root) <= length <= k, length = k (mod 2), every solution replays; for k <= 5 the
    length is the exact distance (a numpy ball of radius 5).  The search is the restatement's: it needs no more iterations or nodes."""
    _, _, ops, _, S = mods()
    iters, cap = LIMITS_333[k]
    assert iters >= NEED_333[k][0] and cap >= NEED_333[k][1]
    env = env_of(3, walks333(k))
    h = env.corner_distance(tables[3]).cpu().numpy().astype(np.int32)
    # the long search replays its iteration as a graph and asks the host rarely
    res = S.astar_search(tables[3], env, 1, iters, weight=1.0, capacity=cap, front="table", graph=k == 7, sync_every=4 if k < 7 else 128)
    length = res["length"].cpu().numpy()
    check_solutions(3, env, res, length)
    assert not bool(res["overflow"].any())
    assert (h <= length).all() and (length <= k).all() and ((length - k) % 2 == 0).all()
    print(f"k={k}: lengths {np.bincount(length).tolist()}, iterations max {int(res['iterations'].max())}, nodes max {int(res['nodes'].max())}")
    if k <= 5:
        roots = ops.to_aos(env.stickers, 500).cpu().numpy()
        assert (length == np.array([ball5[r.tobytes()] for r in roots])).all()
    if k == 5:
        g = S.astar_search(tables[3], env, 1, iters, weight=1.0, capacity=cap, front="table", graph=True)
        for key in ("solved", "length", "actions", "iterations", "nodes", "overflow"):
            assert torch.equal(res[key], g[key]), key
    assert (res["iterations"].cpu().numpy() <= NEED_333[k][0]).all() and (res["nodes"].cpu().numpy() <= NEED_333[k][1]).all()


def follow_node_by_node(cs, scr, B, iters, table, host_table):
    """AStarPlan.step with front="table" beside pattern_ref.relaxed_step on the same roots, compared every 8 iterations and at the end.
    -> the restatement's state, the plain rule's state (tests/astar_ref.py, no relax) after the same iterations."""
    _, _, ops, _, S = mods()
    cube = beam_ref.Cube(cs)
    env = env_of(cs, scr)
    roots = cube.scramble(scr)
    cap = 1 + B * (cube.A - 1) * iters
    score = lambda st: -host_table[R.corner_index(cs, st)].astype(np.float32)
    plan = S.AStarPlan(len(scr), cs, B, cap, DEV, front="table", weight=1.0)
    plan.init(env.stickers, env.stickers.shape[-1])
    ref = R.relaxed_astar(cube, roots, B, 0, score, capacity=cap)["state"]
    plain = astar_ref.astar_search(cube, roots, B, iters, score, capacity=cap)["state"]
    for it in range(iters):
        plan.step(table)
        R.relaxed_step(ref, score)
        if it % 8 == 7 or it == iters - 1:
            torch.cuda.synchronize()
            for name in ("g", "parent", "action", "state", "count", "overflow", "ended", "solution"):
                assert (getattr(plan, name).cpu().numpy() == getattr(ref, name)).all(), (it, name)
            live = np.arange(cap)[None, :] < ref.count[:, None]
            assert (plan.prio.cpu().numpy().view(np.uint32).reshape(-1, cap)[live] == ref.prio.view(np.uint32).reshape(-1, cap)[live]).all(), it
            assert (plan.beam.length.cpu().numpy() == ref.length).all() and (plan.beam.active.cpu().numpy() == ref.active).all()
    return ref, plain


@pytest.mark.parametrize("B", (1, 4))
def test_relax_equals_the_restatement_node_by_node(tables, host_tables, B):
    """AStarPlan.step with front="table" (pop, expand, score, merge, rcp_relax) against pattern_ref.relaxed_astar's stages on 7-move
    3x3x3 roots: after every iteration g, parent, action, prio, state and count of every node are the restatement's, and over the
    run some node's g was lowered (the plain rule of tests/astar_ref.py, run beside it, ends with other g)."""
    ref, plain = follow_node_by_node(3, walks333(7)[:48], B, 96 if B == 1 else 48, tables[3], host_tables[3])
    assert ref.relaxed > 0 and (ref.length <= 7).all(), ref.counters()
    assert (ref.g != plain.g).any() or (ref.length != plain.length).any()


def test_relax_equals_the_restatement_node_by_node_on_the_222(tables, host_tables):
    """The 2x2x2 instantiation in a whole search: B = 4 on 48 11-move roots under the exact distances.  Every cube comes out at its
    distance.  (Under the exact heuristic nothing is offered a lower g -- the restatement's counters stay 0 and relax must write
    nothing; what it writes when there are offers is tests/test_gpu_relax.py's.)"""
    scr = scrambles(2, [11] * 48, seed=222)
    ref, _ = follow_node_by_node(2, scr, 4, 16, tables[2], host_tables[2])
    dist = host_tables[2][R.corner_index(2, beam_ref.Cube(2).scramble(scr))]
    assert (ref.active == 0).all() and (ref.length == dist).all() and dist.max() >= 9, (ref.counters(), ref.length, dist)


def relax_argument_errors(tables, cs):
    _, P, _, _, S = mods()
    L = P.pattern_lib()
    plan = S.AStarPlan(3, cs, 4, 64, DEV, front="table", weight=1.0)
    env = env_of(cs, scrambles(cs, [6, 6, 6], seed=1))
    plan.init(env.stickers, env.stickers.shape[-1])
    for _ in range(3):
        plan.step(tables[cs])
    before = [t.clone() for t in (plan.g, plan.parent, plan.action, plan.prio)]
    b = plan.beam
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    good = dict(n=3, cs=cs, B=4, pitch=b.pitch, C=64, w=1.0, flags=p(b.flags), keys=p(b.keys), live=p(b.live), active=p(b.active), pop=p(plan.pop_node),
                pkeys=p(plan.keys), parent=p(plan.parent), action=p(plan.action), g=p(plan.g), score=p(plan.node_score), prio=p(plan.prio),
                state=p(plan.state), count=p(plan.count), table=p(plan.table), tb=plan.table.numel())
    call = lambda **kw: (lambda a: L.rcp_relax(a["n"], a["cs"], a["B"], a["pitch"], a["C"], a["w"], a["flags"], a["keys"], a["live"], a["active"], a["pop"],
                                              a["pkeys"], a["parent"], a["action"], a["g"], a["score"], a["prio"], a["state"], a["count"], a["table"], a["tb"],
                                              stream()))({**good, **kw})
    for kw in (dict(n=0), dict(cs=4), dict(B=0), dict(B=65537), dict(pitch=500), dict(C=0), dict(C=1 << 31), dict(w=float("nan")), dict(w=-1.0),
               dict(w=float("inf")), dict(flags=None), dict(g=None), dict(table=None), dict(keys=p(b.keys, 8)), dict(g=p(plan.g, 4)),
               dict(prio=p(plan.prio, 4)), dict(tb=plan.table.numel() - 8)):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    for t, was in zip((plan.g, plan.parent, plan.action, plan.prio), before):
        assert torch.equal(t.view(torch.uint8), was.view(torch.uint8))
    assert call() == 0


def test_relax_argument_errors_write_nothing(tables):
    relax_argument_errors(tables, 3)


def test_relax_argument_errors_write_nothing_on_the_222(tables):
    relax_argument_errors(tables, 2)


@pytest.mark.parametrize("cs", (2, 3))
def test_symmetric_images_keep_the_corner_distance(tables, host_tables, cs):
    """Table against rcs_sym_apply, a kernel that shares no code with it: a whole-cube symmetry permutes the move set (amap), so the
    image of a state is as far from solved as the state.  4096 random corner indices, 0 and N - 1 -> CornerTable.states -> every
    symmetry's image -> rcp_lookup: the distance is table[index], and no image reads as illegal."""
    _, _, ops, _, _ = mods()
    from rubiks_cube_solver_amd.tables import get_symmetries
    t, N = tables[cs], R.SIZE[cs]
    idx = np.concatenate([np.random.default_rng(cs).integers(0, N, 4096), [0, N - 1]]).astype(np.int64)
    n = len(idx)
    st = t.states(torch.from_numpy(idx))
    want = torch.from_numpy(host_tables[cs][idx]).to(DEV)
    K = get_symmetries(cs).count
    assert K == (48 if cs == 3 else 6) and int(want.max()) >= 11
    moved = 0
    for s in range(K):
        image = ops.apply_symmetry(st, n, None, cs, s)
        got = t.distance(image, n)
        assert not bool((got == 0xFF).any()), s
        assert torch.equal(got, want), s
        moved += int((ops.to_aos(image, n) != ops.to_aos(st, n)).any(1).sum())
    assert moved > (K - 1) * n // 2                                          # the images are other states, not the states again


def test_net_fronts_are_unchanged(tables, dense_before):
    """front="dense" with a random DeepCube: bit-identical to the run made before any table object existed in the process."""
    assert tables[2].table.numel() and tables[3].table.numel()
    for cs in (2, 3):
        assert dense_run(cs) == dense_before[cs]
