"""The edge pattern databases on the GPU (pattern.EdgeTable / MaxTable, the rce_* entry points of librubikhip.so, front="table" of
search.py with a maximum of tables): the built tables against the restatement (tests/edge_ref.py) at every index, the committed level
counts of the 6-piece tables, the tables proved to be distances through the existing move kernels, unrank / look-up / scores in every
layout and over arbitrary bytes, every argument error, each launching export under capture and replay, and whole searches under the
maximum of a corner table and two edge tables.  All comparisons are exact.  GPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import beam_ref
from tests import edge_ref as R
from tests import layout_cases as LC
from tests import pattern_ref
from tests.test_gpu_cubies import FILL, Arena, rows_arena
from tests.test_gpu_pattern import LIMITS_333, check_solutions, walks333
from tests.test_gpu_search import env_of, scrambles

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as C  # noqa: E402
import stream_driver as D  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
COUNTS = (1, 3, 513, 1029, 2565)
CHUNK = 1 << 20
MASK4 = 0x452                     # {1, 4, 6, 10}: the table the layout, score and stream tests read, equal to the restatement at every index
MASK7 = 0xAB5                     # {0, 2, 4, 5, 7, 9, 11}


def mods():
    from rubiks_cube_solver_amd import _edge_lib, _lib, ops, pattern, search
    return _lib, _edge_lib, ops, pattern, search


def stream():
    from rubiks_cube_solver_amd import _lib
    return _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def p(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def astar_bytes(res):
    return [res[k].cpu().numpy().tobytes() for k in ("solved", "length", "actions", "iterations", "nodes", "overflow")]


@pytest.fixture(scope="module")
def corner():
    _, _, _, pattern, _ = mods()
    return pattern.CornerTable.build(3, DEV)


@pytest.fixture(scope="module")
def corner_alone(corner):
    """astar_search under the CornerTable alone on the 500 walks of 3, 5 and 7 moves, BEFORE any edge table exists in the process."""
    _, _, _, _, S = mods()
    out = {}
    for k in sorted(LIMITS_333):
        iters, cap = LIMITS_333[k]
        out[k] = S.astar_search(corner, env_of(3, walks333(k)), 1, iters, weight=1.0, capacity=cap, front="table", graph=k == 7,
                                sync_every=4 if k < 7 else 128)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def small(corner_alone):
    _, _, _, pattern, _ = mods()
    return {m: pattern.EdgeTable.build(R.pieces(m), DEV) for m in R.SMALL_MASKS}


@pytest.fixture(scope="module")
def six(corner_alone):
    _, _, _, pattern, _ = mods()
    return {m: pattern.EdgeTable.build(m, DEV) for m in (R.LOW6, R.HIGH6)}


@pytest.fixture(scope="module")
def host_six(six):
    return {m: t.table.cpu().numpy() for m, t in six.items()}


@pytest.fixture(scope="module")
def host_corner(corner):
    return corner.table.cpu().numpy()


@pytest.fixture(scope="module")
def table4(small):
    t = small[MASK4]
    assert (t.table.cpu().numpy() == R.small(MASK4)[0]).all()
    return t


# ---------------------------------------------------------------------------------------------------------------- 1. build
@pytest.mark.parametrize("mask", R.SMALL_MASKS)
def test_small_tables_equal_the_restatement_at_every_index(small, mask):
    _, E, _, pattern, _ = mods()
    t = small[mask]
    want, levels = R.small(mask)
    got = t.table.cpu().numpy()
    assert t.mask == mask and t.edges == tuple(R.pieces(mask)) and t.levels == levels and t.depth == len(levels) - 1
    assert got.dtype == np.uint8 and len(got) == R.size(len(t.edges)) and (got == want).all() and not (got == 0xFF).any()
    again = pattern.EdgeTable.build(mask, DEV)                               # building twice gives identical bytes
    assert again.levels == t.levels and torch.equal(again.table, t.table)
    wrapped = pattern.EdgeTable(t.table.clone(), t.edges)                    # a table loaded from disk
    assert wrapped.levels is None and wrapped.depth is None and wrapped.mask == mask
    home = R.home_index(mask)
    assert torch.equal(wrapped.distance(t.cubies([home, 0, len(got) - 1]), 3).cpu(), torch.from_numpy(got[[home, 0, len(got) - 1]]))
    broken = t.table.clone()
    broken[home] = 1
    with pytest.raises(ValueError):
        pattern.EdgeTable(broken, mask)
    with pytest.raises(IndexError):
        t.cubies([0, len(got)])


def test_six_piece_levels_are_the_committed_counts(six, host_six):
    for m, t in six.items():
        assert t.levels == R.LEVELS[m] and sum(t.levels) == 42577920 == t.table.numel()
        assert tuple(np.bincount(host_six[m])) == R.LEVELS[m] and host_six[m][R.home_index(m)] == 0


# --------------------------------------------------------------------------- 2. the table is a distance (the device's own moves)
def prove(t, idx):
    """rce_unrank -> rcc_from_cubies (status 0 from rcc_cubies) -> rc_expand_children -> child codes -> rce_lookup, in chunks:
    h(parent) = table[i], the unranked cube reads back as i, |h(child) - h(parent)| <= 1, h > 0 => some child has h - 1, h == 0 <=> home.
    A byte array with these properties IS the least number of quarter turns that bring the pattern home."""
    _, _, ops, _, _ = mods()
    home = R.home_index(t.mask)
    for at in range(0, len(idx), CHUNK):
        part = torch.from_numpy(idx[at:at + CHUNK])
        n = len(part)
        st = t.states(part)
        assert not bool(ops.cubies(st, n, 3, cubies=False, status=True)["status"].any())
        code = ops.alloc_code(n, 3, DEV, st.shape[-1])
        out = ops.expand_buffers(n, 3, DEV, st.shape[-1], children=False, codes=True)
        ops.encode(st, n, 3, code, 1)
        ops.expand_children(st, n, 3, None, out["child_solved"], out["child_code"], pitch=st.shape[-1])
        h = t.distance(code, n).int()
        assert torch.equal(h, t.table[part.to(DEV)].int())
        down = torch.zeros(n, dtype=torch.bool, device=DEV)
        for a in range(12):
            hc = t.distance(out["child_code"][a], n).int()
            assert bool(((hc - h).abs() <= 1).all()), a
            down |= hc == h - 1
        assert bool((down == (h > 0)).all())
        assert bool(((h == 0) == (part.to(DEV) == home)).all())


def test_six_piece_table_is_the_distance_through_the_move_kernels(six):
    N = six[R.LOW6].table.numel()
    prove(six[R.LOW6], np.concatenate([np.arange(5, N, 16, dtype=np.int64), [0, R.home_index(R.LOW6), N - 1]]))


def test_seven_piece_table_builds_and_is_a_distance(six):
    _, _, _, pattern, _ = mods()
    t = pattern.EdgeTable.build(R.pieces(MASK7), DEV)
    N = R.size(7)
    assert t.table.numel() == N and sum(t.levels) == N and t.levels[0] == 1 and t.levels[1] == 12
    print(f"k=7 mask {MASK7:#x}: levels {t.levels}")
    prove(t, np.concatenate([np.arange(77, N, 4096, dtype=np.int64), [0, R.home_index(MASK7), N - 1]]))


# ---------------------------------------------------------------------------------------------------------- 3. layouts
def doctor(rows, mask):
    """rows [n >= 8, 20] of legal cubes -> a copy whose cubes 0..3 are illegal for `mask`, cube 4 is odd but legal for it."""
    t = R.pieces(mask)
    u = [q for q in range(12) if q not in t]
    bad = rows.copy()
    slot_of = lambda r, piece: 8 + int(np.flatnonzero(bad[r, 8:] >> 1 == piece)[0])
    bad[0, slot_of(0, u[0])] = 24                                            # a byte >= 24 in an untracked piece's slot
    bad[1, slot_of(1, u[0])] = 2 * t[0]                                      # a tracked piece twice
    bad[2, slot_of(2, t[-1])] = 2 * u[1] + 1                                 # a tracked piece absent
    bad[3, slot_of(3, t[0])] = 0xFF
    bad[4, slot_of(4, u[0])] = 2 * u[1]                                      # an untracked piece twice, another absent: not looked at
    bad[5, :8] = 0xFF                                                        # corner rows are not read
    return bad, 4


@pytest.mark.parametrize("n", COUNTS)
def test_unrank_and_lookup_in_every_layout_carved(table4, n):
    """rce_unrank into layout X and rce_lookup from it, every operand 16 bytes past a 32-byte boundary: the rows are the
    restatement's, an index >= N is written solved and flagged, the distances are the table's, doctored rows read 0xFF without a
    table read, guards and pad columns keep their bytes.  The doctored buffer is an RC_FMT_CODE-like one: its corner rows hold FILL."""
    _, E, _, _, _ = mods()
    L, t = E.edge_lib(), table4
    N = t.table.numel()
    host = R.small(MASK4)[0]
    rng = np.random.default_rng(n)
    idx = rng.integers(0, N, n).astype(np.uint32)
    idx[0] = N - 1
    for flagged in (False, True):
        if flagged:
            idx[n - 1] = N                                                   # the first index outside, in the ragged last pack
            if n > 600:
                idx[[7, 600]] = 0xFFFFFFFF, N + 12345
        want, bad = R.unrank_cubies(MASK4, idx.astype(np.int64))
        assert bad.any() == flagged
        dist_want = np.where(bad, 0, host[np.minimum(idx.astype(np.int64), N - 1)]).astype(np.uint8)
        for lay in LC.LAYOUTS:
            offs = LC.carve_offsets(4)
            ind = Arena(4 * n, offs[0])
            ind.expect(idx)
            ind.upload()
            cub = rows_arena(None, n, 20, lay, offs[1]).upload()
            flag = Arena(16, offs[2])
            flag.host[flag.start] = 0
            flag.upload()
            dist = Arena(n, offs[3]).upload()
            assert L.rce_unrank(ind.ptr(), n, MASK4, cub.ptr(), cub.pitch, flag.ptr(), stream()) == 0, L.rc_last_error()
            assert L.rce_lookup(cub.ptr(), n, cub.pitch, MASK4, p(t.table), N, dist.ptr(), stream()) == 0, L.rc_last_error()
            cub.expect_rows(want, cub.pitch)
            flag.host[flag.start] = int(flagged)
            dist.expect(dist_want)
            for a, what in ((ind, "indices"), (cub, "cubies"), (flag, "bad"), (dist, "out")):
                a.check(f"n={n} {lay} flagged={flagged}: {what}")
            if n >= 8 and not flagged:
                rows, n_bad = doctor(want, MASK4)
                rows[6:, :8] = FILL
                code = rows_arena(rows, n, 20, lay, offs[1]).upload()
                dist2 = Arena(n, offs[3]).upload()
                assert L.rce_lookup(code.ptr(), n, code.pitch, MASK4, p(t.table), N, dist2.ptr(), stream()) == 0
                w2 = dist_want.copy()
                w2[:n_bad] = 0xFF
                assert (R.index_of_bytes(MASK4, rows[:, 8:])[:n_bad] == 0xFFFFFFFF).all() and (R.index_of_bytes(MASK4, rows[:, 8:])[n_bad:] == idx[n_bad:]).all()
                dist2.expect(w2)
                code.check("doctored rows")
                dist2.check(f"n={n} {lay}: doctored out")


def test_distance_of_an_env_and_of_walks(six, host_six, corner, host_corner):
    """Admissibility on walks of k = 1..20 moves, 500 cubes each: every member's h <= k, MaxTable.distance is their maximum, and the
    members' distances are the host tables' at the restatement's index."""
    _, _, ops, pattern, _ = mods()
    k = np.repeat(np.arange(1, 21), 500)
    env = env_of(3, scrambles(3, list(k), seed=20))
    mx = pattern.MaxTable(corner, six[R.LOW6], six[R.HIGH6])
    hm = env.edge_distance(mx).cpu().numpy().astype(np.int64)
    st = ops.to_aos(env.stickers, len(k)).cpu().numpy()
    parts = [host_corner[pattern_ref.corner_index(3, st)]]
    for m in (R.LOW6, R.HIGH6):
        h = env.edge_distance(six[m]).cpu().numpy()
        assert (h == host_six[m][R.index_of_states(m, st)]).all()
        parts.append(h)
    assert (parts[0] == env.corner_distance(corner).cpu().numpy()).all()
    assert (hm == np.max(parts, axis=0)).all() and (hm <= k).all() and all((hm >= x).all() for x in parts)
    assert (hm > parts[0]).any() and (hm > parts[1]).any()                   # each kind of table decides somewhere
    only = pattern.MaxTable(None, six[R.LOW6])
    assert torch.equal(only.distance(env), six[R.LOW6].distance(env))


# ---------------------------------------------------------------------------------------------------------------- 4. scores
def slot_bytes(plan):
    """[A * nbp, 12]: the edge bytes of every candidate slot, j = a * nbp + tile * pitch + column."""
    code = plan.code.cpu().numpy()                                           # [A * tiles, 20, pitch]
    return code[:, 8:, :].transpose(0, 2, 1).reshape(-1, 12)


@pytest.mark.parametrize("P,W", ((40, 5), (3, 300)))
def test_scores_of_every_candidate_slot(table4, six, host_six, P, W):
    """A real rc_search_expand over a poisoned code buffer, then rce_score_codes: every slot's score equals numpy, for combine 0 and
    1 -- the live candidates, the slots past `live` as expand left them, and slots past `live` holding arbitrary bytes."""
    _, _, _, _, S = mods()
    plan = S.BeamPlan(P, 3, W, 1, DEV, front="table")
    rng = np.random.default_rng(P * W)
    plan.code.copy_(torch.from_numpy(rng.integers(0, 26, tuple(plan.code.shape), dtype=np.uint8)))
    env = env_of(3, scrambles(3, [1 + i % 9 for i in range(P)], seed=P + W))
    plan.init(env.stickers, env.stickers.shape[-1])
    plan.expand(0)
    torch.cuda.synchronize()
    live = (plan.flags.cpu().numpy() & 1).astype(bool)
    assert live.any() and not live.all()
    # rc_search_expand writes a code into EVERY slot (edge bytes below 24 always), so the poison is gone.  The contract calls the bytes
    # of a slot past `live` arbitrary: every second one of them gets arbitrary bytes again, values of 24 and 25 among them.
    dead = np.flatnonzero(~live.reshape(-1))[::2]
    code = plan.code.cpu().numpy().transpose(0, 2, 1).reshape(-1, 20).copy()
    code[dead] = rng.integers(0, 26, (len(dead), 20), dtype=np.uint8)
    plan.code.copy_(torch.from_numpy(code.reshape(plan.code.shape[0], plan.code.shape[2], 20).transpose(0, 2, 1).copy()))
    e = slot_bytes(plan)
    for mask, t, host in ((MASK4, table4, R.small(MASK4)[0]), (R.LOW6, six[R.LOW6], host_six[R.LOW6])):
        tr = R.pieces(mask)
        ix = R.index_of_bytes(mask, e).astype(np.int64)
        want = np.where(ix == 0xFFFFFFFF, 255, host[np.minimum(ix, len(host) - 1)]).astype(np.float32)
        small_bytes = (e < 24).all(1)
        count = np.stack([(e >> 1 == x).sum(1) for x in tr], 1)
        kinds = {"a byte >= 24": ~small_bytes, "a tracked piece twice": small_bytes & (count > 1).any(1),
                 "a tracked piece absent": small_bytes & (count == 0).any(1)}
        for name, hit in kinds.items():
            assert hit.any() and (want[hit] == 255).all(), name
        assert (want[live.reshape(-1)] < 255).all()
        plan.scores.fill_(float("nan"))
        t.score_codes(plan.code, P, W, plan.pitch, plan.scores, combine=0)
        got = plan.scores.cpu().numpy().reshape(-1)
        assert (got.view(np.uint32) == (-want).view(np.uint32)).all()        # -0.0 for h = 0, bit for bit
        old = np.resize(np.array([0.0, -0.0, -255.0, -3.0, -7.5, 2.0, -1.0, -300.0, -4.0], np.float32), len(want))
        plan.scores.copy_(torch.from_numpy(old).view(plan.scores.shape))
        t.score_codes(plan.code, P, W, plan.pitch, plan.scores, combine=1)
        got = plan.scores.cpu().numpy().reshape(-1)
        mixed = np.where(-want < old, -want, old)
        assert (got.view(np.uint32) == mixed.view(np.uint32)).all() and (mixed != old).any() and (mixed == old).any()
        assert (got[want == 255] <= -255).all()


def test_max_table_scores_are_the_maximum(corner, host_corner, six, host_six):
    """BeamPlan.score with a MaxTable = rcp_score_keys, then one rce_score_codes(combine=1) per edge table: at every live slot the
    negated maximum of the three host tables; a MaxTable without a corner table starts with combine=0."""
    _, _, ops, pattern, S = mods()
    P, W = 40, 5
    plan = S.BeamPlan(P, 3, W, 1, DEV, front="table")
    env = env_of(3, scrambles(3, [2 + i % 9 for i in range(P)], seed=8))
    plan.init(env.stickers, env.stickers.shape[-1])
    plan.expand(0)
    mx = pattern.MaxTable(corner, six[R.LOW6], six[R.HIGH6])
    plan.scores.fill_(float("nan"))
    plan.score(mx)
    got = plan.scores.cpu().numpy()
    e = slot_bytes(plan)
    he = [np.where((ix := R.index_of_bytes(m, e).astype(np.int64)) == 0xFFFFFFFF, 255, host_six[m][np.minimum(ix, 42577919)]) for m in (R.LOW6, R.HIGH6)]
    plan.scores.fill_(float("nan"))
    corner.score_keys(plan.keys, P, W, plan.pitch, plan.scores)
    hc = -plan.scores.cpu().numpy().reshape(-1)
    want = np.maximum(hc, np.maximum(he[0], he[1]).astype(np.float32))
    assert (got.reshape(-1) == -want).all()
    plan.scores.fill_(float("nan"))
    plan.score(pattern.MaxTable(None, six[R.LOW6], six[R.HIGH6]))
    assert (plan.scores.cpu().numpy().reshape(-1) == -np.maximum(he[0], he[1]).astype(np.float32)).all()
    live = (plan.flags.cpu().numpy() & 1).astype(bool).reshape(-1)
    assert live.any() and (want[live] < 255).all()


# ------------------------------------------------------------------------------------------------------- 5. argument errors
def test_argument_errors_write_nothing(table4):
    _, E, _, pattern, S = mods()
    L, t, n = E.edge_lib(), table4, 513
    N = t.table.numel()
    before = t.table.clone()
    rows = rows_arena(None, n, 20, "tight", 0).upload()
    out = Arena(n + 16, 0).upload()
    cnt = torch.zeros(4, dtype=torch.int32, device=DEV)
    flag = torch.zeros(16, dtype=torch.uint8, device=DEV)
    ind = torch.zeros(16, dtype=torch.int32, device=DEV)
    cub = torch.full((20, 16), FILL, dtype=torch.uint8, device=DEV)
    plan = S.BeamPlan(3, 3, 4, 1, DEV, front="table")
    plan.scores.fill_(7.0)
    tb, sp = t.table, stream()
    bad_masks = (0, 0x0FF, 0x1000, 0x1452, -1)                               # no piece, k = 8, bits above 11
    refused = []
    for m in bad_masks:
        refused += [L.rce_build_begin(p(tb), N, m, sp), L.rce_build_level(p(tb), N, m, 0, p(cnt), sp), L.rce_unrank(p(ind), 3, m, p(cub), 16, p(flag), sp),
                    L.rce_lookup(rows.ptr(), n, rows.pitch, m, p(tb), N, out.ptr(), sp),
                    L.rce_score_codes(p(plan.code), 3, 4, plan.pitch, m, p(tb), N, p(plan.scores), 0, sp)]
    M = MASK4
    refused += [L.rce_build_begin(None, N, M, sp), L.rce_build_begin(p(tb, 8), N, M, sp), L.rce_build_begin(p(tb), N - 1, M, sp),
                L.rce_build_begin(p(tb), -1, M, sp),
                L.rce_build_level(p(tb), N - 1, M, 0, p(cnt), sp), L.rce_build_level(p(tb), N, M, -1, p(cnt), sp),
                L.rce_build_level(p(tb), N, M, 254, p(cnt), sp), L.rce_build_level(p(tb), N, M, 0, None, sp),
                L.rce_build_level(p(tb), N, M, 0, p(cnt, 4), sp), L.rce_build_level(None, N, M, 0, p(cnt), sp),
                L.rce_unrank(None, 3, M, p(cub), 16, p(flag), sp), L.rce_unrank(p(ind, 4), 3, M, p(cub), 16, p(flag), sp),
                L.rce_unrank(p(ind), 3, M, None, 16, p(flag), sp), L.rce_unrank(p(ind), 3, M, p(cub, 8), 16, p(flag), sp),
                L.rce_unrank(p(ind), 3, M, p(cub), 8, p(flag), sp), L.rce_unrank(p(ind), 17, M, p(cub), 16, p(flag), sp),
                L.rce_unrank(p(ind), 3, M, p(cub), 16, None, sp), L.rce_unrank(p(ind), -1, M, p(cub), 16, p(flag), sp)]
    assert all(rc == EINVAL for rc in refused), refused
    good = dict(rows=rows.ptr(), n=n, pitch=rows.pitch, mask=M, table=p(tb), bytes=N, out=out.ptr())
    call = lambda **kw: (lambda a: L.rce_lookup(a["rows"], a["n"], a["pitch"], a["mask"], a["table"], a["bytes"], a["out"], sp))({**good, **kw})
    for word, kw in [("rows", dict(rows=None)), ("rows", dict(rows=p(rows.view, 8))), ("n is", dict(n=-1)), ("pitch", dict(pitch=rows.pitch - 8)),
                     ("pitch", dict(pitch=256)), ("table", dict(table=None)), ("table", dict(table=p(tb, 4))), ("bytes", dict(bytes=N - 1)),
                     ("bytes", dict(bytes=0)), ("out", dict(out=None)), ("out", dict(out=p(out.view, 4))), ("mask", dict(mask=0))]:
        assert call(**kw) == EINVAL, (word, kw)
        assert word in L.rc_last_error().decode(), (word, L.rc_last_error())
    good2 = dict(code=p(plan.code), n=3, w=4, pitch=plan.pitch, mask=M, table=p(tb), bytes=N, scores=p(plan.scores), combine=0)
    call2 = lambda **kw: (lambda a: L.rce_score_codes(a["code"], a["n"], a["w"], a["pitch"], a["mask"], a["table"], a["bytes"], a["scores"], a["combine"],
                                                     sp))({**good2, **kw})
    for kw in (dict(code=None), dict(code=p(plan.code, 8)), dict(n=0), dict(w=0), dict(w=65537), dict(pitch=500), dict(pitch=256), dict(table=None),
               dict(table=p(tb, 1)), dict(bytes=N - 1), dict(scores=None), dict(scores=p(plan.scores, 4)), dict(combine=2), dict(combine=-1)):
        assert call2(**kw) == EINVAL, kw
    assert call(n=0) == 0 and L.rce_unrank(p(ind), 0, M, p(cub), 16, p(flag), sp) == 0       # n == 0 succeeds without a launch
    torch.cuda.synchronize()
    rows.check("rows")
    out.check("out after the refused calls")
    assert torch.equal(tb, before) and not bool(flag.any()) and not bool(cnt.any()) and bool((cub == FILL).all()) and bool((plan.scores == 7.0).all())
    assert call2() == 0
    # the Python layer
    env2 = env_of(2, scrambles(2, [3, 3], seed=1))
    with pytest.raises(ValueError):
        t.distance(env2)
    with pytest.raises(ValueError):
        pattern.EdgeTable.build([0], DEV, cube_size=2)
    for bad in (object(), None, t):                                          # a bare EdgeTable is no model of front="table"
        with pytest.raises(ValueError):
            plan.score(bad)


def test_max_table_value_errors_come_before_any_launch(corner, six):
    _, _, _, pattern, S = mods()
    for members in ((), (None,), (corner, "x"), (six[R.LOW6],), (None, corner)):
        with pytest.raises(ValueError):
            pattern.MaxTable(*members)
    mx = pattern.MaxTable(corner, six[R.LOW6])
    env = env_of(3, scrambles(3, [3, 3], seed=1))
    before = env.stickers.clone()
    with pytest.raises(ValueError):
        S._check_table(mx, 3, torch.device("cuda", torch.cuda.current_device() + 1))     # a MaxTable on another device than the cubes
    with pytest.raises(ValueError):
        S._check_table(mx, 2)
    env2 = env_of(2, scrambles(2, [3, 3], seed=1))
    for call in (lambda: S.astar_search(mx, env2, 1, 4, front="table"), lambda: S.beam_search(mx, env2, 1, 4, front="table"),
                 lambda: S.beam_search_symmetric(mx, env2, 1, 4, front="table"), lambda: S.beam_solve_percentage(mx, 2, 2, 2, 1, 4, front="table"),
                 lambda: S.astar_solve_percentage(mx, 2, 2, 2, 1, 4, front="table")):
        with pytest.raises(ValueError):
            call()
    assert torch.equal(env.stickers, before)


# -------------------------------------------------------------------------------------------------------- 6. stream order
def _host4(ctx):
    if "edge4" not in ctx.cache:
        ctx.cache["edge4"] = ctx.torch.as_tensor(np.array(R.small(MASK4)[0])).to(ctx.dev)
    return ctx.cache["edge4"]


def _s_build_begin(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _edge_lib, _lib
    nb = R.size(4)
    table = arena.output((nb,))
    home = R.home_index(MASK4)

    def check(w):
        got = table.cpu().numpy()
        assert got[home] == 0 and (np.delete(got, home) == 0xFF).all()
    return C.built(lambda: _lib.check(_edge_lib.edge_lib().rce_build_begin(C.P(table), nb, MASK4, ctx.sp())), [], check)


def _s_build_level(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _edge_lib, _lib
    t = ctx.torch
    depth, nb = int(variant), R.size(4)
    dist, levels = R.small(MASK4)
    start = t.as_tensor(np.where(dist <= depth, dist, 0xFF).astype(np.uint8))
    want = np.where(dist <= depth + 1, dist, 0xFF).astype(np.uint8)
    want_count = levels[depth + 1] if depth + 1 < len(levels) else 0
    table, count = arena.state((nb,)), arena.output((4,), t.int32)

    def check(w):
        C.vec_same(table, want, "table")
        assert int(count[0]) == want_count, ("count", int(count[0]), want_count)
    return C.built(lambda: _lib.check(_edge_lib.edge_lib().rce_build_level(C.P(table), nb, MASK4, depth, C.P(count), ctx.sp())),
                   [lambda w: table.copy_(start)], check)


def _s_indices(w):
    i = np.random.default_rng(C._SEED[w]).integers(0, R.size(4), C.N).astype(np.int64)
    i[11 if w == "A" else 1000] = R.size(4) + 5
    return i


def _s_unrank(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _edge_lib, _lib
    n = C.N
    idxs = {w: _s_indices(w) for w in C.SETS}
    index, f1 = C.vec_input(ctx, arena, {w: idxs[w].astype(np.uint32).view(np.int32) for w in C.SETS})
    cub, bad = arena.output((C.tiles_of(n), 20, C.pitch_of(n))), arena.state((16,))

    def check(w):
        e_cub, e_bad = R.unrank_cubies(MASK4, idxs[w])
        assert e_bad.sum() == 1
        C.same(ctx, cub, n, e_cub, "cubies")
        assert bad.cpu().numpy().tolist() == [1] + [0] * 15, "bad"
    return C.built(lambda: _lib.check(_edge_lib.edge_lib().rce_unrank(C.P(index), n, MASK4, C.P(cub), C.pitch_of(n), C.P(bad), ctx.sp())),
                   [f1, lambda w: bad.zero_()], check)


def _s_rows(w):
    rows, _ = R.unrank_cubies(MASK4, np.minimum(_s_indices(w), R.size(4) - 1))
    return doctor(rows, MASK4)[0]


def _s_lookup(ctx, cs, variant, arena):
    from rubiks_cube_solver_amd import _edge_lib, _lib
    n, table = C.N, _host4(ctx)
    host = {w: C.tiled(ctx, _s_rows(w), n) for w in C.SETS}
    src, out = arena.input((C.tiles_of(n), 20, C.pitch_of(n))), arena.output((n,))

    def check(w):
        ix = R.index_of_bytes(MASK4, _s_rows(w)[:, 8:]).astype(np.int64)
        want = np.where(ix == 0xFFFFFFFF, 0xFF, R.small(MASK4)[0][np.minimum(ix, R.size(4) - 1)]).astype(np.uint8)
        assert (want == 0xFF).any() and (want < 5).any()
        C.vec_same(out, want, "out")
    return C.built(lambda: _lib.check(_edge_lib.edge_lib().rce_lookup(C.P(src), n, C.pitch_of(n), MASK4, C.P(table), table.numel(), C.P(out), ctx.sp())),
                   [lambda w: src.copy_(host[w])], check)


def _s_score(ctx, cs, variant, arena):
    """variant "<P>x<W>x<combine>": every slot of the code buffer holds edge bytes -- of a pattern, or arbitrary ones (dead slots)."""
    from rubiks_cube_solver_amd import _edge_lib, _lib, search
    t = ctx.torch
    Pn, W, combine = (int(x) for x in variant.split("x"))
    pitch = search.beam_pitch(Pn * W)
    tiles = -(-Pn * W // pitch)
    total = 12 * tiles * pitch
    table, dist = _host4(ctx), R.small(MASK4)[0]
    M = {}
    for w in C.SETS:
        rng = np.random.default_rng(C._SEED[w] + Pn)
        rows = R.unrank_cubies(MASK4, rng.integers(0, R.size(4), total))[0]
        junk = rng.random(total) < 0.1
        rows[junk, 8:] = rng.integers(0, 26, (int(junk.sum()), 12), dtype=np.uint8)
        ix = R.index_of_bytes(MASK4, rows[:, 8:]).astype(np.int64)
        h = np.where(ix == 0xFFFFFFFF, 255, dist[np.minimum(ix, R.size(4) - 1)]).astype(np.float32)
        old = np.resize(np.array([0.0, -0.0, -255.0, -3.0, -7.5, 2.0, -1.0], np.float32), total)
        M[w] = dict(code=rows.reshape(12 * tiles, pitch, 20).transpose(0, 2, 1).copy(), old=old,
                    want=np.where(-h < old, -h, old) if combine else -h)
        assert (h == 255).any() and (h < 5).any()
    code, f1 = C.vec_input(ctx, arena, {w: M[w]["code"] for w in C.SETS})
    scores = (arena.state if combine else arena.output)((12, tiles * pitch), t.float32)
    fills = [f1] + ([lambda w: scores.copy_(t.as_tensor(M[w]["old"]).view(scores.shape))] if combine else [])

    def check(w):
        assert (scores.cpu().numpy().reshape(-1).view(np.uint32) == M[w]["want"].view(np.uint32)).all(), "scores"
    return C.built(lambda: _lib.check(_edge_lib.edge_lib().rce_score_codes(C.P(code), Pn, W, pitch, MASK4, C.P(table), table.numel(), C.P(scores), combine,
                                                                          ctx.sp())), fills, check)


# the form of tests/stream_cases.py ROWS, kept here: that table is pinned to the eight signature tables it lists
EDGE_ROWS = [C.Row("rce_build_begin", _s_build_begin, (3,)), C.Row("rce_build_level", _s_build_level, (3,), (0, 3, 9)),
             C.Row("rce_unrank", _s_unrank, (3,)), C.Row("rce_lookup", _s_lookup, (3,)),
             C.Row("rce_score_codes", _s_score, (3,), ("40x5x0", "3x300x0", "40x5x1", "3x300x1"))]
EDGE_CASES = [(f"{r.label}-{v}", r, v) for r in EDGE_ROWS for v in r.variants]


def test_every_launching_export_has_a_stream_row():
    from rubiks_cube_solver_amd import _edge_lib
    host_only = {"rce_table_bytes", "rce_home_index", "rce_tables"}          # launch nothing
    assert {r.export for r in EDGE_ROWS} == set(_edge_lib.EDGE_SIGNATURES) - host_only
    assert not {r.export for r in EDGE_ROWS} & {r.export for r in C.ROWS}


@pytest.fixture(scope="module")
def ctx(oracle):
    return C.Ctx(oracle, "cuda")


@pytest.mark.parametrize("row,variant", [c[1:] for c in EDGE_CASES], ids=[c[0] for c in EDGE_CASES])
def test_one_call_under_capture_and_replay(ctx, row, variant):
    from tests.test_gpu_stream_order import GraphBackend
    try:
        with torch.no_grad():
            D.run(GraphBackend(ctx.ops, ctx.L), lambda arena: row.build(ctx, 3, variant, arena))
    except Exception as e:  # noqa: BLE001
        if any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError")) and "capture" not in str(e).lower():
            pytest.exit(f"a GPU fault in this case: nothing more is started on the device -- {e}", returncode=3)
        raise


# ---------------------------------------------------------------------------------------------------------------- 7. search
@pytest.fixture(scope="module")
def maxtable(corner, six):
    _, _, _, pattern, _ = mods()
    return pattern.MaxTable(corner, six[R.LOW6], six[R.HIGH6])


def host_score(host_corner, host_six):
    def score(st):
        h = host_corner[pattern_ref.corner_index(3, st)]
        for m in (R.LOW6, R.HIGH6):
            h = np.maximum(h, host_six[m][R.index_of_states(m, st)])
        return -h.astype(np.float32)
    return score


@pytest.mark.parametrize("k", sorted(LIMITS_333))
def test_astar_under_the_maximum_on_the_333(maxtable, corner, corner_alone, k):
    """The 500 walks of k moves, batch 1, weight 1: every cube solved, h(root) <= length <= k, and the length is the CornerTable-alone
    run's for every cube (both are A* proper under a consistent bound, so both are optimal).  Iterations and nodes are printed, not
    asserted: a dominating consistent bound does not guarantee fewer expansions per instance under ties.  Then the CornerTable-alone
    search once more: bit-equal to the run made before any edge table existed."""
    _, _, _, _, S = mods()
    iters, cap = LIMITS_333[k]
    env = env_of(3, walks333(k))
    h = env.edge_distance(maxtable).cpu().numpy().astype(np.int32)
    kw = dict(weight=1.0, capacity=cap, front="table", graph=k == 7, sync_every=4 if k < 7 else 128)
    res = S.astar_search(maxtable, env, 1, iters, **kw)
    length = res["length"].cpu().numpy()
    check_solutions(3, env, res, length)
    assert not bool(res["overflow"].any())
    assert (h <= length).all() and (length <= k).all()
    base = corner_alone[k]
    assert (length == base["length"].cpu().numpy()).all()
    print(f"k={k}: iterations max {int(res['iterations'].max())} sum {int(res['iterations'].sum())} (corner alone {int(base['iterations'].max())}, "
          f"{int(base['iterations'].sum())}); nodes max {int(res['nodes'].max())} sum {int(res['nodes'].sum())} (corner alone "
          f"{int(base['nodes'].max())}, {int(base['nodes'].sum())})")
    again = S.astar_search(corner, env, 1, iters, **kw)
    assert astar_bytes(again) == astar_bytes(base)


def test_small_astar_followed_node_by_node(maxtable, host_corner, host_six):
    """AStarPlan.step with a MaxTable (P = 3, B = 4) beside pattern_ref.relaxed_step fed with the device tables' own scores: after
    every iteration g, parent, action, prio, state and count of every node are the restatement's."""
    _, _, _, _, S = mods()
    cube = beam_ref.Cube(3)
    scr = walks333(7)[:3]
    env, roots = env_of(3, scr), cube.scramble(scr)
    B, iters = 4, 24
    cap = 1 + B * (cube.A - 1) * iters
    score = host_score(host_corner, host_six)
    plan = S.AStarPlan(3, 3, B, cap, DEV, front="table", weight=1.0)
    plan.init(env.stickers, env.stickers.shape[-1])
    ref = pattern_ref.relaxed_astar(cube, roots, B, 0, score, capacity=cap)["state"]
    for it in range(iters):
        plan.step(maxtable)
        pattern_ref.relaxed_step(ref, score)
        torch.cuda.synchronize()
        for name in ("g", "parent", "action", "state", "count", "overflow", "ended", "solution"):
            assert (getattr(plan, name).cpu().numpy() == getattr(ref, name)).all(), (it, name)
        live = np.arange(cap)[None, :] < ref.count[:, None]
        assert (plan.prio.cpu().numpy().view(np.uint32).reshape(-1, cap)[live] == ref.prio.view(np.uint32).reshape(-1, cap)[live]).all(), it
        assert (plan.beam.length.cpu().numpy() == ref.length).all() and (plan.beam.active.cpu().numpy() == ref.active).all()
    assert (ref.count > 1).all()


def test_beam_followed_depth_by_depth(maxtable, host_corner, host_six):
    """BeamPlan.step with a MaxTable (P = 40, W = 5) beside beam_ref.Stepper: at every depth the device's scores of every candidate
    are the host tables' maximum, and the Stepper fed with them keeps as many per problem, ends with the same lengths and moves."""
    _, _, _, _, S = mods()
    cube = beam_ref.Cube(3)
    P, W, depth = 40, 5, 6
    scr = scrambles(3, [1 + i % 6 for i in range(P)], seed=40)
    env, roots = env_of(3, scr), cube.scramble(scr)
    score = host_score(host_corner, host_six)
    plan = S.BeamPlan(P, 3, W, depth, DEV, front="table")
    plan.init(env.stickers, env.stickers.shape[-1])
    ref = beam_ref.Stepper(cube, roots, W, depth)
    for d in range(depth):
        plan.expand(d & 1)
        plan.score(maxtable)
        ref.expand()
        dev = plan.scores.cpu().numpy()                                      # [A, nbp]: candidate c = w * A + a of problem p at [a, p * W + w]
        scores = {}
        for pr, cd in ref.cand.items():
            mine = dev[cd["a"], pr * W + cd["w"]]
            assert (mine == score(cd["children"])).all(), (d, pr)
            scores[pr] = mine
        plan.select()
        ref.select(scores)
        assert (plan.sel_count.cpu().numpy() == ref.sel_count()).all(), d
        plan.advance(d & 1)
        plan.depth.add_(1)
        ref.advance()
        assert (plan.live.cpu().numpy() == ref.live).all() and (plan.length.cpu().numpy() == ref.length).all(), d
    plan.backtrack()
    assert (plan.actions.cpu().numpy() == ref.backtrack()).all() and (ref.length >= 0).sum() >= P // 2
    res = S.beam_search(maxtable, env, W, depth, front="table")
    assert (res["length"].cpu().numpy() == ref.length).all() and (res["actions"].cpu().numpy() == ref.backtrack()).all()
    sym = S.beam_search_symmetric(maxtable, env, W, depth, symmetries=[0], front="table")
    assert torch.equal(sym["length"], res["length"])
    assert S.beam_solve_percentage(maxtable, 3, 2, 4, 12, 4, front="table") == [100.0] * 2
    assert S.astar_solve_percentage(maxtable, 3, 2, 4, 1, 32, front="table") == [100.0] * 2
