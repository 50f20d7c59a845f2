"""The oracle against the cube group itself (CPU).  Every number asserted here is a published fact or follows from one
(tests/group_ref.py): sphere sizes of both cubes (OEIS A079762 / A080601), the 3 674 160 states of the 2x2x2, orders of move words,
commuting faces, splitmix64's test vector.  Nothing here compares the oracle with a fixture or with the product: an error made the
same way in `tables.py`, `rc_tables.h` and `oracle_np.tables_222()` passes every parity test, and fails these.
All comparisons are exact."""
import numpy as np
import pytest

from tests import group_ref as G


@pytest.fixture(scope="module")
def levels_222(oracle):
    return G.oracle_bfs(oracle, 2, None)


@pytest.fixture(scope="module")
def levels_333(oracle):
    return G.oracle_bfs(oracle, 3, 7)


def test_222_spheres_are_the_whole_group(levels_222):
    """d = 0..14 = A079762, 3 674 160 states in all, depth 15 empty (the search stopped by itself: the last level's children are all
    known states)."""
    assert tuple(len(lv.states) for lv in levels_222) == G.SPHERES_222
    assert sum(len(lv.states) for lv in levels_222) == G.GROUP_222
    assert levels_222[-1].child_code is not None                                  # level 14 WAS expanded and gave nothing new


def test_222_exactly_one_solved_state(oracle, levels_222):
    """The solved flag of the expansion is set on the root's level only, and on every child that IS the solved row and no other."""
    assert [int(lv.solved.sum()) for lv in levels_222] == [1] + [0] * 14
    for lv in levels_222:
        assert ((lv.child_solved != 0) == lv.children_equal_solved).all(), lv.depth
    assert int(sum(lv.children_equal_solved.sum() for lv in levels_222)) == 6    # the six states of depth 1, one move each
    allst = np.concatenate([lv.states for lv in levels_222])
    assert len(allst) == G.GROUP_222 and int(oracle.is_solved(2, allst).sum()) == 1


def test_222_code_is_injective_and_tables_build(levels_222):
    code = np.concatenate([lv.code for lv in levels_222])
    assert G.count_distinct(G.pack_code(code, 21)) == G.GROUP_222
    g = G.build_222(levels_222)
    assert int((g.dist == 0).sum()) == 1 and np.bincount(g.dist).tolist() == list(G.SPHERES_222)
    # every move changes the distance by exactly one (parity), and some move goes down from every state but solved
    d_nbr = g.dist[g.nbr].astype(np.int16) - g.dist[:, None]
    assert (np.abs(d_nbr) == 1).all()
    assert ((d_nbr == -1).any(axis=1) == (g.dist > 0)).all()
    # a, a ^ 1 is the identity on the whole group
    for a in range(6):
        assert (g.nbr[g.nbr[:, a], a ^ 1] == np.arange(G.GROUP_222)).all(), a
    # the parent pointers of the search replay: state = parent moved by `move`
    for lv_prev, lv in zip(levels_222[:-1], levels_222[1:]):
        assert (g.nbr[g.ids(lv_prev.code)[lv.parent], lv.move] == g.ids(lv.code)).all(), lv.depth


def test_333_spheres_to_depth_7(levels_333):
    assert tuple(len(lv.states) for lv in levels_333) == G.SPHERES_333
    assert [int(lv.solved.sum()) for lv in levels_333] == [1] + [0] * 7
    for lv in levels_333[:-1]:
        assert ((lv.child_solved != 0) == lv.children_equal_solved).all(), lv.depth


def test_333_code_collisions_are_the_recorded_ones(levels_333, golden):
    """The 20-byte code is not injective on the 3x3x3: 93838 / 878854 / 8221382 distinct codes at d = 5, 6, 7.

    Cause, from one colliding pair at depth 5: the two states differ in eight corner stickers, every one of them on a corner slot whose
    hash (colours . [1, 2, 10]) is a row the reference's corner_pieceInds table leaves at zeros (it fills 24 of the 44 reachable hashes,
    py333.py:171-180), so both states read (piece 0, orientation 0) there and the rest of the code is equal.  The fixture recorded
    from the reference (tests/golden/tables_333.npz) has those zero rows: the reference does not distinguish the states either.
    Recorded behaviour (VERDICT a5), not a bug."""
    counts = tuple(G.count_distinct(G.pack_code(lv.code, 24)) for lv in levels_333)
    assert counts == G.CODES_333
    lv = levels_333[5]
    order, first = G._sorted_groups(G.pack_code(lv.code, 24))
    j = int(np.flatnonzero(~first)[0])
    a, b = lv.states[order[j - 1]], lv.states[order[j]]
    assert (a != b).any() and (lv.code[order[j - 1]] == lv.code[order[j]]).all()
    t = golden("tables_333")
    cdefs, clut = t["corner_pieceDefs"].astype(np.int64), t["corner_pieceInds"].astype(np.int64)
    edefs = t["edge_pieceDefs"].astype(np.int64)
    differ = np.flatnonzero(a != b)
    slots = [s for s in range(8) if np.isin(cdefs[s], differ).any()]
    assert slots and np.isin(differ, cdefs[slots]).all() and not np.isin(differ, edefs).any()     # only corner stickers differ
    for s in slots:
        ha, hb = int(a[cdefs[s]] @ [1, 2, 10]), int(b[cdefs[s]] @ [1, 2, 10])
        assert not clut[ha].any() and not clut[hb].any(), (s, ha, hb)                              # unfilled rows of the reference's table
        assert lv.code[order[j]][s] == 0
    filled = np.flatnonzero(clut.any(axis=1))
    # 24 entries written; (piece 0, orientation 0) among them is itself all zeros, so 23 rows are visibly filled, all different
    assert len(filled) == 23 and len(np.unique(clut[filled], axis=0)) == 23


@pytest.mark.parametrize("cs", [3, 2])
def test_word_orders_commuting_faces_and_inverses(oracle, cs):
    """Every word of group_ref.WORD_ORDERS returns every start state first at exactly its order; U/D, R/L, F/B commute on the 3x3x3;
    a then a ^ 1 is the identity.  Start states: solved, the ball of radius 2 and 512 depth-30 scrambles."""
    A = G.N_ACTIONS[cs]
    rng = np.random.default_rng(cs)
    scr = oracle.solved(cs, 512)
    for _ in range(30):
        scr = oracle.step(cs, scr, rng.integers(0, A, len(scr), dtype=np.uint8))[0]
    ball = np.concatenate([lv.states for lv in G.oracle_bfs(oracle, cs, 2)])
    start = np.concatenate([ball, scr])
    n = len(start)
    counts = np.stack([(start == c).sum(axis=1) for c in range(6)])
    for word, acts, order in G.words_for(cs):
        st = start
        for k in range(1, order + 1):
            for a in acts:
                st = oracle.step(cs, st, np.full(n, a, np.uint8))[0]
            same = (st == start).all(axis=1)
            assert same.all() if k == order else not same.any(), (word, k)
        assert (np.stack([(st == c).sum(axis=1) for c in range(6)]) == counts).all()
    move = lambda s, name: oracle.step(cs, s, np.full(n, G.ACTION_NAMES[cs].index(name), np.uint8))[0]
    if cs == 3:
        for x, y in G.COMMUTING_333:
            assert (move(move(start, x), y) == move(move(start, y), x)).all(), (x, y)
            assert (move(move(start, x), y + "'") == move(move(start, y + "'"), x)).all(), (x, y)
    assert not (move(move(start, "U"), "R") == move(move(start, "R"), "U")).all(axis=1).any()       # adjacent faces never commute
    for a in range(A):
        mid = oracle.step(cs, start, np.full(n, a, np.uint8))[0]
        assert not (mid == start).all(axis=1).any()
        assert (oracle.step(cs, mid, np.full(n, a ^ 1, np.uint8))[0] == start).all(), a


def test_splitmix64_published_vector():
    st, out = G.SPLITMIX64_SEED, []
    for _ in range(5):
        st, z = G.splitmix64(st)
        out.append(z)
    assert tuple(out) == G.SPLITMIX64_VECTOR


@pytest.mark.parametrize("A", [12, 6])
@pytest.mark.parametrize("triple", G.RNG_TRIPLES)
def test_rng_restatement_equals_oracle(oracle, triple, A):
    """DESIGN.md section 5 on Python big ints gives the oracle's action stream (so the C restatement has no 64-bit slip: shifts,
    wrap-around, the hi32 multiply), also for seeds / streams / walks beyond 2^32 and 2^63."""
    seed, stream, walk = triple
    got = oracle.rng_actions(seed, stream, walk, 200, A)
    assert (got == G.rng_actions(seed, stream, walk, 200, A)).all()
    assert int(got.max()) < A and len(np.unique(got)) == A
