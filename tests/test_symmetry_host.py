"""The cube symmetries without a GPU: tables.get_symmetries against the numpy restatement (tests/sym_ref.py) and against the group
itself (oracle moves), the generated header and the library's own tables, and the three-way ABI check of the rcs_* extension of
librubiksearch.so (header <-> exports <-> SYM_SIGNATURES).  Every comparison is exact."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import group_ref as G
from tests import sym_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBES = (3, 2)


def sym(cs):
    from rubiks_cube_solver_amd.tables import get_symmetries
    return get_symmetries(cs)


def walk(oracle, cs, depth, seed):
    """[depth + 1, S]: the states along one random walk from solved, by the oracle's moves."""
    rng = np.random.default_rng(seed)
    st, out = oracle.solved(cs, 1), []
    out.append(st[0])
    for a in rng.integers(0, G.N_ACTIONS[cs], depth):
        st = oracle.step(cs, st, np.array([a], np.uint8))[0]
        out.append(st[0])
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("cs", CUBES)
def test_count_order_and_restatement(cs):
    y, r = sym(cs), R.build(cs)
    K, S, A = R.N_SYM[cs], G.N_STICKERS[cs], G.N_ACTIONS[cs]
    assert y.count == r.K == K
    assert y.perm.shape == (K, S) and y.relabel.shape == (K, 6) and y.amap.shape == (K, A + 1) and y.compose.shape == (K, K)
    assert (y.perm[0] == np.arange(S)).all() and (y.relabel[0] == np.arange(6)).all() and (y.amap[0] == np.arange(A + 1)).all()
    assert y.det.tolist() == [1] * (K // 2) + [-1] * (K // 2)                 # rotations first
    for name in ("perm", "relabel", "amap", "det", "inverse", "compose"):
        assert (getattr(y, name) == getattr(r, name)).all(), name
    for s in range(K):                                                       # every perm is a permutation, every relabel one of the faces
        assert sorted(y.perm[s]) == list(range(S)) and sorted(y.relabel[s]) == list(range(6))


@pytest.mark.parametrize("cs", CUBES)
def test_solved_is_fixed_and_amap_permutes_the_actions(oracle, cs):
    y = sym(cs)
    A = G.N_ACTIONS[cs]
    solved = oracle.solved(cs, 1)
    for s in range(y.count):
        assert (y.apply(solved, s) == solved).all(), s
        assert sorted(y.amap[s][:A]) == list(range(A)) and y.amap[s][A] == A, s
        assert ((y.amap[s][:A] ^ 1) == y.amap[s][np.arange(A) ^ 1]).all(), s    # a turn's inverse maps to the image's inverse


@pytest.mark.parametrize("cs", CUBES)
def test_equivariance_along_walks_with_oracle_moves(oracle, cs):
    """T_s(move_a(x)) == move_{amap[s][a]}(T_s(x)) for every s and every a at every state of 40-move walks."""
    y = sym(cs)
    A = G.N_ACTIONS[cs]
    x = np.concatenate([walk(oracle, cs, 40, seed) for seed in (1, 2)])      # [82, S]
    n = len(x)
    for a in range(A):
        moved = oracle.step(cs, x, np.full(n, a, np.uint8))[0]
        for s in range(y.count):
            right = oracle.step(cs, y.apply(x, s), np.full(n, y.amap[s][a], np.uint8))[0]
            assert (y.apply(moved, s) == right).all(), (s, a)


@pytest.mark.parametrize("cs", CUBES)
def test_compose_inverse_and_distinct_images(oracle, cs):
    y = sym(cs)
    K = y.count
    x = walk(oracle, cs, 25, 7)[-1:]
    images = np.stack([y.apply(x, s)[0] for s in range(K)])
    assert len({r.tobytes() for r in images}) == K                           # a scrambled state has K distinct images
    for s in range(K):
        for u in range(K):
            got = y.perm[s][y.perm[u]]                                        # apply s, then u: the gathers composed ...
            assert (got == y.perm[y.compose[s][u]]).all() and (y.relabel[u][y.relabel[s]] == y.relabel[y.compose[s][u]]).all(), (s, u)
            assert (y.apply(y.apply(x, s), u) == y.apply(x, y.compose[s][u])).all(), (s, u)
        assert y.compose[s][y.inverse[s]] == 0 and y.compose[y.inverse[s]][s] == 0, s
    assert sorted(y.inverse) == list(range(K))
    for s in range(K):                                                       # closed: every row and column of the table is a permutation
        assert sorted(y.compose[s]) == list(range(K)) and sorted(y.compose[:, s]) == list(range(K))


def test_222_is_the_corner_restriction_of_the_matching_333_symmetries():
    """Each 2x2x2 symmetry is the 3x3x3 one with the same matrix, read on the corner stickers."""
    y2, y3 = sym(2), sym(3)
    corner3 = np.array([f * 9 + k for f in range(6) for k in (0, 2, 6, 8)])   # corner stickers of the 3x3x3 in 2x2x2 numbering order
    where = {int(c): i for i, c in enumerate(corner3)}
    for s2 in range(y2.count):
        hits = [s3 for s3 in range(y3.count) if (y3.matrix[s3] == y2.matrix[s2]).all()]
        assert len(hits) == 1
        s3 = hits[0]
        assert (y3.relabel[s3] == y2.relabel[s2]).all() and y3.det[s3] == y2.det[s2]
        assert [where[int(y3.perm[s3][c])] for c in corner3] == y2.perm[s2].tolist()
        for a, name in enumerate(G.ACTION_NAMES[2]):                          # and the move relabelling agrees on U, F, R
            assert G.ACTION_NAMES[3][y3.amap[s3][G.ACTION_NAMES[3].index(name)]] == G.ACTION_NAMES[2][y2.amap[s2][a]]


@pytest.mark.parametrize("cs", CUBES)
def test_reference_canonical_form(oracle, cs):
    """sym_ref's own canonical form: constant on an orbit, never above an image, the lowest minimiser; the solved cube's is 0."""
    K = R.N_SYM[cs]
    x = walk(oracle, cs, 12, 3)
    s0, img0 = R.canonical(cs, x)
    assert s0[0] == 0 and (img0[0] == x[0]).all()
    for t in range(K):
        st, img = R.canonical(cs, R.apply(cs, x, t))
        assert (img == img0).all()
    im = R.all_images(cs, x)
    for c in range(len(x)):
        rows = [im[s, c].tobytes() for s in range(K)]
        assert img0[c].tobytes() == min(rows) and rows.index(min(rows)) == s0[c]


# ------------------------------------------------------------------------------------- generated header, library tables
def test_generated_symmetry_header_is_current():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_tables
    finally:
        sys.path.pop(0)
    assert open(gen_tables.OUT_SYM).read() == gen_tables.render_sym()
    assert open(gen_tables.OUT).read() == gen_tables.render()                 # rc_tables.h is untouched by the new generator
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tables.py"), "--check"]).returncode == 0


@pytest.mark.parametrize("cs", CUBES)
def test_library_tables_are_the_packages(cs):
    """rcs_sym_count / rcs_sym_tables: host-only exports, the library loads and answers without a GPU."""
    from rubiks_cube_solver_amd import _sym_lib
    y = sym(cs)
    assert _sym_lib.count(cs) == y.count
    got = _sym_lib.tables(cs)
    assert set(got) == {"perm", "relabel", "amap", "inverse", "compose"}
    for name, arr in got.items():
        assert arr.dtype == np.uint8 and (arr == getattr(y, name)).all(), name
    L = _sym_lib.sym_lib()
    assert L.rcs_sym_count(4) == -1
    assert L.rcs_sym_tables(cs, None, None, None, None, None) == 0             # any pointer may be NULL
    assert L.rcs_sym_tables(5, None, None, None, None, None) == -1 and b"cube_size" in L.rc_search_last_error()


# ------------------------------------------------------------------------------------------------------------------ ABI
def prototypes(header, prefix):
    """{function: number of parameters} of every `prefix`* prototype of a public header, comments stripped, (void) = 0."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    found = re.findall(r"^(?:int|int64_t|const char \*|void)\s*(" + prefix + r"\w+)\(([^)]*)\)", text, re.M)
    return {fn: 0 if args.strip() in ("", "void") else args.count(",") + 1 for fn, args in found}


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in nm.splitlines() if " T " in l}


def test_header_exports_and_signature_table_agree():
    from rubiks_cube_solver_amd import _build, _native, _search_lib, _sym_lib
    protos = prototypes("rubiksym.h", "rcs_")
    assert protos == {"rcs_sym_count": 1, "rcs_sym_tables": 6, "rcs_sym_apply": 10, "rcs_sym_canonical": 8}
    assert prototypes("rubiksym.h", "rc_") == {}                             # the extension declares nothing under the frozen prefix
    L = _sym_lib.sym_lib()                                                   # loads without a GPU
    assert L is _search_lib.search_lib()                                     # the same loaded library, not a second one
    names = exported(_search_lib.LIB_PATH)
    assert {e for e in names if e.startswith("rcs_")} == set(protos) == set(_sym_lib.SYM_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_sym_lib.SYM_SIGNATURES[fn])[0]) == n_params, fn
    # the rc_search_* surface is its header's, unchanged, and the two signature tables do not overlap
    assert {e for e in names if e.startswith("rc_")} == set(prototypes("rubiksearch.h", "rc_")) == set(_search_lib.SIGNATURES)
    assert not set(_search_lib.SIGNATURES) & set(_sym_lib.SYM_SIGNATURES)
    # the new sources are part of the library's identity: before rubiksearch.h, the public header last
    src = [os.path.basename(p) for p in _build.LIBRARIES["search"].sources]
    assert src == ["rc_search.hip", "rc_host.h", "rc_device.h", "rc_tables.h", "rc_table.h", "rc_sym.h", "rc_sym_tables.h", "rubiksearch.h", "rubiksym.h"]
    assert _search_lib.build_id() == _build.source_hash(_build.LIBRARIES["search"].sources)
    without = [p for p in _build.LIBRARIES["search"].sources if os.path.basename(p) not in ("rc_sym.h", "rc_sym_tables.h", "rubiksym.h")]
    assert _build.source_hash(without) != _search_lib.build_id()
    # librubikhip.so does not see the new files: rc_tables.h and its source list are what they were
    assert [os.path.basename(p) for p in _build.LIBRARIES["hip"].sources] == ["rubikhip.hip", "rc_host.h", "rc_device.h", "rc_tables.h", "rc_table.h",
                                                                              "rc_cubies.h", "rc_edge.h", "rc_chain.h", "rc_ida.h", "rc_episode.h",
                                                                              "rubikhip.h", "rubikepisode.h"]


def test_python_argument_errors_come_before_any_device_use():
    from rubiks_cube_solver_amd import search
    assert search.symmetry_indices("rotations", 3) == list(range(24)) and search.symmetry_indices("all", 2) == list(range(6))
    assert search.symmetry_indices((0, 5, 24, 47), 3) == [0, 5, 24, 47]
    with pytest.raises(ValueError):
        search.symmetry_indices("reflections", 3)
    with pytest.raises(IndexError):
        search.symmetry_indices((0, 6), 2)
    with pytest.raises(IndexError):
        search.symmetry_indices((), 3)
