"""The layout case table (tests/layout_cases.py) has teeth.  No GPU.

  address rule  the header's st[(n / pitch) * R * pitch + s * pitch + n % pitch], restated as a plain loop, is what ops.from_aos /
                ops.to_aos implement for every layout and size of the table and every row count (state, code, family)
  teeth         states scattered under layout X and gathered under layout Y differ from the original, for every ordered pair of
                distinct layouts and every size: a kernel that used one operand's tiling for another cannot pass the device matrix
  coverage      the generators yield every ordered pair / triple, variant and mode the device matrix is meant to run
"""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layout_cases as C  # noqa: E402

ROWS = sorted({*C.S_OF.values(), *C.SL_OF.values(), *C.NF_OF.values()})        # 7, 15, 20, 24, 51, 54


def rule_index(n, rows, pitch):
    """flat index of every (cube, row), one at a time"""
    idx = np.empty((n, rows), np.int64)
    for c in range(n):
        for r in range(rows):
            idx[c, r] = (c // pitch) * rows * pitch + r * pitch + c % pitch
    return idx


def test_layout_table():
    assert C.LAYOUTS == ("tight", "padded", "t512", "t1024") and C.SIZES == (513, 1029, 2565) and set(C.CUBE_SIZES) == {2, 3}
    for n in C.SIZES:
        assert n % 512 in (1, 5) and n // 512 >= 1                               # whole wave spans + a ragged tail of 1 or 5
        C.check_premise(n, *C.LAYOUTS)
        assert C.layout("tight", n) == (C.ceil16(n), 1) and C.layout("padded", n) == (C.ceil16(n) + 48, 1)
        assert C.layout("t512", n) == (512, -(-n // 512)) and C.layout("t1024", n) == (1024, -(-n // 1024))
        assert C.all_differ(n, *C.POLICY_TRIPLE) and len(set(C.POLICY_TRIPLE)) == 3
    assert not C.EXCLUDED


@pytest.mark.parametrize("n", C.SIZES)
def test_address_rule_is_from_aos_and_to_aos(n):
    from rubiks_cube_solver_amd import ops
    rng = np.random.default_rng(n)
    for rows in ROWS:
        aos = rng.integers(0, 250, (n, rows), dtype=np.uint8)
        for name in C.LAYOUTS:
            pitch, tiles = C.layout(name, n)
            idx = rule_index(n, rows, pitch)
            assert idx.max() < tiles * rows * pitch and len(np.unique(idx)) == n * rows
            buf = ops.from_aos(aos, "cpu", pitch)
            assert tuple(buf.shape) == C.shape(name, n, rows)
            flat = buf.numpy().reshape(-1)
            assert (flat[idx] == aos).all(), (rows, name)
            assert int(flat.astype(np.int64).sum()) == int(aos.astype(np.int64).sum())      # the pad columns are zero
            assert (ops.to_aos(buf, n).numpy() == aos).all()
            raw = torch.zeros(C.shape(name, n, rows), dtype=torch.uint8)                    # to_aos alone, from bytes placed by the rule
            raw.view(-1)[torch.from_numpy(idx.reshape(-1))] = torch.from_numpy(aos.reshape(-1))
            assert (ops.to_aos(raw, n).numpy() == aos).all()
            assert C.gather(C.scatter(aos[:3].tolist(), pitch, tiles), 3, rows, pitch) == aos[:3].tolist()   # the table's own helpers


@pytest.mark.parametrize("cs", C.CUBE_SIZES)
@pytest.mark.parametrize("n", C.SIZES)
def test_teeth(oracle, cs, n):
    """Scatter under X, gather under Y: at least one cube < n comes back different (in fact most do), for the state rows and the code
    rows of the oracle's random walks."""
    rng = np.random.default_rng(n + cs)
    acts = rng.integers(0, C.A_OF[cs], (n, 17), dtype=np.uint8)
    states = oracle.adi(cs, n, 17, actions_in=acts, want_children=False)["parents"][:, -1]
    codes = oracle.encode(cs, states)[0]
    for aos in (states, codes):
        rows = aos.shape[1]
        size = max(C.nbytes(x, n, rows) for x in C.LAYOUTS)
        for x, y in itertools.permutations(C.LAYOUTS, 2):
            if n in C.EXCLUDED.get((x, y), ()):
                continue
            px, py = C.layout(x, n)[0], C.layout(y, n)[0]
            flat = np.zeros(size, np.uint8)
            flat[_fast_index(n, rows, px)] = aos
            back = flat[_fast_index(n, rows, py)]
            wrong = (back != aos).any(1)
            assert wrong.any(), (x, y, n, rows)
            assert wrong.mean() > 0.5, (x, y, n, rows, wrong.mean())             # not a corner case: most cubes are wrong


def _fast_index(n, rows, pitch):
    c, r = np.arange(n)[:, None], np.arange(rows)[None, :]
    return C.address(c, r, pitch, rows)


def test_fast_index_is_the_rule():
    for n, rows, pitch in ((513, 7, 512), (1029, 20, 1040), (1029, 24, 1024)):
        assert (_fast_index(n, rows, pitch) == rule_index(n, rows, pitch)).all()


def test_generators_cover_the_matrix():
    """Every ordered pair / triple the matrix names is there, per entry point: pruning a generator fails here."""
    L4 = C.LAYOUTS
    triples, pairs = set(itertools.product(L4, L4, L4)), set(itertools.product(L4, L4))
    step = C.step_code_cases()
    for pack in (1, 2):
        assert {(a, b, c) for a, b, c, v, ip in step if v == pack and not ip} == triples
        assert {(a, c) for a, b, c, v, ip in step if v == pack and ip} == {(a, c) for a, c in pairs if a != c}
        assert all(a == b for a, b, c, v, ip in step if ip)
        for pol in (1, 2, 3, 4):
            hit = [(a, b, c) for a, b, c, v, ip in step if v == pol * 10 + pack]
            assert hit and all(len({a, b, c}) == 3 for a, b, c in hit)
    assert len(step) == 2 * (64 + 12 + 4)
    dense = C.step_dense_cases()
    for tile in (1, 2):
        assert {(a, b) for a, b, v in dense if v == tile * 100000} == pairs
    assert C.DENSE == ("U8", "F16", "BF16", "F32")
    assert C.WORKSPACE_CASE == dict(cs=3, fmt="BF16", n=(1 << 17) + 5, lin="t512", lout="tight")
    enc = C.encode_cases()
    assert {(a, b) for a, b in enc if b in L4} == pairs
    assert {(a, b) for a, b in enc if b in C.DENSE} == set(itertools.product(L4, C.DENSE))
    assert {a for a, b in enc if b == "flags"} == set(L4) and len(enc) == 16 + 16 + 4
    exp = C.expand_cases()
    for pack in (1, 2):
        for parts in (1, 3, "A"):
            for outputs in ("all", "flags"):
                assert {(a, b) for a, b, v, p, o in exp if v == pack + 800 and p == parts and o == outputs} == pairs
    for pack in (0, 2):
        assert {(a, b) for a, b, v, p, o in exp if v == pack + 100 and p is None and o == "stickers"} == pairs
    assert C.expand_variant(801, "A", 12) == 12801 and C.expand_variant(802, 3, 6) == 3802 and C.expand_variant(100, None, 6) == 100
    c2d = C.code_to_dense_cases()
    want = {100000, 200000, 300000, 400000} | {400000 + f + 10 * t for f in (1, 2, 4) for t in (2, 3, 4)}
    for name in L4:
        assert want <= {v for lc, v in c2d if lc == name}
    for n in C.SIZES:
        scr = C.scramble_cases(n)
        assert set(scr) == set(itertools.product(L4, (C.ceil16(n), C.ceil16(n) + 32), ("replay", "drawn", "copy"), (False, True)))
    offs = C.carve_offsets(8)
    assert offs[:3] == [16, 48, 80] and all(o % 32 == 16 for o in offs) and len({o % 256 for o in offs}) == 8
