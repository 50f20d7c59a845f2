"""The rcc_* section of librubikhip.so without a GPU: header <-> exports <-> CUBIE_SIGNATURES, the untouched rc_* surface and build
id, the numpy restatement of the rule (tests/cubie_ref.py) on oracle walks, every status bit alone, the count of legal 2x2x2
assemblies, the package's own numpy rule (tables.get_cubies) and tables against the restatement, and the argument errors that come
before any device use.  Everything is integer-exact."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from rubiks_cube_solver_amd import _build, _cubie_lib, _lib, _native, tables
from tests import cubie_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUBE_SIZES = (3, 2)


def prototypes(header, prefix):
    """{function: number of parameters} of every `prefix`* prototype of a public header, comments stripped, (void) = 0."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    found = re.findall(r"^(?:int|int64_t|const char \*|void)\s*(" + prefix + r"\w+)\(([^)]*)\)", text, re.M)
    return {fn: 0 if args.strip() in ("", "void") else args.count(",") + 1 for fn, args in found}


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in nm.splitlines() if " T " in l}


@pytest.fixture(scope="module")
def walked(oracle):
    """{cs: [30 + 1, 64, S]}: 64 walks of 30 oracle moves from solved, every step kept."""
    out = {}
    for cs in CUBE_SIZES:
        rng = np.random.default_rng(40 + cs)
        st, steps = oracle.solved(cs, 64), []
        steps.append(st)
        for _ in range(30):
            st = oracle.step(cs, st, rng.integers(0, R.A_OF[cs], 64).astype(np.uint8))[0]
            steps.append(st)
        out[cs] = np.stack(steps)
        out[cs].setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------ ABI and build
def test_header_exports_and_signature_table_agree():
    protos = prototypes("rubikhip.h", "rcc_")
    assert protos == {"rcc_cubies": 10, "rcc_from_cubies": 8, "rcc_tables": 5}
    L = _cubie_lib.cubie_lib()                                              # loads without a GPU
    assert L is _lib.lib()                                                  # the same loaded library, not a second one
    names = exported(_lib.LIB_PATH)
    assert {e for e in names if e.startswith("rcc_")} == set(protos) == set(_cubie_lib.CUBIE_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_cubie_lib.CUBIE_SIGNATURES[fn])[0]) == n_params, fn
    # the rc_* surface is still the 38 of the header, and the two tables do not overlap
    rc = prototypes("rubikhip.h", "rc_")
    assert len(rc) == 38 and {e for e in names if e.startswith("rc_")} == set(rc) == set(_lib.SIGNATURES)
    assert not set(_lib.SIGNATURES) & set(_cubie_lib.CUBIE_SIGNATURES)
    # no new library: the build id is the hash of the source list, the section's own file (csrc/rc_cubies.h) included
    assert list(_build.LIBRARIES) == ["hip", "tree", "search", "net"]
    src = [os.path.basename(p) for p in _build.LIBRARIES["hip"].sources]
    assert src == ["rubikhip.hip", "rc_host.h", "rc_device.h", "rc_tables.h", "rc_table.h", "rc_cubies.h", "rc_edge.h", "rc_chain.h", "rc_ida.h", "rc_episode.h",
                   "rubikhip.h", "rubikepisode.h"]
    assert _lib.build_id() == _build.source_hash(_build.LIBRARIES["hip"].sources) == _build.embedded_id(_lib.LIB_PATH)


def test_generated_tables_are_current_and_constants_are_exported():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tables.py"), "--check"]).returncode == 0
    import rubiks_cube_solver_amd as pkg
    header = open(os.path.join(ROOT, "include", "rubikhip.h")).read()
    for name, bit in (("RCC_BAD_COLOUR", 1), ("RCC_BAD_FIXED", 2), ("RCC_BAD_PIECE", 4), ("RCC_DUP_PIECE", 8), ("RCC_TWIST", 16), ("RCC_FLIP", 32),
                      ("RCC_PARITY", 64)):
        assert getattr(pkg, name) == bit == getattr(tables, name) and pkg.RCC_NAMES[bit] == name
        assert re.search(r"#define " + name + r" " + str(bit) + r"u\b", header), name
    assert (R.BAD_COLOUR, R.BAD_FIXED, R.BAD_PIECE, R.DUP_PIECE, R.TWIST, R.FLIP, R.PARITY) == (1, 2, 4, 8, 16, 32, 64)


@pytest.mark.parametrize("cs", CUBE_SIZES)
def test_library_tables_and_package_tables_are_the_geometrys(cs):
    """rcc_tables (the generated header, through the library) = tables.get_cubies = the restatement's own derivation."""
    rule, mine, theirs = R.rule(cs), tables.get_cubies(cs), _cubie_lib.tables(cs)
    for got in (mine.corner_cw, theirs["corner_cw"]):
        assert (got == rule.corner).all()
    for got in (mine.corner_colours, theirs["corner_colours"]):
        assert (got == rule.ccol).all()
    assert (mine.edge_facelets == rule.edge).all() and (theirs["edge_facelets"] == rule.edge).all()
    assert (mine.edge_colours == rule.ecol).all() and (theirs["edge_colours"] == rule.ecol).all()
    assert sorted(mine.fixed.tolist()) == sorted(rule.fixed.tolist())
    # the handedness is the geometry's, not the listing's: the slots listed counter-clockwise have their last two stickers swapped --
    # all but DFR on the 3x3x3 (the listing mixes handedness), all seven on the 2x2x2 (its sixth slot is listed DRF)
    listed = tables.get_tables(cs).corner_defs
    swapped = [bool((a != b).any()) for a, b in zip(listed, rule.corner)]
    assert swapped == ([True] * 6 + [False, True] if cs == 3 else [True] * 7)


# ------------------------------------------------------------------------------------------- the restatement on oracle walks
@pytest.mark.parametrize("cs", CUBE_SIZES)
def test_solved_and_walks(oracle, walked, cs):
    rule = R.rule(cs)
    cub, status, cidx, eidx = R.cubies(cs, oracle.solved(cs, 1))
    assert cub[0].tolist() == [3 * q for q in range(rule.nc)] + [2 * q for q in range(rule.ne)]
    assert status[0] == 0 and cidx[0] == 0 and (eidx is None) == (cs == 2) and (cs == 2 or eidx[0] == 0)
    flat = walked[cs].reshape(-1, R.S_OF[cs])
    cub, status, cidx, eidx = R.cubies(cs, flat)
    assert (status == 0).all()
    cp, co = cub[:, :rule.nc] // 3, cub[:, :rule.nc] % 3
    assert (np.sort(cp, axis=1) == np.arange(rule.nc)).all() and (co.sum(axis=1) % 3 == 0).all()
    assert (cidx < (88179840 if cs == 3 else 3674160)).all()
    if cs == 3:
        ep, eo = cub[:, 8:] // 2, cub[:, 8:] % 2
        assert (np.sort(ep, axis=1) == np.arange(12)).all() and (eo.sum(axis=1) % 2 == 0).all()
        assert (R._sign(cp.astype(np.int64)) == R._sign(ep.astype(np.int64))).all()
        assert (eidx < 479001600 * 2048).all()
        # the edge byte IS RC_FMT_CODE's: the oracle's own code rows
        code = oracle.encode(cs, flat)[0][:, 8:]
        assert (cub[:, 8:] == code).all()
    # distinct states have distinct indices, equal states equal ones
    key = cidx.astype(np.uint64) if cs == 2 else np.stack([cidx.astype(np.uint64), eidx], axis=1)
    assert len(np.unique(key, axis=0)) == len(np.unique(flat, axis=0))
    # round trips
    back, bad = R.from_cubies(cs, cub)
    assert not bad.any() and (back == flat).all()
    # the package's numpy rule says the same
    mine = tables.get_cubies(cs).cubies(flat)
    assert (mine[0] == cub).all() and (mine[1] == status).all() and (mine[2] == cidx).all() and (cs == 2 or (mine[3] == eidx).all())


@pytest.mark.parametrize("cs", CUBE_SIZES)
def test_random_well_formed_cubies_round_trip(cs):
    """cubies(from_cubies(c)) == c for any permutation of the pieces with any orientations, legal or not; both rules agree on them."""
    rule, rng = R.rule(cs), np.random.default_rng(7)
    n = 500
    c = np.concatenate([np.stack([rng.permutation(rule.nc) for _ in range(n)]) * 3 + rng.integers(0, 3, (n, rule.nc)),
                        (np.stack([rng.permutation(rule.ne) for _ in range(n)]) * 2 + rng.integers(0, 2, (n, rule.ne))).reshape(n, rule.ne)],
                       axis=1).astype(np.uint8)
    st, bad = R.from_cubies(cs, c)
    assert not bad.any()
    cub, status, cidx, eidx = R.cubies(cs, st)
    assert (cub == c).all() and (status & 15 == 0).all() and ((status == 0) == (cidx != 0xFFFFFFFF)).all()
    assert 0 < (status == 0).sum() < n                                       # about one in 12 | 3 is legal
    mine = tables.get_cubies(cs)
    assert (mine.from_cubies(c)[0] == st).all()
    got = mine.cubies(st)
    assert (got[0] == cub).all() and (got[1] == status).all() and (got[2] == cidx).all() and (cs == 2 or (got[3] == eidx).all())


# ------------------------------------------------------------------------------------------------------ every bit fires alone
@pytest.mark.parametrize("cs", CUBE_SIZES)
def test_every_high_bit_fires_alone_and_is_invariant(oracle, walked, cs):
    start = walked[cs][30][:16]
    cub = R.cubies(cs, start)[0]
    rng = np.random.default_rng(3)
    for t, f, p in R.classes(cs):
        st, bad = R.from_cubies(cs, R.mutate(cs, cub, t, f, p))
        assert not bad.any()
        want = R.class_status(t, f, p)
        assert (want == 0) == ((t, f, p) == (0, 0, 0))
        for _ in range(21):                                                   # the state itself, then 20 further oracle moves
            status = R.cubies(cs, st)[1]
            assert (status == want).all(), (t, f, p, np.unique(status))
            assert (tables.get_cubies(cs).cubies(st)[1] == want).all()
            st = oracle.step(cs, st, rng.integers(0, R.A_OF[cs], len(st)).astype(np.uint8))[0]


@pytest.mark.parametrize("cs", CUBE_SIZES)
def test_every_low_bit_has_a_case(walked, cs):
    state = np.array(walked[cs][30][5])
    want = {R.BAD_COLOUR: R.BAD_COLOUR | R.BAD_PIECE, R.BAD_FIXED: R.BAD_FIXED, R.BAD_PIECE: R.BAD_PIECE, R.DUP_PIECE: R.DUP_PIECE}
    for bit, s in R.low_bit_cases(cs, state):
        for status, cidx in (R.cubies(cs, s[None])[1:3], tables.get_cubies(cs).cubies(s[None])[1:3]):
            assert status[0] == want[bit] and status[0] & 0x70 == 0 and cidx[0] == 0xFFFFFFFF, (bit, status)
    # a high-bit mutation on top of a low-bit defect stays silent: bits 16..64 are evaluated only when bits 1..8 are clear
    cub = R.mutate(cs, R.cubies(cs, state[None])[0], 1, cs == 3, cs == 3)
    s = R.from_cubies(cs, cub)[0][0]
    s[R.rule(cs).fixed[0]] ^= 1
    assert R.cubies(cs, s[None])[1][0] == R.BAD_FIXED == tables.get_cubies(cs).cubies(s[None])[1][0]


# --------------------------------------------------------------------------------------------------------------------- counting
def test_the_legal_222_assemblies_are_the_group():
    """Of all 7! * 3^7 = 11 022 480 assemblies of the 2x2x2 exactly 3 674 160 are legal -- the group order tests/test_group_host.py finds
    by search -- and their corner_index values are exactly 0 .. 3 674 159, each once."""
    import itertools
    perms = np.array(list(itertools.permutations(range(7))), np.uint8)                      # [5040, 7]
    oris = np.array(list(itertools.product(range(3), repeat=7)), np.uint8)                  # [2187, 7]
    seen = np.zeros(3674160, np.uint8)
    legal = total = 0
    for chunk in np.array_split(perms, 40):
        c = (chunk[:, None, :] * 3 + oris[None, :, :]).reshape(-1, 7)
        st, bad = R.from_cubies(2, c)
        cub, status, cidx, _ = R.cubies(2, st)
        assert not bad.any() and (cub == c).all() and (status & ~np.uint8(R.TWIST) == 0).all()
        ok = status == 0
        assert (cidx[~ok] == 0xFFFFFFFF).all()
        np.add.at(seen, cidx[ok], 1)
        legal, total = legal + int(ok.sum()), total + len(c)
    assert total == 11022480 and legal == 3674160 and (seen == 1).all()


# -------------------------------------------------------------------------------------------------------------- argument errors
def test_python_argument_errors_come_before_any_device_use():
    import torch
    from rubiks_cube_solver_amd import ops
    from rubiks_cube_solver_amd.vec_env import VecCubeEnv
    st = torch.zeros((1, 54, 16), dtype=torch.uint8)                          # a host tensor: no device is ever touched
    with pytest.raises(_lib.RubikHipError, match="HIP tensor"):
        ops.cubies(st, 4, 3)
    with pytest.raises(_lib.RubikHipError, match="HIP tensor"):
        ops.from_cubies(torch.zeros((1, 20, 16), dtype=torch.uint8), 4, 3)
    with pytest.raises(NotImplementedError):
        ops.cubies(st, 4, 4)
    with pytest.raises(NotImplementedError):
        _cubie_lib.tables(4)
    env = object.__new__(VecCubeEnv)                                          # an env cannot be built without a device
    env.num_envs, env.cube_size, env.stickers = 4, 3, st
    with pytest.raises(ValueError, match=r"\[4, 54\]"):
        env.set_sim_cube(np.zeros((3, 54), np.uint8), check=True)
    with pytest.raises(ValueError, match="cubies must be"):
        env.from_cubies(np.zeros((4, 7), np.uint8))
    assert tables.rcc_status_names(16 | 64) == ["RCC_TWIST", "RCC_PARITY"]
