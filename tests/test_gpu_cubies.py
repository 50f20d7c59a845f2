"""The cubie kernels on the GPU (include/rubikhip.h rcc_cubies, rcc_from_cubies) and what is built on them (ops.cubies / from_cubies,
VecCubeEnv.cubies / legality / from_cubies / set_sim_cube(check=True)).

  a. against the numpy restatement (tests/cubie_ref.py): every cube count that opens another path, both cube sizes, every ordered pair
     of layouts, every operand carved 16 bytes past a 32-byte boundary, the bytes around every buffer, every subset of the outputs;
  b. the argument errors (RC_EINVAL, nothing written) and the *bad flag;
  c. by mathematics, on the device's own moves: whole spheres, all 11 022 480 assemblies of the 2x2x2, invariance under moves and symmetries;
  d. the Python surface.
Every comparison is exact."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from rubiks_cube_solver_amd import _cubie_lib, _lib, ops, tables
from tests import cubie_ref as R
from tests import layout_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = (1, 3, 513, 1029, 2565)
GUARD = 256                                          # bytes kept around every carved operand
FILL = 0xA5                                          # what pad columns and guards hold before a launch
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    _lib.init(torch.device(DEV, torch.cuda.current_device()))
    return _cubie_lib.cubie_lib()


def stream():
    return _lib.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


class Pool:
    """The shared inputs and references of one cube size, computed once: 2565 states -- oracle walks, every illegal class built from
    them, the four low-bit cases -- their cubies, status and indices by the restatement, and the restatement's states of those cubies."""

    def __init__(self, oracle, cs):
        n = max(COUNTS)
        walked = np.concatenate([R.walks(oracle, cs, 64, d, 50 + d) for d in (0, 1, 7, 30)])
        cub = R.cubies(cs, walked)[0]
        parts = [walked]
        for t, f, p in R.classes(cs)[1:]:                                   # 3x3x3: the eleven illegal classes
            parts.append(R.from_cubies(cs, R.mutate(cs, cub[64:128], t, f, p))[0])
        parts.append(np.stack([s for _, s in R.low_bit_cases(cs, walked[200])]))
        junk = walked[128:160].copy()                                        # arbitrary bytes, values 6..255 among them
        rng = np.random.default_rng(cs)
        hit = rng.random(junk.shape) < 0.1
        junk[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
        junk[:, 0] = np.array([6, 7, 8, 9, 10, 11, 12, 13, 0x10, 0x7F, 0x80, 0xFF] * 3, np.uint8)[:len(junk)]   # every kind of v_perm selector
        parts.append(junk)
        every = np.concatenate(parts)
        self.states = every[np.arange(n) % len(every)]
        self.cubies, self.status, self.cidx, self.eidx = R.cubies(cs, self.states)
        assert {int(s) for s in self.status} >= {R.class_status(*c) for c in R.classes(cs)} | {2, 4, 5, 8}
        self.cubies_in = self.cubies.copy()                                  # inputs of rcc_from_cubies: 0xFF slots would flag the cube
        self.cubies_in[self.cubies_in == R.NONE] = 0
        self.back, bad = R.from_cubies(cs, self.cubies_in)
        assert not bad.any()
        for a in (self.states, self.cubies, self.status, self.cidx, self.cubies_in, self.back):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def pools(oracle):
    return {cs: Pool(oracle, cs) for cs in LC.CUBE_SIZES}


# ------------------------------------------------------------------------------------------------- carved operands
def addresses(n, rows, pitch):
    """[n, rows] byte offsets of include/rubikhip.h's rule: (c / pitch) * rows * pitch + r * pitch + c % pitch."""
    c = np.arange(n)[:, None]
    return (c // pitch) * rows * pitch + np.arange(rows)[None, :] * pitch + c % pitch


class Arena:
    """One operand inside a larger allocation: GUARD bytes of FILL on both sides, the operand `offset` bytes past a 32-byte boundary.
    `host` is the expected content of the whole allocation; check() compares the device's bytes with it."""

    def __init__(self, nbytes, offset):
        self.start = GUARD + offset
        self.host = np.full(self.start + nbytes + GUARD, FILL, np.uint8)
        self.nbytes = nbytes

    def upload(self):
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 32 == 0
        self.view = self.dev[self.start:self.start + self.nbytes]
        return self

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def expect(self, values):
        """The operand is an array of len(values) elements from its first byte on."""
        raw = np.ascontiguousarray(values).view(np.uint8).reshape(-1)
        self.host[self.start:self.start + len(raw)] = raw

    def expect_rows(self, rows_aos, pitch):
        n, rows = rows_aos.shape
        self.host[self.start + addresses(n, rows, pitch)] = rows_aos

    def check(self, what):
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero(got != self.host)
        assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at operand offset {int(bad[0]) - self.start}"


def rows_arena(aos, n, rows, layout, offset):
    """A tiled operand in `layout`; aos [n, rows] is uploaded as its content (None: all FILL)."""
    pitch, tiles = LC.layout(layout, n)
    a = Arena(tiles * rows * pitch, offset)
    a.pitch = pitch
    if aos is not None:
        a.expect_rows(aos, pitch)
    return a


def run_cubies(lib, P, cs, n, lay_st, lay_c, offset, outputs=("cubies", "status", "corner", "edge")):
    """One rcc_cubies call on the pool's first n states with every operand in an arena of its own; checks every byte."""
    S, SL = LC.S_OF[cs], LC.SL_OF[cs]
    offs = LC.carve_offsets(5) if offset else [0] * 5
    st = rows_arena(P.states[:n], n, S, lay_st, offs[0]).upload()
    cub = rows_arena(None, n, SL, lay_c, offs[1]).upload()
    status, cidx, eidx = Arena(n, offs[2]).upload(), Arena(4 * n, offs[3]).upload(), Arena(8 * n, offs[4]).upload()
    want = {o for o in outputs if not (o == "edge" and cs == 2)}
    rc = lib.rcc_cubies(st.ptr(), n, st.pitch, cs, cub.ptr() if "cubies" in want else None, cub.pitch, status.ptr() if "status" in want else None,
                        cidx.ptr() if "corner" in want else None, eidx.ptr() if "edge" in want else None, stream())
    assert rc == 0, lib.rc_last_error()
    if "cubies" in want:
        cub.expect_rows(P.cubies[:n], cub.pitch)
    if "status" in want:
        status.expect(P.status[:n])
    if "corner" in want:
        cidx.expect(P.cidx[:n])
    if "edge" in want:
        eidx.expect(P.eidx[:n])
    for a, what in ((st, "st"), (cub, "cubies"), (status, "status"), (cidx, "corner_index"), (eidx, "edge_index")):
        a.check(f"rcc_cubies cs={cs} n={n} {lay_st}->{lay_c} +{offset} {sorted(want)}: {what}")


# ------------------------------------------------------------------------------------- a. against the restatement
@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_cubies_equal_the_restatement_in_every_layout_pair(lib, pools, cs, n, offset):
    for lay_st, lay_c in LC.PAIRS:
        run_cubies(lib, pools[cs], cs, n, lay_st, lay_c, offset)


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_from_cubies_equals_the_restatement_in_every_layout_pair(lib, pools, cs, n, offset):
    P, S, SL = pools[cs], LC.S_OF[cs], LC.SL_OF[cs]
    offs = LC.carve_offsets(3) if offset else [0] * 3
    for lay_c, lay_st in LC.PAIRS:
        cub = rows_arena(P.cubies_in[:n], n, SL, lay_c, offs[0]).upload()
        st = rows_arena(None, n, S, lay_st, offs[1]).upload()
        flag = Arena(16, offs[2])
        flag.host[flag.start] = 0
        flag.upload()
        assert lib.rcc_from_cubies(cub.ptr(), n, cub.pitch, cs, st.ptr(), st.pitch, flag.ptr(), stream()) == 0, lib.rc_last_error()
        st.expect_rows(P.back[:n], st.pitch)
        for a, what in ((cub, "cubies"), (st, "st"), (flag, "bad")):
            a.check(f"rcc_from_cubies cs={cs} n={n} {lay_c}->{lay_st} +{offset}: {what}")


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_every_subset_of_the_outputs_gives_the_same_bytes(lib, pools, cs):
    names = ("cubies", "status", "corner", "edge")[:4 if cs == 3 else 3]
    for k in range(1, len(names) + 1):
        for subset in itertools.combinations(names, k):
            for n in (3, 1029):
                run_cubies(lib, pools[cs], cs, n, "t512", "padded", 16, subset)


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_the_eight_cube_pack_and_the_streamed_rows(lib, pools, cs):
    """2^18 + 5 cubes: the size from which the 2x2x2 takes 8 cubes per lane, and (3x3x3, everything asked for) streams past the cache
    threshold are both beyond what the small cases run; the pool's states, repeated."""
    n = (1 << 18) + 5
    P = pools[cs]
    idx = np.arange(n) % len(P.states)
    st = ops.from_aos(P.states[idx], DEV)
    out = ops.cubies(st, n, cs, index=True)
    assert (ops.to_aos(out["cubies"], n).cpu().numpy() == P.cubies[idx]).all()
    assert (out["status"].cpu().numpy() == P.status[idx]).all()
    assert (out["corner_index"].cpu().numpy().view(np.uint32) == P.cidx[idx]).all()
    if cs == 3:
        assert (out["edge_index"].cpu().numpy().view(np.uint64) == P.eidx[idx]).all()
    back = ops.from_cubies(ops.from_aos(P.cubies_in[idx], DEV), n, cs)
    assert (ops.to_aos(back, n).cpu().numpy() == P.back[idx]).all()


# -------------------------------------------------------------------------------------------- b. argument errors, *bad
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_argument_errors_write_nothing(lib, pools, cs):
    P, S, SL, n = pools[cs], LC.S_OF[cs], LC.SL_OF[cs], 513
    st = rows_arena(P.states[:n], n, S, "tight", 0).upload()
    cub = rows_arena(P.cubies_in[:n], n, SL, "tight", 0).upload()
    status, cidx, eidx, flag = Arena(n + 16, 0).upload(), Arena(4 * n + 16, 0).upload(), Arena(8 * n + 16, 0).upload(), Arena(32, 0).upload()
    p = lambda a, off=0: ctypes.c_void_p(a.view.data_ptr() + off)
    e = eidx.ptr() if cs == 3 else None
    good = dict(st=st.ptr(), n=n, pitch=st.pitch, cs=cs, cubies=cub.ptr(), cpitch=cub.pitch, status=status.ptr(), cidx=cidx.ptr(), eidx=e)
    call = lambda **kw: (lambda a: lib.rcc_cubies(a["st"], a["n"], a["pitch"], a["cs"], a["cubies"], a["cpitch"], a["status"], a["cidx"], a["eidx"], stream()))({**good, **kw})
    cases = [("st", dict(st=None)), ("nothing to write", dict(cubies=None, status=None, cidx=None, eidx=None)), ("st", dict(st=p(st, 8))),
             ("cubies", dict(cubies=p(cub, 4))), ("status", dict(status=p(status, 8))), ("corner_index", dict(cidx=p(cidx, 4))),
             ("pitch", dict(pitch=st.pitch - 8)), ("pitch", dict(pitch=256)), ("cubie_pitch", dict(cpitch=cub.pitch + 8)), ("cubie_pitch", dict(cpitch=496)),
             ("cube_size", dict(cs=4)), ("n_cubes", dict(n=-1))]
    cases += [("edge_index", dict(eidx=p(eidx, 8)))] if cs == 3 else [("edge_index", dict(eidx=eidx.ptr()))]
    for word, kw in cases:
        assert call(**kw) == EINVAL, (word, kw)
        assert word in lib.rc_last_error().decode(), (word, lib.rc_last_error())
    good = dict(cubies=cub.ptr(), n=n, cpitch=cub.pitch, cs=cs, st=st.ptr(), pitch=st.pitch, bad=flag.ptr())
    call = lambda **kw: (lambda a: lib.rcc_from_cubies(a["cubies"], a["n"], a["cpitch"], a["cs"], a["st"], a["pitch"], a["bad"], stream()))({**good, **kw})
    for word, kw in [("cubies", dict(cubies=None)), ("cubies", dict(cubies=p(cub, 8))), ("st", dict(st=None)), ("st", dict(st=p(st, 4))), ("bad", dict(bad=None)),
                     ("pitch", dict(pitch=st.pitch + 4)), ("cubie_pitch", dict(cpitch=64)), ("cube_size", dict(cs=1)), ("n_cubes", dict(n=-5))]:
        assert call(**kw) == EINVAL, (word, kw)
        assert word in lib.rc_last_error().decode(), (word, lib.rc_last_error())
    assert call(n=0) == 0 and lib.rcc_cubies(st.ptr(), 0, st.pitch, cs, cub.ptr(), cub.pitch, None, None, None, stream()) == 0      # nothing to do: no launch
    for a, what in ((st, "st"), (cub, "cubies"), (status, "status"), (cidx, "corner_index"), (eidx, "edge_index"), (flag, "bad")):
        a.check(f"cs={cs}: {what} after the refused calls")


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_an_unnameable_byte_writes_solved_and_sets_bad(lib, pools, cs):
    P, S, SL, n = pools[cs], LC.S_OF[cs], LC.SL_OF[cs], 1029
    c = np.array(P.cubies_in[:n])
    hit = {5: (0, 3 * R.rule(cs).nc), 700: (SL - 1, 24), 1028: (2, 0xFF)}      # the first value no slot of that kind can hold; the last cube (ragged pack)
    for cube, (slot, value) in hit.items():
        c[cube, slot] = value
    want, bad = R.from_cubies(cs, c)
    assert sorted(np.flatnonzero(bad)) == sorted(hit) and (want[list(hit)] == R.rule(cs).solved).all()
    cub = rows_arena(c, n, SL, "t512", 16).upload()
    st = rows_arena(None, n, S, "padded", 48).upload()
    flag = Arena(16, 16)
    flag.host[flag.start] = 0
    flag.upload()
    assert lib.rcc_from_cubies(cub.ptr(), n, cub.pitch, cs, st.ptr(), st.pitch, flag.ptr(), stream()) == 0
    st.expect_rows(want, st.pitch)
    flag.host[flag.start] = 1
    for a in (cub, st, flag):
        a.check("unnameable byte")
    with pytest.raises(ValueError):
        ops.from_cubies(ops.from_aos(c, DEV), n, cs)
    # a pad column that names nothing is nobody's cube: no flag
    flag2 = torch.zeros(1, dtype=torch.uint8, device=DEV)
    buf = ops.from_aos(np.array(P.cubies_in[:n]), DEV, pitch=1040)
    buf[:, :, n:] = 0xFF
    ops.from_cubies(buf, n, cs, bad=flag2)
    assert int(flag2) == 0


# ------------------------------------------------------------------------- c. by mathematics on the device's own moves
def device_children(cs, states):
    """[n, S] -> [n, A, S]: rc_expand_children of every state."""
    n, A = len(states), LC.A_OF[cs]
    st = ops.from_aos(states, DEV)
    out = ops.expand_buffers(n, cs, DEV, st.shape[-1], children=True, codes=False)
    ops.expand_children(st, n, cs, out["children"], out["child_solved"], None, pitch=st.shape[-1])
    return np.stack([ops.to_aos(out["children"][a], n).cpu().numpy() for a in range(A)], axis=1)


def device_cubies(cs, states, index=True):
    n = len(states)
    out = ops.cubies(ops.from_aos(states, DEV), n, cs, index=index)
    host = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)
    return ops.to_aos(out["cubies"], n).cpu().numpy(), out["status"].cpu().numpy(), host(out["corner_index"], np.uint32), host(out["edge_index"], np.uint64)


def move_on_cubies(cs, cub, a):
    """The cubies of move_a(x) from the cubies of x: a face turn carries whole cubies, slot p receives the cubie of slot q turned by d,
    where (q, d) is what move_a(solved) shows in slot p (the restatement reads it off tables.py's permutation of the solved cube)."""
    rule, t = R.rule(cs), tables.get_tables(cs)
    moved = R.cubies(cs, t.solved[t.perm[a]][None])[0][0]
    out = np.empty_like(cub)
    for p in range(rule.nc + rule.ne):
        m = 3 if p < rule.nc else 2
        q, d = int(moved[p]) // m + (0 if p < rule.nc else rule.nc), int(moved[p]) % m
        out[:, p] = cub[:, q] // m * m + (cub[:, q] % m + d) % m
    return out


@pytest.mark.parametrize("cs,depth,count", [(3, 4, 11206), (2, 5, None)])
def test_whole_spheres(cs, depth, count):
    """Every state within `depth` moves of solved, driven by rc_expand_children: legal, distinct indices, and the cubies of every child
    are one move's image of its parent's."""
    A = LC.A_OF[cs]
    frontier = R.rule(cs).solved[None].copy()
    seen = frontier.copy()
    for _ in range(depth):
        kids = device_children(cs, frontier)
        pc = device_cubies(cs, frontier, index=False)[0]
        kc = device_cubies(cs, kids.reshape(-1, kids.shape[-1]), index=False)[0].reshape(len(frontier), A, -1)
        for a in range(A):
            assert (kc[:, a] == move_on_cubies(cs, pc, a)).all()
        flat = np.unique(kids.reshape(-1, kids.shape[-1]), axis=0)
        known = {s.tobytes() for s in seen}
        frontier = np.stack([s for s in flat if s.tobytes() not in known])
        seen = np.concatenate([seen, frontier])
    assert count is None or len(seen) == count
    cub, status, cidx, eidx = device_cubies(cs, seen)
    assert (status == 0).all()
    key = cidx.astype(np.uint64)[:, None] if cs == 2 else np.stack([cidx.astype(np.uint64), eidx], axis=1)
    assert len(np.unique(key, axis=0)) == len(seen)
    assert (cidx < (88179840 if cs == 3 else 3674160)).all() and (cs == 2 or (eidx < 479001600 * 2048).all())
    ref = R.cubies(cs, seen)
    assert (ref[0] == cub).all() and (ref[2] == cidx).all() and (cs == 2 or (ref[3] == eidx).all())


def test_all_222_assemblies_on_the_device():
    """All 7! * 3^7 = 11 022 480 assemblies through rcc_from_cubies, then rcc_cubies: 3 674 160 are legal, the others are twisted and
    nothing else, and the legal ones' corner_index values are a permutation of 0 .. 3 674 159."""
    perms = torch.tensor(list(itertools.permutations(range(7))), dtype=torch.uint8, device=DEV)
    oris = torch.tensor(list(itertools.product(range(3), repeat=7)), dtype=torch.uint8, device=DEV)
    c = (perms[:, None, :] * 3 + oris[None, :, :]).reshape(-1, 7)
    n, pitch = len(c), ops.DEFAULT_TILE
    assert n == 11022480
    tiles = -(-n // pitch)
    buf = torch.zeros((tiles * pitch, 7), dtype=torch.uint8, device=DEV)
    buf[:n] = c
    cub = buf.reshape(tiles, pitch, 7).permute(0, 2, 1).contiguous()
    st = ops.from_cubies(cub, n, 2)
    out = ops.cubies(st, n, 2, index=True)
    assert torch.equal(ops.to_aos(out["cubies"], n), c)
    status, idx = out["status"], out["corner_index"]
    assert int((status == 0).sum()) == 3674160 and bool(((status == 0) | (status == R.TWIST)).all())
    assert bool((idx[status != 0] == -1).all())
    legal = idx[status == 0].to(torch.int64)
    assert torch.equal(torch.sort(legal).values, torch.arange(3674160, device=DEV))
    assert bool((status == 0).eq(oris.sum(dim=1, dtype=torch.int64).remainder(3).eq(0)[None, :].expand(5040, -1).reshape(-1)).all())


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_status_is_invariant_under_the_devices_moves(oracle, cs):
    """The twelve (t, f, p) classes (three on the 2x2x2): the status byte is the class's and stays it along 20 rc_apply_moves."""
    base = R.cubies(cs, R.walks(oracle, cs, 16, 30, 9))[0]
    classes = R.classes(cs)
    states = np.concatenate([R.from_cubies(cs, R.mutate(cs, base, *c))[0] for c in classes])
    want = np.repeat([R.class_status(*c) for c in classes], 16).astype(np.uint8)
    n = len(states)
    st = ops.from_aos(states, DEV)
    gen = torch.Generator(device="cpu").manual_seed(cs)
    for step in range(21):
        assert (ops.cubies(st, n, cs, cubies=False)["status"].cpu().numpy() == want).all(), step
        acts = torch.randint(0, LC.A_OF[cs], (n,), dtype=torch.uint8, generator=gen).to(DEV)
        ops.apply_moves(st, st, acts, n, cs, None, None, None, _lib.FMT_NONE)
    assert set(want.tolist()) == {R.class_status(*c) for c in classes} and (want == 0).sum() == 16


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_every_symmetry_of_a_legal_state_is_legal(oracle, cs):
    states = R.walks(oracle, cs, 64, 30, 21)
    st = ops.from_aos(states, DEV)
    for s in range(tables.get_symmetries(cs).count):
        img = ops.apply_symmetry(st, 64, None, cs, s)
        assert int(ops.cubies(img, 64, cs, cubies=False)["status"].max()) == 0, s


# ------------------------------------------------------------------------------------------------------ d. Python surface
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_env_methods(pools, cs):
    from rubiks_cube_solver_amd.vec_env import VecCubeEnv
    P, n = pools[cs], 1029
    env = VecCubeEnv(n, device=DEV, cube_size=cs, obs=None)
    env.set_sim_cube(np.array(P.states[:n]))                                           # check=False: anything loads, as before
    assert (env.sim_cube.cpu().numpy() == P.states[:n]).all()
    assert (env.legality().cpu().numpy() == P.status[:n]).all()
    assert (ops.to_aos(env.cubies(), n).cpu().numpy() == P.cubies[:n]).all()
    got = env.cubies(index=True)
    assert len(got) == (3 if cs == 3 else 2) and (got[1].cpu().numpy().view(np.uint32) == P.cidx[:n]).all()
    assert cs == 2 or (got[2].cpu().numpy().view(np.uint64) == P.eidx[:n]).all()
    # check=True: the first offending cube, its bits by name, the count; the env keeps its cubes
    failed = np.flatnonzero(P.status[:n])
    first = int(failed[0])
    names = " \\| ".join(tables.rcc_status_names(int(P.status[first])))
    with pytest.raises(ValueError, match=rf"cube {first} .*{names}.*; {len(failed)} of {n} cubes failed"):
        env.set_sim_cube(np.array(P.states[:n]), check=True)
    assert (env.sim_cube.cpu().numpy() == P.states[:n]).all()
    legal = P.states[:n][P.status[:n] == 0]
    env2 = VecCubeEnv(len(legal), device=DEV, cube_size=cs, obs="code")
    env2.set_sim_cube(legal, check=True)
    assert (env2.sim_cube.cpu().numpy() == legal).all()
    # from_cubies: rows or the tiled tensor cubies() returns; an unnameable byte raises and changes nothing
    env.from_cubies(np.array(P.cubies_in[:n]))
    assert (env.sim_cube.cpu().numpy() == P.back[:n]).all()
    env3 = VecCubeEnv(len(legal), device=DEV, cube_size=cs, obs=None)
    env3.from_cubies(env2.cubies())
    assert (env3.sim_cube.cpu().numpy() == legal).all()
    broken = np.array(P.cubies_in[:n])
    broken[7, 0] = 0xFF
    with pytest.raises(ValueError):
        env.from_cubies(broken)
    assert (env.sim_cube.cpu().numpy() == P.back[:n]).all()


def test_beam_search_on_the_legal_cubes_of_a_batch(oracle):
    """A batch with illegal cubes, filtered by legality() == 0: the search returns for the cubes it is given exactly what it returns
    for the same cubes inside the unfiltered batch."""
    from rubiks_cube_solver_amd import search
    from rubiks_cube_solver_amd.vec_env import VecCubeEnv
    from tests import beam_ref
    cs = 2
    w = beam_ref.stub_weights(cs, 0)
    model = torch.nn.Linear(len(w), 1, bias=False)
    with torch.no_grad():
        model.weight.copy_(torch.tensor(w)[None])

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = model

        def forward(self, x):
            v = self.lin(x.reshape(x.shape[0], -1))
            return v, v
    legal = np.concatenate([R.walks(oracle, cs, 6, k, 30 + k) for k in (1, 2, 3, 4)])
    twisted = R.from_cubies(cs, R.mutate(cs, R.cubies(cs, legal[:8])[0], 1, 0, 0))[0]
    mixed = np.concatenate([legal[:12], twisted, legal[12:]])
    env = VecCubeEnv(len(mixed), device=DEV, cube_size=cs, obs=None)
    env.set_sim_cube(mixed)
    keep = (env.legality() == 0).cpu().numpy()
    assert keep.sum() == 24 and not keep[12:20].any()
    whole = search.beam_search(Net().to(DEV), env, 64, 6)
    sub = VecCubeEnv(int(keep.sum()), device=DEV, cube_size=cs, obs=None)
    sub.set_sim_cube(mixed[keep], check=True)
    part = search.beam_search(Net().to(DEV), sub, 64, 6)
    k = torch.from_numpy(keep).to(DEV)
    assert torch.equal(part["solved"], whole["solved"][k]) and torch.equal(part["length"], whole["length"][k])
    assert torch.equal(part["actions"], whole["actions"][:, k])
    assert bool(part["solved"].any()) and not bool(whole["solved"][~k].any())      # and no search ever "solves" a twisted cube
