"""The symmetry kernels on the GPU (include/rubiksym.h: rcs_sym_apply, rcs_sym_canonical) and what is built on them
(ops.apply_symmetry / canonical_symmetry, VecCubeEnv.apply_symmetry / canonical, search.beam_search_symmetric).

  a. apply and canonical against the numpy restatement (tests/sym_ref.py): every cube count that opens another path, every ordered
     pair of layouts, every operand carved 16 bytes past a 32-byte boundary, the bytes around every buffer;
  b. by mathematics, on the device's own moves: equivariance, composition, inverses, solvedness and parity, whole spheres;
  c. the canonical form: constant on orbits, minimal, lowest minimiser on states with stabilisers, orbit counts two ways (Burnside);
  d. the env methods and the symmetric beam search.
Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests import group_ref as G
from tests import layout_cases as LC
from tests import sym_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
COUNTS = (1, 3, 4, 5, 511, 513, 1029, 2565)
DEPTHS = (0, 1, 20)                                  # cube i of the pool is a device walk of depth DEPTHS[i % 3]
GUARD = 256                                          # bytes kept around every carved operand
FILL = 0xA5                                          # what pad columns and guards hold before a launch


@pytest.fixture(scope="module")
def ops():
    from rubiks_cube_solver_amd import ops as o
    return o


@pytest.fixture(scope="module")
def lib():
    from rubiks_cube_solver_amd import _lib, _sym_lib
    _lib.init(torch.device(DEV, torch.cuda.current_device()))
    return _sym_lib.sym_lib()


def to_dev(ops, states):
    """[n, S] host rows (the pool's are read-only: copied) -> a tiled device buffer in the default layout."""
    return ops.from_aos(np.array(states), DEV)


def device_walks(ops, cs, n, depth, seed):
    """[n, S] states of rc_scramble walks of `depth` moves from solved."""
    st = ops.alloc_states(n, cs, DEV)
    ops.fill_solved(st, n, cs)
    if depth:
        ops.scramble(st, n, cs, depth, seed=seed, stream_id=9)
    return ops.to_aos(st, n).cpu().numpy()


class Pool:
    """The shared inputs and references of one cube size, computed once: 2565 states, their K images, their canonical forms."""

    def __init__(self, ops, cs):
        n = max(COUNTS)
        per = [device_walks(ops, cs, n, d, 11 + d) for d in DEPTHS]
        self.depth = np.array([DEPTHS[i % 3] for i in range(n)])
        self.states = np.stack([per[i % 3][i] for i in range(n)])
        self.images = R.all_images(cs, self.states)                     # [K, n, S]
        self.can_sym, self.can_img = R.canonical(cs, self.states)
        self.states.setflags(write=False)
        self.images.setflags(write=False)


@pytest.fixture(scope="module")
def pools(ops):
    return {cs: Pool(ops, cs) for cs in LC.CUBE_SIZES}


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
        self.dev = None

    def upload(self):
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 32 == 0
        self.view = self.dev[self.start:self.start + self.nbytes]
        assert self.view.data_ptr() % 32 == (self.start % 32)
        return self

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def check(self, what):
        got = self.dev.cpu().numpy()
        bad = np.flatnonzero(got != self.host)
        assert len(bad) == 0, f"{what}: {len(bad)} bytes differ, first at operand offset {int(bad[0]) - self.start}"


def state_arena(states, rows, layout, offset):
    n = len(states)
    pitch, tiles = LC.layout(layout, n)
    a = Arena(tiles * rows * pitch, offset)
    a.addr = a.start + addresses(n, rows, pitch)
    a.pitch = pitch
    if states is not None:
        a.host[a.addr] = states
    return a


def vec_arena(values, offset):
    a = Arena(len(values), offset)
    a.host[a.start:a.start + len(values)] = values
    return a


def stream():
    from rubiks_cube_solver_amd._lib import stream_ptr
    return stream_ptr(torch.device(DEV, torch.cuda.current_device()))


# ------------------------------------------------------------------------------------- a. against the restatement
def sym_cases(K, n, rng):
    """The per-cube index vectors: drawn at random, all equal, one differing cube in the last pack (the ragged tail where n % 4)."""
    drawn = rng.integers(0, K, n).astype(np.uint8)
    equal = np.full(n, K - 1, np.uint8)
    one = np.full(n, 1, np.uint8)
    one[n - 1] = K - 2
    return (("drawn", drawn), ("equal", equal), ("one", one))


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_apply_matches_restatement(lib, pools, cs, n, offset):
    """Every ordered pair of layouts for (in, out).  Uniform: every s, spread over the pairs so that each pair sees K / 16 (at
    least one) of them and each s at least one pair.  Per cube: the three index vectors with every pair."""
    pool, S, K = pools[cs], LC.S_OF[cs], R.N_SYM[cs]
    x = pool.states[:n]
    rng = np.random.default_rng(n * 10 + cs)
    vectors = sym_cases(K, n, rng)
    for pi, (lin, lout) in enumerate(LC.PAIRS):
        src = state_arena(x, S, lin, offset).upload()
        out0 = state_arena(x, S, lout, offset)
        out0.host[out0.addr] = 7                                         # a value no image holds
        out0.upload()
        pristine = out0.dev.clone()
        for s in sorted({s for s in range(K) if s % 16 == pi % 16} | {pi % K}):
            out0.dev.copy_(pristine)
            rc = lib.rcs_sym_apply(src.ptr(), out0.ptr(), n, src.pitch, out0.pitch, cs, None, s, None, stream())
            assert rc == 0, lib.rc_search_last_error()
            out0.host[out0.addr] = pool.images[s, :n]
            out0.check(f"uniform s={s} {lin}->{lout}")
        for name, vec in vectors:
            sv = vec_arena(vec, offset).upload()
            flag = vec_arena(np.zeros(1, np.uint8), 0).upload()
            out0.dev.copy_(pristine)
            rc = lib.rcs_sym_apply(src.ptr(), out0.ptr(), n, src.pitch, out0.pitch, cs, sv.ptr(), 0, flag.ptr(), stream())
            assert rc == 0, lib.rc_search_last_error()
            out0.host[out0.addr] = pool.images[vec, np.arange(n)]
            out0.check(f"per cube {name} {lin}->{lout}")
            sv.check("sym")
            flag.check("flag")                                           # still zero: no index was out of range
        src.check(f"input {lin}")


@pytest.mark.parametrize("offset", [0, 16])
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_canonical_matches_restatement(lib, pools, cs, n, offset):
    pool, S = pools[cs], LC.S_OF[cs]
    x = pool.states[:n]
    for lin, lout in LC.PAIRS:
        src = state_arena(x, S, lin, offset).upload()
        out = state_arena(x, S, lout, offset)
        out.host[out.addr] = 7
        out.upload()
        so = vec_arena(np.full(n, 0xEE, np.uint8), offset).upload()
        rc = lib.rcs_sym_canonical(src.ptr(), n, src.pitch, cs, so.ptr(), out.ptr(), out.pitch, stream())
        assert rc == 0, lib.rc_search_last_error()
        so.host[so.start:so.start + n] = pool.can_sym[:n]
        out.host[out.addr] = pool.can_img[:n]
        so.check(f"sym_out {lin}->{lout}")
        out.check(f"image {lin}->{lout}")
        src.check(f"input {lin}")
    # without the image: sym_out alone, and pitch_out is ignored
    so = vec_arena(np.full(n, 0xEE, np.uint8), offset).upload()
    assert lib.rcs_sym_canonical(src.ptr(), n, src.pitch, cs, so.ptr(), None, 0, stream()) == 0
    so.host[so.start:so.start + n] = pool.can_sym[:n]
    so.check("sym_out alone")


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_argument_errors_name_the_operand_and_launch_nothing(lib, pools, cs):
    S, K, n = LC.S_OF[cs], R.N_SYM[cs], 37
    x = pools[cs].states[:n]
    src = state_arena(x, S, "tight", 0).upload()
    out = state_arena(x, S, "padded", 0)
    out.host[out.addr] = 7
    out.upload()
    sv = vec_arena(np.zeros(n, np.uint8), 0).upload()
    so = vec_arena(np.full(n, 0xEE, np.uint8), 0).upload()
    p = lambda a, d=0: ctypes.c_void_p(a.view.data_ptr() + d)
    good = dict(i=p(src), o=p(out), n=n, pi=src.pitch, po=out.pitch, cs=cs, sym=p(sv), su=0, so=p(so))
    # (the words the message must hold, the argument that is wrong); 2^28 * S >= 2^32 for both cube sizes
    bad = [("in is", dict(i=None)), ("in is", dict(i=p(src, 8))), ("out is", dict(o=None)), ("out is", dict(o=p(out, 4))), ("sym is", dict(sym=p(sv, 1))),
           ("pitch_in", dict(pi=n)), ("pitch_in", dict(pi=0)), ("pitch_in", dict(pi=32)), ("pitch_out", dict(po=48 + 8)), ("pitch_out", dict(po=-64)),
           ("pitch_in", dict(pi=1 << 28)), ("cube_size", dict(cs=4)), ("n_cubes", dict(n=-1)), ("sym_uniform", dict(sym=None, su=K)),
           ("sym_uniform", dict(sym=None, su=-1)), ("in == out", dict(o=p(src), po=src.pitch)), ("overlap", dict(o=p(src, 16), po=src.pitch))]
    for word, change in bad:
        a = {**good, **change}
        rc = lib.rcs_sym_apply(a["i"], a["o"], a["n"], a["pi"], a["po"], a["cs"], a["sym"], a["su"], None, stream())
        assert rc == -1 and word in lib.rc_search_last_error().decode(), (word, change, rc, lib.rc_search_last_error())
    bad_c = [b for b in bad if b[0] not in ("sym is", "sym_uniform", "out is")] + [("out is", dict(o=p(out, 4))), ("sym_out is", dict(so=None)),
                                                                                     ("sym_out is", dict(so=p(so, 2)))]
    for word, change in bad_c:
        a = {**good, **change}
        rc = lib.rcs_sym_canonical(a["i"], a["n"], a["pi"], a["cs"], a["so"], a["o"], a["po"], stream())
        assert rc == -1 and word in lib.rc_search_last_error().decode(), (word, change, rc, lib.rc_search_last_error())
    # n_cubes == 0 succeeds, and nothing above or here was launched: every byte is where it was
    assert lib.rcs_sym_apply(p(src), p(out), 0, src.pitch, out.pitch, cs, None, 0, None, stream()) == 0
    assert lib.rcs_sym_apply(p(src), p(out), 0, src.pitch, out.pitch, cs, p(sv), 0, None, stream()) == 0
    assert lib.rcs_sym_canonical(p(src), 0, src.pitch, cs, p(so), p(out), out.pitch, stream()) == 0
    for a, what in ((src, "in"), (out, "out"), (sv, "sym"), (so, "sym_out")):
        a.check(what)


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_out_of_range_index_sets_the_flag_and_keeps_the_cube(lib, ops, pools, cs):
    S, K, n = LC.S_OF[cs], R.N_SYM[cs], 517
    pool = pools[cs]
    x = pool.states[:n]
    vec = np.random.default_rng(5).integers(0, K, n).astype(np.uint8)
    vec[[3, 515]] = (K, 255)
    want = pool.images[np.where(vec < K, vec, 0), np.arange(n)]
    src = state_arena(x, S, "t512", 0).upload()
    out = state_arena(x, S, "tight", 0)
    out.host[out.addr] = 7
    out.upload()
    sv = vec_arena(vec, 0).upload()
    flag = vec_arena(np.zeros(1, np.uint8), 0).upload()
    assert lib.rcs_sym_apply(src.ptr(), out.ptr(), n, src.pitch, out.pitch, cs, sv.ptr(), 0, flag.ptr(), stream()) == 0
    out.host[out.addr] = want
    out.check("images")
    flag.host[flag.start] = 1
    flag.check("flag")
    # the same through ops: IndexError; an int out of range is refused on the host
    st = to_dev(ops, x)
    with pytest.raises(IndexError):
        ops.apply_symmetry(st, n, None, cs, torch.from_numpy(vec).to(DEV))
    with pytest.raises(IndexError):
        ops.apply_symmetry(st, n, None, cs, K)
    got = ops.apply_symmetry(st, n, None, cs, torch.from_numpy(np.where(vec < K, vec, 0).astype(np.uint8)).to(DEV))
    assert (ops.to_aos(got, n).cpu().numpy() == want).all()


# ------------------------------------------------------------------------------------------- b. by mathematics
def dev_apply(ops, cs, st, n, s):
    return ops.apply_symmetry(st, n, None, cs, s)


def same(ops, a, b, n):
    """Equal cubes (pad columns of a fresh output hold anything)."""
    return torch.equal(ops.to_aos(a, n), ops.to_aos(b, n))


def dev_move(ops, cs, st, n, a):
    out = torch.empty_like(st)
    ops.apply_moves(st, out, torch.full((st.shape[0] * st.shape[-1],), a, dtype=torch.uint8, device=DEV), n, cs)
    return out


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_equivariance_with_the_device_moves(ops, pools, cs):
    """T_s(move_a(x)) == move_{amap[s][a]}(T_s(x)) for every (s, a), moves by rc_apply_moves, both symmetry kernels."""
    r, n = R.build(cs), 512
    x = to_dev(ops, pools[cs].states[:n])
    moved = [dev_move(ops, cs, x, n, a) for a in range(G.N_ACTIONS[cs])]
    for s in range(r.K):
        tx = dev_apply(ops, cs, x, n, s)
        per_cube = torch.full((n,), s, dtype=torch.uint8, device=DEV)
        for a in range(G.N_ACTIONS[cs]):
            right = dev_move(ops, cs, tx, n, int(r.amap[s][a]))
            assert same(ops, dev_apply(ops, cs, moved[a], n, s), right, n), (s, a)
            if a == s % G.N_ACTIONS[cs]:
                assert same(ops, dev_apply(ops, cs, moved[a], n, per_cube), right, n), (s, a)


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_composition_and_inverses(ops, pools, cs):
    r = R.build(cs)
    K = r.K
    n = K * K                                                            # cube s * K + u: apply s, then u
    x = to_dev(ops, pools[cs].states[np.arange(n) % 2565])
    first = torch.arange(K, dtype=torch.uint8).repeat_interleave(K).to(DEV)
    second = torch.arange(K, dtype=torch.uint8).repeat(K).to(DEV)
    both = torch.from_numpy(r.compose.reshape(-1)).to(DEV)
    assert same(ops, dev_apply(ops, cs, dev_apply(ops, cs, x, n, first), n, second), dev_apply(ops, cs, x, n, both), n)
    inv = torch.from_numpy(r.inverse).to(DEV).repeat_interleave(K)
    assert same(ops, dev_apply(ops, cs, dev_apply(ops, cs, x, n, first), n, inv), x, n)
    for s in range(K):                                                   # and with the uniform kernel
        assert same(ops, dev_apply(ops, cs, dev_apply(ops, cs, x, n, s), n, int(r.inverse[s])), x, n), s
        u = (5 * s + 1) % K
        assert same(ops, dev_apply(ops, cs, dev_apply(ops, cs, x, n, s), n, u), dev_apply(ops, cs, x, n, int(r.compose[s][u])), n), (s, u)


def permutation_parity(p):
    seen, odd = np.zeros(len(p), bool), 0
    for i in range(len(p)):
        k, length = i, 0
        while not seen[k]:
            seen[k] = True
            k = p[k]
            length += 1
        odd ^= (length - 1) & 1 if length else 0                            # a cycle of length L is L - 1 transpositions
    return odd


def state_parity(ops, cs, st, n):
    """Parity of the walk that made each state, read off the device's compact code: a quarter turn is a 4-cycle of edge cubies
    (3x3x3: slots 8..19, piece = code / 2) and of corner cubies (2x2x2: 7 slots, piece = code / 3; the eighth cubie never moves)."""
    from rubiks_cube_solver_amd import _lib
    code = ops.alloc_code(n, cs, DEV)
    ops.encode(st, n, cs, code, _lib.FMT_CODE)
    c = ops.to_aos(code, n).cpu().numpy().astype(np.int64)
    pieces = c[:, 8:] // 2 if cs == 3 else c // 3
    for row in pieces:
        assert sorted(row) == list(range(pieces.shape[1]))
    return np.array([permutation_parity(row) for row in pieces])


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_solved_flag_and_parity_class_are_invariant(ops, pools, cs):
    pool, n = pools[cs], 600
    x = to_dev(ops, pool.states[:n])
    done0 = torch.empty(n, dtype=torch.uint8, device=DEV)
    ops.is_solved(x, n, cs, done0)
    assert (done0.cpu().numpy() == (pool.depth[:n] == 0)).all()          # a 1- or 20-move walk of the pool is never back at solved
    assert (state_parity(ops, cs, x, n) == pool.depth[:n] % 2).all()
    done = torch.empty(n, dtype=torch.uint8, device=DEV)
    for s in range(R.N_SYM[cs]):
        tx = dev_apply(ops, cs, x, n, s)
        ops.is_solved(tx, n, cs, done)
        assert torch.equal(done, done0), s
        assert (state_parity(ops, cs, tx, n) == pool.depth[:n] % 2).all(), s


@pytest.fixture(scope="module")
def spheres(ops):
    """The complete spheres, 3x3x3 to depth 4 and 2x2x2 to depth 5, by rc_expand_children and tests/group_ref.py."""
    from rubiks_cube_solver_amd import _lib
    from tests.test_gpu_group import dev_bfs
    out = {}
    for cs, depth, counts in ((3, 4, G.SPHERES_333), (2, 5, G.SPHERES_222)):
        levels = dev_bfs(ops, _lib, cs, depth)
        assert tuple(len(lv.states) for lv in levels) == tuple(counts[:depth + 1])
        out[cs] = [lv.states for lv in levels]
    return out


def sorted_words(states):
    w = G.pack(states)
    return w[np.lexsort(w.T[::-1])]


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_every_symmetry_maps_each_sphere_onto_itself(ops, spheres, cs):
    for d, sph in enumerate(spheres[cs]):
        n = len(sph)
        want = sorted_words(sph)
        x = to_dev(ops, sph)
        for s in range(R.N_SYM[cs]):
            got = ops.to_aos(dev_apply(ops, cs, x, n, s), n).cpu().numpy()
            assert (sorted_words(got) == want).all(), (d, s)


# --------------------------------------------------------------------------------------------- c. canonical form
def dev_canonical(ops, cs, states):
    n = len(states)
    x = to_dev(ops, states)
    img = torch.full_like(x, 7)
    sym = ops.canonical_symmetry(x, n, None, cs, out=img)
    return sym.cpu().numpy(), ops.to_aos(img, n).cpu().numpy()


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_canonical_image_is_constant_on_orbits_and_minimal(ops, pools, cs):
    K, m = R.N_SYM[cs], 60
    x = pools[cs].states[:m]
    orbit = R.all_images(cs, x)                                          # [K, m, S]: row t = T_t(x), by the restatement ...
    on_dev = ops.to_aos(dev_apply(ops, cs, to_dev(ops, np.tile(x, (K, 1))), K * m,
                                  torch.arange(K, dtype=torch.uint8).repeat_interleave(m).to(DEV)), K * m).cpu().numpy()
    assert (on_dev == orbit.reshape(K * m, -1)).all()                    # ... and by the device
    sym, img = dev_canonical(ops, cs, on_dev)
    img = img.reshape(K, m, -1)
    assert (img == img[0]).all()                                         # canonical(T_t(x)) is the same image for every t
    for c in range(m):
        rows = [orbit[t, c].tobytes() for t in range(K)]
        assert img[0, c].tobytes() == min(rows)                          # <= every image, and one of them


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_lowest_minimiser_on_states_with_stabilisers(ops, spheres, cs):
    """The solved cube (stabiliser = all K), the depth-1 sphere (on the 3x3x3 a face turn is fixed by the four rotations about its
    axis) and the depth-2 sphere (half turns, turns of opposite faces): several s give the smallest image, sym_out is the lowest."""
    K = R.N_SYM[cs]
    x = np.concatenate(spheres[cs][:3])
    sym, img = dev_canonical(ops, cs, x)
    ref_sym, ref_img = R.canonical(cs, x)
    assert (sym == ref_sym).all() and (img == ref_img).all()
    im = R.all_images(cs, x)
    tied = []
    for c in range(len(x)):
        minimisers = [s for s in range(K) if (im[s, c] == img[c]).all()]
        assert sym[c] == minimisers[0]
        tied.append(len(minimisers))
    assert sym[0] == 0 and tied[0] == K                                  # the solved cube: every s is a minimiser, the lowest is 0
    if cs == 3:
        assert min(tied[1:13]) >= 4 and max(tied[13:]) >= 2              # every face turn, and some states two moves out


@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_orbit_counts_two_ways(ops, spheres, cs):
    """Per sphere: the number of distinct canonical images (rcs_sym_canonical) == Burnside's (1 / K) sum_s #{x : T_s x == x} with the
    fixed points found through rcs_sym_apply == the restatement's count."""
    K = R.N_SYM[cs]
    for d, sph in enumerate(spheres[cs]):
        n = len(sph)
        _, img = dev_canonical(ops, cs, sph)
        by_canonical = G.count_distinct(G.pack(img))
        x = to_dev(ops, sph)
        xa = ops.to_aos(x, n)
        fixed = sum(int((ops.to_aos(dev_apply(ops, cs, x, n, s), n) == xa).all(dim=1).sum()) for s in range(K))
        assert fixed % K == 0, (d, fixed)
        assert by_canonical == fixed // K == R.orbit_count(cs, sph), (d, by_canonical, fixed // K)
        assert R.burnside(cs, sph) == fixed // K


# ------------------------------------------------------------------------------------------------------ d. env
@pytest.mark.parametrize("obs", ["onehot", "code"])
@pytest.mark.parametrize("cs", LC.CUBE_SIZES)
def test_env_apply_symmetry(oracle, pools, cs, obs):
    from rubiks_cube_solver_amd import VecCubeEnv
    r, n, A = R.build(cs), 300, G.N_ACTIONS[cs]
    x = pools[cs].states[:n]
    env = VecCubeEnv(n, DEV, cs, obs=obs, auto_reset=True, scramble_count=3, max_episode_steps=9)
    env.set_sim_cube(np.array(x))
    env.elapsed.copy_(torch.arange(n, dtype=torch.int32) % 7)
    env.episode.copy_(torch.arange(n, dtype=torch.int32) % 5)
    counters = [t.clone() for t in (env.elapsed, env.episode, env.ended, env.episode_length)]

    def check_obs(o, states):
        code, onehot = oracle.encode(cs, states)
        if obs == "code":
            from rubiks_cube_solver_amd import ops
            assert (ops.to_aos(o, n).cpu().numpy() == code).all()
        else:
            assert (o.cpu().numpy() == onehot).all()

    rng = np.random.default_rng(3)
    host = x
    for sym in (5 % r.K, rng.integers(0, r.K, n).astype(np.uint8), r.K - 1):
        arg = torch.from_numpy(sym).to(DEV) if isinstance(sym, np.ndarray) else int(sym)
        o = env.apply_symmetry(arg)
        host = R.apply(cs, host, sym)
        assert (env.sim_cube.cpu().numpy() == host).all()
        check_obs(o, host)
        env.check_actions()                                              # nothing was out of range
    for got, want in zip((env.elapsed, env.episode, env.ended, env.episode_length), counters):
        assert torch.equal(got, want)
    assert (env.canonical().cpu().numpy() == R.canonical(cs, host)[0]).all()
    assert (env.sim_cube.cpu().numpy() == host).all()                    # canonical() leaves the cubes as they are
    # a following step(amap[s][a]) is the image of step(a): plain envs, per-cube symmetries and actions
    a = rng.integers(0, A, n).astype(np.uint8)
    s = rng.integers(0, r.K, n).astype(np.uint8)
    e1, e2 = VecCubeEnv(n, DEV, cs, obs=None), VecCubeEnv(n, DEV, cs, obs=None)
    e1.set_sim_cube(np.array(x))
    e2.set_sim_cube(np.array(x))
    e1.step(torch.from_numpy(a).to(DEV))
    e1.apply_symmetry(torch.from_numpy(s).to(DEV))
    e2.apply_symmetry(torch.from_numpy(s).to(DEV))
    e2.step(torch.from_numpy(r.amap[s, a]).to(DEV))
    assert torch.equal(e1.sim_cube, e2.sim_cube)
    assert (e1.sim_cube.cpu().numpy() == R.apply(cs, oracle.step(cs, x, a)[0], s)).all()
    # a bad index in a tensor surfaces at check_actions(), once
    s[7] = r.K
    e2.apply_symmetry(torch.from_numpy(s).to(DEV))
    with pytest.raises(IndexError):
        e2.check_actions()
    e2.check_actions()
    with pytest.raises(IndexError):
        e2.apply_symmetry(r.K)


# ------------------------------------------------------------------------------------------- d. symmetric beam search
def random_net(cs):
    from tests.test_gpu_search import DeepCube, _random_deepcube
    return DeepCube(_random_deepcube(cs)).to(DEV).eval()


def scrambled_env(cs, depths, seed):
    from rubiks_cube_solver_amd import VecCubeEnv
    A = G.N_ACTIONS[cs]
    rng = np.random.default_rng(seed)
    scr = np.full((len(depths), max(depths)), A, np.uint8)
    for i, k in enumerate(depths):
        scr[i, :k] = rng.integers(0, A, k)
    env = VecCubeEnv(len(depths), DEV, cs, obs=None)
    env.reset(actions=scr)
    return env


@pytest.mark.parametrize("cs,P,W,D", [(2, 40, 4, 10), (3, 20, 8, 6)])
def test_identity_alone_is_beam_search(cs, P, W, D):
    from rubiks_cube_solver_amd import search
    env = scrambled_env(cs, [1 + i % (8 if cs == 2 else 4) for i in range(P)], 1)
    model = random_net(cs)
    a = search.beam_search(model, env, W, D)
    b = search.beam_search_symmetric(model, env, W, D, symmetries=(0,))
    for k in ("solved", "length", "actions"):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert (b["symmetry"].cpu().numpy() == np.where(a["solved"].cpu().numpy(), 0, -1)).all() and b["symmetry"].dtype == torch.int32


@pytest.mark.parametrize("cs,P,maxk,W,D,syms", [(2, 40, 8, 4, 12, "all"), (3, 20, 4, 8, 8, (0, 5, 24, 47))])
def test_symmetric_beam_search(oracle, cs, P, maxk, W, D, syms):
    from rubiks_cube_solver_amd import search
    A = G.N_ACTIONS[cs]
    env = scrambled_env(cs, [1 + i % maxk for i in range(P)], 2)
    before = env.stickers.clone()
    x = env.sim_cube.cpu().numpy()
    res = search.beam_search_symmetric(random_net(cs), env, W, D, symmetries=syms, return_all=True)
    assert torch.equal(env.stickers, before)
    idx = search.symmetry_indices(syms, cs)
    k = len(idx)
    all_len, all_act = res["all_length"].cpu().numpy(), res["all_actions"].cpu().numpy()
    assert all_len.shape == (k, P) and all_act.shape == (k, D, P) and res["actions"].shape == (D, P)
    solved_root = oracle.solved(cs, 1)[0]
    for j in range(k):                                                   # every image's mapped-back list solves the ORIGINAL cube
        st = x.copy()
        for d in range(D):
            live = d < all_len[j]
            assert (all_act[j, d][live] < A).all() and (all_act[j, d][~live] == A).all(), (j, d)
            assert not (st[live] == solved_root).all(axis=1).any(), (j, d)   # ... at exactly its reported length: not solved before it
            acts = np.where(live, all_act[j, d], 0).astype(np.uint8)
            nxt = oracle.step(cs, st, acts)[0]
            st = np.where(live[:, None], nxt, st)
        ok = all_len[j] >= 0
        assert (st[ok] == solved_root).all()
    assert (all_len >= 0).any()
    length, chosen, actions = res["length"].cpu().numpy(), res["symmetry"].cpu().numpy(), res["actions"].cpu().numpy()
    for p in range(P):
        solved_js = [j for j in range(k) if all_len[j, p] >= 0]
        if not solved_js:
            assert length[p] == -1 and chosen[p] == -1 and not bool(res["solved"][p]) and (actions[:, p] == A).all()
            continue
        best = min(solved_js, key=lambda j: (all_len[j, p], j))          # the minimum length, ties to the lowest j
        assert length[p] == all_len[best, p] and chosen[p] == idx[best] and bool(res["solved"][p])
        assert (actions[:, p] == all_act[best, :, p]).all()
