"""rcx_episode_end (include/rubikepisode.h) and what is built on it, on the device: the kernel against the numpy restatement of its
rule (tests/episode_ref.py: Oracle.step moves, big-int draws) and against the library's own rc_scramble, its argument errors, the
auto-reset VecCubeEnv end to end and under a replayed hipGraph, and rollout.collect.  Every comparison is exact.

Layouts come from tests/layout_cases.py: the multi-tile sizes run in 512-cube tiles and in one padded tile, the small sizes in one
padded tile.  Pad columns of the state buffer are filled with 0xEE and every counter array has 8 sentinel elements behind cube n - 1:
a lane of the last pack that wrote past the batch would change them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import episode_ref as E
from tests import layout_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = (1, 5, 256, 257) + C.SIZES                                 # 513, 1029, 2565: whole waves + a ragged tail, several 512 tiles
assert C.SIZES == (513, 1029, 2565)
SENTINEL = {torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A}
SLACK = 8


def tilings(n):
    return ("t512", "padded") if n > 512 else ("padded",)


SIZE_CASES = [(cs, n, lay) for cs in C.CUBE_SIZES for n in SIZES for lay in tilings(n)]
KW = dict(seed=5, stream_id=9, walk_offset=1000, walk_stride=4096)


@pytest.fixture(scope="module")
def ops():
    from rubiks_cube_solver_amd import ops as o
    return o


@pytest.fixture(scope="module")
def X():
    from rubiks_cube_solver_amd import _episode_lib, _lib
    _lib.init(torch.device(DEV, torch.cuda.current_device()))
    return _episode_lib


_STARTS = {}


def starts(oracle, cs, n):
    """[n, S] reachable, mostly unsolved start states (4-move walks), computed once per shape and shared read only."""
    if (cs, n) not in _STARTS:
        _STARTS[cs, n] = oracle.adi(cs, n, 5, seed=21, stream=4, want_children=False)["parents"][:, -1].copy()
    return _STARTS[cs, n]


def put(ops, aos, lay, n):
    """[n, S] host stickers -> device buffer in layout `lay`, every pad column 0xEE."""
    pitch, tiles = C.layout(lay, n)
    full = np.full((tiles * pitch, aos.shape[1]), 0xEE, np.uint8)
    full[:n] = aos
    buf = ops.from_aos(full, DEV, pitch)
    assert tuple(buf.shape) == C.shape(lay, n, aos.shape[1])
    return buf


def vec(values, n, dtype):
    """[n] device array with SLACK sentinel elements behind it"""
    t = torch.full((n + SLACK,), SENTINEL[dtype], dtype=dtype, device=DEV)
    t[:n] = torch.as_tensor(np.asarray(values)).to(DEV, dtype)
    return t


def host(t, n):
    return t[:n].cpu().numpy()


def run_and_compare(ops, oracle, cs, n, lay, st0, done, elapsed, episode, **kw):
    """One ops.episode_end on the device and the rule on the host; everything compared.  -> the host results."""
    want = E.episode_end(oracle, cs, st0, done, elapsed, episode, **kw)
    buf = put(ops, st0, lay, n)
    d_done, d_el, d_ep = vec(done, n, torch.uint8), vec(elapsed, n, torch.int32), vec(episode, n, torch.int32)
    d_ended, d_len = vec(np.full(n, 77), n, torch.uint8), vec(np.full(n, -3), n, torch.int32)
    ops.episode_end(buf, n, cs, d_done, d_el, d_ep, d_ended, d_len, **kw)
    compare(ops, n, buf, (d_done, d_el, d_ep, d_ended, d_len), done, want)
    return want


def compare(ops, n, buf, dev_vecs, done, want):
    d_done, d_el, d_ep, d_ended, d_len = dev_vecs
    w_st, w_el, w_ep, w_ended, w_len = want
    total = buf.shape[0] * buf.shape[2]
    got = ops.to_aos(buf, total).cpu().numpy()
    assert (host(d_ended, n) == w_ended).all() and (host(d_len, n) == w_len).all()
    assert (host(d_el, n) == w_el).all() and (host(d_ep, n) == w_ep).all() and (host(d_done, n) == done).all()
    bad = np.flatnonzero((got[:n] != w_st).any(axis=1))
    assert len(bad) == 0, (bad[:8], w_ended[bad[:8]])
    assert (got[n:] == 0xEE).all()                                   # pad columns keep their bytes
    for t in dev_vecs:
        assert (t[n:] == SENTINEL[t.dtype]).all()                   # nothing written behind cube n - 1


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("cs,n,lay", SIZE_CASES)
def test_no_cube_ended(ops, oracle, cs, n, lay):
    """Nothing ended: the state buffer is byte-equal to before (pads included), elapsed + 1, ended = length = 0, episode untouched."""
    st0 = starts(oracle, cs, n)
    rng = np.random.default_rng(n)
    elapsed, episode = rng.integers(0, 50, n), rng.integers(0, 9, n)
    buf = put(ops, st0, lay, n)
    before = buf.clone()
    d_done, d_el, d_ep = vec(np.zeros(n), n, torch.uint8), vec(elapsed, n, torch.int32), vec(episode, n, torch.int32)
    d_ended, d_len = vec(np.full(n, 77), n, torch.uint8), vec(np.full(n, -3), n, torch.int32)
    ops.episode_end(buf, n, cs, d_done, d_el, d_ep, d_ended, d_len, max_steps=0, depth=(1, 3), **KW)
    assert torch.equal(buf, before)
    assert (host(d_el, n) == elapsed + 1).all() and (host(d_ep, n) == episode).all()
    assert (host(d_ended, n) == 0).all() and (host(d_len, n) == 0).all()
    for t in (d_done, d_el, d_ep, d_ended, d_len):
        assert (t[n:] == SENTINEL[t.dtype]).all()
    # the same through the time limit: below it nothing ends either
    run_and_compare(ops, oracle, cs, n, lay, st0, np.zeros(n, np.uint8), np.zeros(n, np.int32), episode, max_steps=2, depth=2, **KW)


@pytest.mark.parametrize("cs,n,lay", SIZE_CASES)
def test_all_ended(ops, oracle, cs, n, lay):
    """Every cube solved its episode: each one becomes the reference scramble of its own walk."""
    rng = np.random.default_rng(n + 1)
    want = run_and_compare(ops, oracle, cs, n, lay, starts(oracle, cs, n), np.ones(n, np.uint8), rng.integers(0, 50, n),
                           rng.integers(0, 3, n), max_steps=0, depth=(3, 3), **KW)
    assert (want[3] == 1).all() and (want[4] > 0).all()


def mixed_mask(n):
    """n = 1029.  Wave 0 (cubes 0..255): pack p < 16 holds subset p of a 4-pack, the other packs nothing.  Wave 1: nothing.  Wave 2
    (512..767): only a cube of its last lane.  Wave 3: nothing.  The ragged tail (1024..1028): only cube n - 1."""
    assert n == 1029
    m = np.zeros(n, np.uint8)
    for p in range(16):
        for j in range(4):
            m[4 * p + j] = (p >> j) & 1
    m[765] = 1
    m[n - 1] = 1
    assert not m[256:512].any() and not m[768:1024].any() and m[512:768].sum() == 1 and 764 <= 765 < 768 and m[1024:].sum() == 1
    return m


@pytest.mark.parametrize("lay", tilings(1029))
@pytest.mark.parametrize("cs", C.CUBE_SIZES)
def test_mixed_masks(ops, oracle, cs, lay):
    """All 16 subsets of a pack, a wave without an ended cube next to a wave whose last lane alone ended, only the last cube of a
    ragged tail: ended cubes are their reference scrambles, their neighbours keep their bytes."""
    n = 1029
    m = mixed_mask(n)
    st0 = starts(oracle, cs, n)
    want = run_and_compare(ops, oracle, cs, n, lay, st0, m, np.arange(n) % 7, np.arange(n) % 3, max_steps=0, depth=(1, 4), **KW)
    assert (want[0][m == 0] == st0[m == 0]).all() and (want[3] == m).all()


@pytest.mark.parametrize("cs", C.CUBE_SIZES)
def test_truncation(ops, oracle, cs):
    """max_steps = 3, elapsed from {0, 1, 2, 5}, done 0 and 1: terminated wins over truncated; max_steps = 0 never truncates."""
    n = 257
    elapsed = np.array([0, 1, 2, 5], np.int32)[np.arange(n) % 4]
    done = ((np.arange(n) // 4) % 2).astype(np.uint8)
    st0 = starts(oracle, cs, n)
    _, el, _, ended, length = run_and_compare(ops, oracle, cs, n, "padded", st0, done, elapsed, np.zeros(n, np.int32), max_steps=3, depth=2, **KW)
    assert (ended[done == 1] == 1).all()
    assert (ended[done == 0] == np.where(elapsed[done == 0] + 1 >= 3, 2, 0)).all() and set(ended.tolist()) == {0, 1, 2}
    assert (length[ended != 0] == elapsed[ended != 0] + 1).all() and (el[ended != 0] == 0).all()
    ended0 = run_and_compare(ops, oracle, cs, n, "padded", st0, done, elapsed, np.zeros(n, np.int32), max_steps=0, depth=2, **KW)[3]
    assert (ended0 == done).all()


@pytest.mark.parametrize("depth", [(0, 0), (3, 3), (1, 4)])
@pytest.mark.parametrize("cs", C.CUBE_SIZES)
def test_depth_and_consecutive_episodes(ops, oracle, cs, depth):
    """Two calls with the same mask start episodes 1 and 2 of the ended cubes: both are the reference's, and they differ from each
    other; another stream_id gives other cubes.  (Depth 0: every fresh cube is the solved cube.)
    Two independent scrambles of depth >= 1 coincide with probability <= 1/6 per cube: more than half of ~250 cubes must differ."""
    n = 513
    m = (np.random.default_rng(3).random(n) < 0.5).astype(np.uint8)
    st0, zeros = starts(oracle, cs, n), np.zeros(n, np.int32)
    kw = dict(max_steps=0, depth=depth, **KW)
    first = run_and_compare(ops, oracle, cs, n, "t512", st0, m, zeros, zeros, **kw)
    second = run_and_compare(ops, oracle, cs, n, "t512", first[0], m, first[1], first[2], **kw)
    assert (first[2] == m).all() and (second[2] == 2 * m.astype(np.int32)).all()
    other = run_and_compare(ops, oracle, cs, n, "t512", st0, m, zeros, zeros, **dict(kw, stream_id=KW["stream_id"] + 1))
    a, b, c = first[0][m == 1], second[0][m == 1], other[0][m == 1]
    if depth == (0, 0):
        assert (a == oracle.solved(cs, 1)).all() and (b == a).all() and (c == a).all()
    else:
        assert (a != b).any(axis=1).mean() > 0.5 and (a != c).any(axis=1).mean() > 0.5


@pytest.mark.parametrize("cs", C.CUBE_SIZES)
def test_agrees_with_rc_scramble(ops, oracle, cs):
    """depth (3, 3): the ended cubes are rc_fill_solved + rc_scramble(depth 3) at walk_offset + ep * walk_stride, from the library."""
    n, S = 1029, C.S_OF[cs]
    rng = np.random.default_rng(8)
    m = (rng.random(n) < 0.4).astype(np.uint8)
    episode = rng.integers(0, 3, n).astype(np.int32)
    st0 = starts(oracle, cs, n)
    buf = put(ops, st0, "t512", n)
    d_done, d_el, d_ep = vec(m, n, torch.uint8), vec(np.zeros(n), n, torch.int32), vec(episode, n, torch.int32)
    d_ended, d_len = vec(np.zeros(n), n, torch.uint8), vec(np.zeros(n), n, torch.int32)
    ops.episode_end(buf, n, cs, d_done, d_el, d_ep, d_ended, d_len, max_steps=0, depth=3, **KW)
    got = ops.to_aos(buf, n).cpu().numpy()
    assert (got[m == 0] == st0[m == 0]).all()
    for ep in (1, 2, 3):
        ref = ops.alloc_states(n, cs, DEV)
        ops.fill_solved(ref, n, cs)
        ops.scramble(ref, n, cs, 3, seed=KW["seed"], stream_id=KW["stream_id"], walk_offset=KW["walk_offset"] + ep * KW["walk_stride"])
        pick = (m == 1) & (episode + 1 == ep)
        assert pick.any() and (got[pick] == ops.to_aos(ref, n).cpu().numpy()[pick]).all()
    assert got.shape == (n, S)


# ---------------------------------------------------------------------------------------------------------- the C ABI
P = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731


def abi_operands(ops, oracle, cs, n, lay, carved=False):
    """Operands of one raw rcx_episode_end call.  carved: every pointer 16 bytes past a 32-byte boundary (layout_cases.carve_offsets)."""
    st0 = starts(oracle, cs, n)
    rng = np.random.default_rng(12)
    done, elapsed, episode = (rng.random(n) < 0.3).astype(np.uint8), rng.integers(0, 4, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32)
    src = [put(ops, st0, lay, n), vec(done, n, torch.uint8), vec(elapsed, n, torch.int32), vec(episode, n, torch.int32),
           vec(np.full(n, 77), n, torch.uint8), vec(np.full(n, -3), n, torch.int32)]
    if carved:
        out = []
        for t, off in zip(src, C.carve_offsets(len(src))):
            raw = torch.full((off + t.numel() * t.element_size() + 64,), 0xEE, dtype=torch.uint8, device=DEV)
            view = raw[off:off + t.numel() * t.element_size()].view(t.dtype).reshape(t.shape)
            assert view.data_ptr() % 32 == 16
            view.copy_(t)
            out.append(view)
        src = out
    return st0, done, elapsed, episode, src


def raw_call(X, L, cs, n, pitch, t, *, max_steps=3, lo=1, hi=3, stride=4096, null=None, offs=None):
    """rcx_episode_end on tensors t = [st, done, elapsed, episode, ended, length]; offs: byte offsets added to the pointers."""
    ptrs = [None if null == i else P(x, (offs or {}).get(i, 0)) for i, x in enumerate(t)]
    return X.episode_lib().rcx_episode_end(ptrs[0], n, pitch, cs, ptrs[1], ptrs[2], max_steps, ptrs[3], lo, hi, KW["seed"], KW["stream_id"],
                                           KW["walk_offset"], stride, ptrs[4], ptrs[5], L.stream_ptr(DEV))


@pytest.mark.parametrize("cs", C.CUBE_SIZES)
def test_argument_errors(ops, oracle, X, cs):
    """Every RC_EINVAL of the header: -1, the operand named, nothing launched (all buffers as before); n_cubes = 0 succeeds."""
    from rubiks_cube_solver_amd import _lib as L
    n, names = 257, ("st", "done", "elapsed", "episode", "ended", "length")
    _, _, _, _, t = abi_operands(ops, oracle, cs, n, "padded")
    pitch = t[0].shape[2]
    before = [x.clone() for x in t]
    err = lambda: L.lib().rc_last_error().decode()

    def refused(word, *a, **k):
        assert raw_call(X, L, cs, *a, **k) == -1 and word in err(), (word, err())

    for i, name in enumerate(names):
        refused(name + " is NULL or not 16-byte aligned", n, pitch, t, null=i)
        refused(name + " is NULL or not 16-byte aligned", n, pitch, t, offs={i: 4})   # 4-byte aligned, not 16: done / ended included
        refused(name + " is NULL or not 16-byte aligned", n, pitch, t, offs={i: 8})
    refused("pitch", n, pitch - 8, t)                                    # not a multiple of 16
    refused("pitch", n, 256, t)                                          # several tiles need a power of two >= 512: 256 < n
    refused("pitch", n, 0, t)
    assert raw_call(X, L, 4, n, pitch, t) == -1 and "cube_size" in err()
    refused("n_cubes", -1, pitch, t)
    refused("max_steps", n, pitch, t, max_steps=-1)
    refused("depth_lo", n, pitch, t, lo=-1)
    refused("depth_hi", n, pitch, t, lo=3, hi=2)
    refused("walk_stride", n, pitch, t, stride=-1)
    assert raw_call(X, L, cs, 0, pitch, t) == 0
    torch.cuda.synchronize()
    for x, y in zip(t, before):
        assert torch.equal(x, y)
    # the Python layer refuses the same before it reaches the library
    with pytest.raises(L.RubikHipError):
        ops.episode_end(t[0], n, cs, t[1][4:], t[2], t[3], t[4], t[5], max_steps=3, depth=(1, 3), **KW)
    with pytest.raises(ValueError):
        ops.episode_end(t[0], n, cs, t[1], t[2], t[3], t[4], t[5], max_steps=3, depth=(3, 1), **KW)


@pytest.mark.parametrize("lay", tilings(1029))
@pytest.mark.parametrize("cs", C.CUBE_SIZES)
def test_carved_pointers(ops, oracle, X, cs, lay):
    """Every pointer 16 bytes past a 32-byte boundary: 16 bytes is all the alignment the call needs."""
    from rubiks_cube_solver_amd import _lib as L
    n = 1029
    st0, done, elapsed, episode, t = abi_operands(ops, oracle, cs, n, lay, carved=True)
    kw = dict(max_steps=3, depth=(1, 3), seed=KW["seed"], stream_id=KW["stream_id"], walk_offset=KW["walk_offset"], walk_stride=4096)
    assert raw_call(X, L, cs, n, t[0].shape[2], t) == 0, L.lib().rc_last_error()
    compare(ops, n, t[0], t[1:], done, E.episode_end(oracle, cs, st0, done, elapsed, episode, **kw))


# ---------------------------------------------------------------------------------------------------------- VecCubeEnv
def make_env(cs, obs, case, **kw):
    from rubiks_cube_solver_amd.vec_env import VecCubeEnv
    return VecCubeEnv(case["n"], DEV, cs, obs=obs, seed=case["seed"], stream_id=case["stream_id"], auto_reset=True,
                      scramble_count=case["scramble_count"], max_episode_steps=case["max_episode_steps"], **kw)


@pytest.mark.parametrize("obs", ["code", "onehot"])
@pytest.mark.parametrize("cs", C.CUBE_SIZES)
def test_vec_env_end_to_end(ops, oracle, cs, obs):
    """40 steps of host-drawn actions: reward, done, ended, episode_length, observation and stickers of every step equal the reference
    env's.  The run holds terminated and truncated episodes (asserted on the reference first)."""
    case = E.ENV_CASE
    run = E.env_run(oracle, cs)
    assert (run["ended"] == 1).any() and (run["ended"] == 2).any()
    n = case["n"]
    env = make_env(cs, obs, case)
    acts = torch.as_tensor(run["actions"]).to(DEV)
    for t in range(case["steps"]):
        o, reward, done, info = env.step(acts[t])
        assert set(info) == {"ended", "episode_length"}
        assert (reward.cpu().numpy() == run["reward"][t]).all() and (done.cpu().numpy() == run["done"][t]).all(), t
        assert (info["ended"].cpu().numpy() == run["ended"][t]).all() and (info["episode_length"].cpu().numpy() == run["length"][t]).all(), t
        assert (ops.to_aos(env.stickers, n).cpu().numpy() == run["stickers"][t]).all(), t
        if obs == "code":
            assert (ops.to_aos(o, n).cpu().numpy() == run["code"][t]).all(), t
        else:
            assert o.dtype == torch.float32 and (o.cpu().numpy() == run["onehot"][t]).all(), t
    assert (env.episode.cpu().numpy() == (run["ended"] != 0).sum(axis=0)).all()
    # reset() and init_state() start new episodes and leave the auto-reset count running; clone() carries the counters
    ep = env.episode.clone()
    twin = env.clone()
    assert torch.equal(twin.elapsed, env.elapsed) and torch.equal(twin.episode, env.episode) and twin.elapsed.data_ptr() != env.elapsed.data_ptr()
    env.reset(scramble_count=2)
    assert int(env.elapsed.abs().sum()) == 0 and torch.equal(env.episode, ep)
    env.step(acts[0])
    env.init_state()
    assert int(env.elapsed.abs().sum()) == 0 and int(twin.elapsed.sum()) > 0
    env.check_actions()


def test_vec_env_graph_replay(ops):
    """One captured step replayed 12 times with the action buffer refilled in place = 12 eager steps of a twin env; the episode
    counters advance on replay."""
    case = dict(E.ENV_CASE, n=513, max_episode_steps=4)
    n, cs = case["n"], 3
    env, twin = make_env(cs, "code", case), make_env(cs, "code", case)
    acts = torch.as_tensor(np.random.default_rng(2).integers(0, 12, size=(13, n)).astype(np.uint8)).to(DEV)
    a_buf = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        env.step(a_buf)                                              # warm-up outside the capture: one real step, the twin takes it too
    torch.cuda.current_stream().wait_stream(side)
    twin.step(acts[0])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.step(a_buf)
    for t in range(1, 13):
        a_buf.copy_(acts[t])
        g.replay()
        o2, r2, d2, i2 = twin.step(acts[t])
        same = lambda x, y: torch.equal(ops.to_aos(x, n), ops.to_aos(y, n))     # cubes < n: the pad columns of two allocations differ
        assert same(out[0], o2) and torch.equal(out[1], r2) and torch.equal(out[2], d2), t
        assert torch.equal(out[3]["ended"], i2["ended"]) and torch.equal(out[3]["episode_length"], i2["episode_length"]), t
        assert same(env.stickers, twin.stickers) and torch.equal(env.elapsed, twin.elapsed) and torch.equal(env.episode, twin.episode), t
    assert int(env.episode.max()) >= 2 and int(env.elapsed.max()) < 4


class TablePolicy(torch.nn.Module):
    """(value, logits) from an observation: a fixed random linear map of the dense one-hot, or of the first code rows."""

    def __init__(self, cs, obs, n):
        super().__init__()
        g = torch.Generator().manual_seed(4)
        self.obs, self.n, A = obs, n, C.A_OF[cs]
        R, Cc = C.RC_OF[cs]
        self.w = (torch.randn((R * Cc, A), generator=g) * 0.3).to(DEV)
        self.t = torch.randn((24, 24, A), generator=g).to(DEV)

    def forward(self, x):
        if self.obs == "onehot":
            return None, x.reshape(x.shape[0], -1) @ self.w
        from rubiks_cube_solver_amd import ops
        code = ops.to_aos(x, self.n).long()
        return None, self.t[code[:, 0], code[:, 1]]


@pytest.mark.parametrize("obs", ["onehot", "code"])
@pytest.mark.parametrize("cs", C.CUBE_SIZES)
def test_rollout_collect(ops, oracle, cs, obs):
    """collect() with a fixed generator: the returned actions replayed through the reference env reproduce reward, done and ended
    (and, with obs='code', the codes each action was chosen from)."""
    from rubiks_cube_solver_amd import rollout
    case = dict(E.ENV_CASE, n=300, steps=8, max_episode_steps=4)
    n, T = case["n"], case["steps"]
    env = make_env(cs, obs, case)
    gen = torch.Generator(device=DEV).manual_seed(17)
    out = rollout.collect(TablePolicy(cs, obs, n), env, T, generator=gen)
    assert {k: (tuple(v.shape), v.dtype) for k, v in out.items() if k != "codes"} == {
        "actions": ((T, n), torch.uint8), "reward": ((T, n), torch.float32), "done": ((T, n), torch.uint8), "ended": ((T, n), torch.uint8)}
    assert all(v.is_cuda for v in out.values()) and ("codes" in out) == (obs == "code")
    ref = E.RefEnv(oracle, cs, n, seed=case["seed"], stream_id=case["stream_id"], scramble_count=case["scramble_count"],
                   max_episode_steps=case["max_episode_steps"])
    actions = out["actions"].cpu().numpy()
    assert actions.max() < C.A_OF[cs] and len(np.unique(actions)) > 1
    code = oracle.encode(cs, ref.st)[0]
    for t in range(T):
        if obs == "code":
            assert tuple(out["codes"].shape[1:]) == tuple(env._obs_buf.shape)
            assert (ops.to_aos(out["codes"][t], n).cpu().numpy() == code).all(), t
        code, _, reward, done, ended, _ = ref.step(actions[t])
        assert (out["reward"][t].cpu().numpy() == reward).all() and (out["done"][t].cpu().numpy() == done).all(), t
        assert (out["ended"][t].cpu().numpy() == ended).all(), t
    assert (out["ended"] == 2).any()
    with pytest.raises(ValueError):
        from rubiks_cube_solver_amd.vec_env import VecCubeEnv
        rollout.collect(TablePolicy(cs, obs, n), VecCubeEnv(16, DEV, cs, obs=obs), 2)


def test_default_path_untouched(ops):
    """auto_reset=False (the default): no episode tensors, step returns an empty info dict, `active` still parks cubes."""
    from rubiks_cube_solver_amd.vec_env import VecCubeEnv
    env = VecCubeEnv(64, DEV, 3, obs="code")
    assert not env.auto_reset and not any(hasattr(env, k) for k in ("elapsed", "episode", "ended", "episode_length"))
    env.reset(scramble_count=3)
    before = env.stickers.clone()
    a = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert env.step(a, active=torch.zeros(64, dtype=torch.bool, device=DEV))[3] == {} and torch.equal(env.stickers, before)
    assert env.step(a)[3] == {} and not torch.equal(env.stickers, before)
    twin = env.clone()
    assert not hasattr(twin, "elapsed")
    auto = VecCubeEnv(64, DEV, 3, obs=None, auto_reset=True, scramble_count=1)
    with pytest.raises(ValueError):
        auto.step(a, active=torch.ones(64, dtype=torch.bool, device=DEV))
    assert auto.step(a)[0] is None
