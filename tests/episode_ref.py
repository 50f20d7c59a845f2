"""The per-cube rule of include/rubikepisode.h (rcx_episode_end) restated in numpy, and a reference auto-reset env on top of it.
TEST INFRASTRUCTURE ONLY.

Moves are the CPU oracle's (oracle.oracle_np.Oracle.step); the draws are the big-int restatement of the per-walk generator in
tests/group_ref.py (splitmix64 chain + xoroshiro128+), here in a variant that returns the RAW 32-bit draws, so that the depth draw
and the action draws of one episode come out of one stream: draw 0 scaled to hi - lo + 1 (when hi > lo), the following ones to A.
"""
from __future__ import annotations

import numpy as np

from tests import group_ref as G

_M64 = (1 << 64) - 1
A_OF = G.N_ACTIONS
AUTO_RESET_STREAM = 2 ** 32            # VecCubeEnv's auto-reset draws use stream_id + 2**32


def raw_draws(seed, stream, walk, n):
    """The first n raw draws of walk (seed, stream, walk): the high 32 bits of xoroshiro128+'s outputs, as Python ints.
    group_ref.rng_actions is [(r * A) >> 32 for r in raw_draws(...)]."""
    rotl = lambda x, k: ((x << k) | (x >> (64 - k))) & _M64
    _, a = G.splitmix64(seed & _M64)
    _, b = G.splitmix64(a ^ (stream & _M64))
    st, s0 = G.splitmix64(b ^ (walk & _M64))
    _, s1 = G.splitmix64(st)
    if (s0 | s1) == 0:
        s1 = 0x9E3779B97F4A7C15
    out = []
    for _ in range(n):
        r = (s0 + s1) & _M64
        s1 ^= s0
        s0, s1 = rotl(s0, 24) ^ s1 ^ ((s1 << 16) & _M64), rotl(s1, 37)
        out.append(r >> 32)
    return out


def episode_draws(seed, stream, walk, lo, hi, A):
    """(k, actions uint8 [k]) of the episode that walk starts: k = lo (+ the first draw scaled to hi - lo + 1 when hi > lo)."""
    assert 0 <= lo <= hi
    raw = raw_draws(seed, stream, walk, hi + 1)
    k = lo
    if hi > lo:
        k += (raw[0] * (hi - lo + 1)) >> 32
        raw = raw[1:]
    return k, np.array([(r * A) >> 32 for r in raw[:k]], np.uint8)


def fresh_cubes(oracle, cs, walks, lo, hi, seed, stream):
    """[len(walks), S] stickers: the solved cube moved by each walk's episode draws (Oracle.step, one call per move depth)."""
    A = A_OF[cs]
    st = oracle.solved(cs, len(walks)).copy()
    draws = [episode_draws(seed, stream, int(w), lo, hi, A) for w in walks]
    ks = np.array([k for k, _ in draws], np.int64)
    for d in range(int(ks.max(initial=0))):
        sub = np.flatnonzero(ks > d)
        st[sub] = oracle.step(cs, st[sub], np.array([draws[i][1][d] for i in sub], np.uint8))[0]
    return st, ks


def episode_end(oracle, cs, st, done, elapsed, episode, *, max_steps, depth, seed, stream_id, walk_offset, walk_stride):
    """The rule, for every cube of [n, S] stickers.  Inputs are not modified.
    -> (stickers, elapsed, episode, ended uint8, length int32)."""
    lo, hi = (depth, depth) if isinstance(depth, int) else depth
    st, elapsed, episode = np.array(st, np.uint8), np.array(elapsed, np.int32), np.array(episode, np.int32)
    n = len(st)
    e = elapsed + 1
    terminated = np.asarray(done) != 0
    truncated = ~terminated & (max_steps > 0) & (e >= max_steps)
    over = terminated | truncated
    ended = np.where(terminated, 1, np.where(truncated, 2, 0)).astype(np.uint8)
    length = np.where(over, e, 0).astype(np.int32)
    elapsed = np.where(over, 0, e).astype(np.int32)
    episode = episode + over.astype(np.int32)
    idx = np.flatnonzero(over)
    if len(idx):
        walks = [(walk_offset + int(episode[i]) * walk_stride + int(i)) & _M64 for i in idx]
        st[idx] = fresh_cubes(oracle, cs, walks, lo, hi, seed, stream_id)[0]
    assert st.shape[0] == n
    return st, elapsed, episode, ended, length


class RefEnv:
    """VecCubeEnv(auto_reset=True) on the host: stickers [n, S], the counters, and step() by the rule above."""

    def __init__(self, oracle, cs, n, *, seed, stream_id, scramble_count, max_episode_steps):
        self.o, self.cs, self.n = oracle, cs, n
        self.seed, self.stream_id, self.depth, self.max_steps = seed, stream_id, scramble_count, max_episode_steps
        self.st = oracle.solved(cs, n).copy()
        self.elapsed = np.zeros(n, np.int32)
        self.episode = np.zeros(n, np.int32)

    def step(self, actions):
        """-> (code [n, SLOTS] and one-hot [n, R, C] of the states after any reset, reward, done, ended, length)."""
        self.st, _, done, reward = self.o.step(self.cs, self.st, np.asarray(actions, np.uint8))
        self.st, self.elapsed, self.episode, ended, length = episode_end(
            self.o, self.cs, self.st, done, self.elapsed, self.episode, max_steps=self.max_steps, depth=self.depth, seed=self.seed,
            stream_id=self.stream_id + AUTO_RESET_STREAM, walk_offset=0, walk_stride=self.n)
        code, onehot = self.o.encode(self.cs, self.st)
        return code, onehot, reward, done, ended, length


# the end-to-end case of tests/test_gpu_episode.py (checked on the CPU in tests/test_episode_host.py): host-drawn actions, the same for
# the device env and the reference env
ENV_CASE = dict(n=1029, steps=40, seed=5, stream_id=3, scramble_count=(1, 3), max_episode_steps=7, action_seed=11)
_RUNS = {}


def env_run(oracle, cs, case=None):
    """The reference env driven by the case's actions, computed once per cube size and shared (read only):
    dict(actions [T, n], stickers [T, n, S], code, onehot, reward, done, ended, length: one entry per step)."""
    case = case or ENV_CASE
    key = (cs, tuple(sorted(case.items())))
    if key not in _RUNS:
        n, T = case["n"], case["steps"]
        env = RefEnv(oracle, cs, n, seed=case["seed"], stream_id=case["stream_id"], scramble_count=case["scramble_count"],
                     max_episode_steps=case["max_episode_steps"])
        actions = np.random.default_rng(case["action_seed"]).integers(0, A_OF[cs], size=(T, n)).astype(np.uint8)
        run = {k: [] for k in ("stickers", "code", "onehot", "reward", "done", "ended", "length")}
        for t in range(T):
            code, onehot, reward, done, ended, length = env.step(actions[t])
            for k, v in zip(run, (env.st.copy(), code, onehot, reward, done, ended, length)):
                run[k].append(v)
        _RUNS[key] = dict({k: np.stack(v) for k, v in run.items()}, actions=actions)
    return _RUNS[key]
