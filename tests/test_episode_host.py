"""The rcx_* extension of librubikhip.so without a GPU: header <-> exports <-> EPISODE_SIGNATURES (the three-way check of
tests/test_native_libs.py for the new prefix), the untouched rc_* surface, the numpy restatement of the rule (tests/episode_ref.py)
against the oracle's generator, and the argument errors VecCubeEnv raises before it touches a device."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import episode_ref as E
from tests import group_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prototypes(header, prefix):
    """{function: number of parameters} of every `prefix`* prototype of a public header, comments stripped, (void) = 0."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    found = re.findall(r"^(?:int|int64_t|const char \*|void)\s*(" + prefix + r"\w+)\(([^)]*)\)", text, re.M)
    return {fn: 0 if args.strip() in ("", "void") else args.count(",") + 1 for fn, args in found}


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in nm.splitlines() if " T " in l}


def test_header_exports_and_signature_table_agree():
    from rubiks_cube_solver_amd import _build, _episode_lib, _lib, _native
    protos = prototypes("rubikepisode.h", "rcx_")
    assert set(protos) == {"rcx_episode_end", "rcx_episode_build_tag"} and protos["rcx_episode_end"] == 17
    assert prototypes("rubikepisode.h", "rc_") == {}                      # the extension declares nothing under the frozen prefix
    L = _episode_lib.episode_lib()                                          # loads without a GPU
    assert L is _lib.lib()                                                  # the same loaded library, not a second one
    names = exported(_lib.LIB_PATH)
    assert {e for e in names if e.startswith("rcx_")} == set(protos) == set(_episode_lib.EPISODE_SIGNATURES)
    for fn, n_params in protos.items():
        assert hasattr(L, fn) and len(_native.signature(_episode_lib.EPISODE_SIGNATURES[fn])[0]) == n_params, fn
    # the rc_* surface is the header's, unchanged: nothing of the extension leaked into it, and the tables do not overlap
    assert {e for e in names if e.startswith("rc_")} == set(prototypes("rubikhip.h", "rc_")) == set(_lib.SIGNATURES)
    assert not set(_lib.SIGNATURES) & set(_episode_lib.EPISODE_SIGNATURES)
    # the extension's sources are part of the library's identity, after the files that were hashed before, in their old order
    src = [os.path.basename(p) for p in _build.LIBRARIES["hip"].sources]
    assert [s for s in src if s not in ("rc_episode.h", "rubikepisode.h")] == ["rubikhip.hip", "rc_host.h", "rc_device.h", "rc_tables.h", "rc_table.h", "rc_cubies.h", "rc_edge.h",
                                                                             "rc_chain.h", "rc_ida.h", "rubikhip.h"]
    assert "rc_episode.h" in src and src[-1] == "rubikepisode.h"
    assert _episode_lib.build_tag() == _lib.build_id() == _build.source_hash(_build.LIBRARIES["hip"].sources)


@pytest.mark.parametrize("A", [6, 12])
def test_fixed_depth_draws_are_the_walk_generators(oracle, A):
    """depth_lo == depth_hi: the episode's actions are Oracle.rng_actions(seed, stream, walk, k, A) (and group_ref's restatement)."""
    for seed, stream, walk in G.RNG_TRIPLES + ((5, 3 + E.AUTO_RESET_STREAM, 2 * 1029 + 17),):
        for k in (0, 1, 3, 30):
            got_k, acts = E.episode_draws(seed, stream, walk, k, k, A)
            assert got_k == k and acts.dtype == np.uint8 and len(acts) == k
            assert (acts == oracle.rng_actions(seed, stream, walk, k, A)).all()
            assert (acts == G.rng_actions(seed, stream, walk, k, A)).all()


def test_depth_range_draw():
    """(lo, hi): every k lies in the range and a range of 4 is exhausted over 1000 walks (seed 5, the GPU test's); the depth is the
    stream's FIRST draw, the actions are the draws after it."""
    seed, stream, A = 5, 3 + E.AUTO_RESET_STREAM, 12
    ks = []
    for walk in range(1000):
        k, acts = E.episode_draws(seed, stream, walk, 1, 4, A)
        raw = E.raw_draws(seed, stream, walk, 5)
        assert 1 <= k <= 4 and k == 1 + ((raw[0] * 4) >> 32) and len(acts) == k
        assert list(acts) == [(r * A) >> 32 for r in raw[1:1 + k]]
        ks.append(k)
    assert set(ks) == {1, 2, 3, 4}
    assert min(np.bincount(ks)[1:]) > 200                                    # and about evenly: 250 each expected


def test_rule_on_a_small_batch(oracle):
    """The restated rule on hand-made counters: terminated wins over truncated, max_steps 0 never truncates, cubes that go on keep
    their stickers, ended cubes are the scramble of walk_offset + episode * walk_stride + i."""
    cs, n = 2, 6
    st = oracle.step(cs, oracle.solved(cs, n), np.arange(n, dtype=np.uint8) % 6)[0]
    done = np.array([0, 1, 0, 1, 0, 0], np.uint8)
    elapsed = np.array([0, 0, 2, 2, 5, 1], np.int32)
    episode = np.array([0, 4, 0, 1, 2, 9], np.int32)
    kw = dict(depth=2, seed=7, stream_id=1, walk_offset=100, walk_stride=10)
    out, el, ep, ended, length = E.episode_end(oracle, cs, st, done, elapsed, episode, max_steps=3, **kw)
    assert ended.tolist() == [0, 1, 2, 1, 2, 0] and length.tolist() == [0, 1, 3, 3, 6, 0]
    assert el.tolist() == [1, 0, 0, 0, 0, 2] and ep.tolist() == [0, 5, 1, 2, 3, 9]
    assert (out[[0, 5]] == st[[0, 5]]).all()
    for i in (1, 2, 3, 4):
        acts = oracle.rng_actions(7, 1, 100 + int(ep[i]) * 10 + i, 2, 6)
        want = oracle.solved(cs, 1)
        for a in acts:
            want = oracle.step(cs, want, np.array([a], np.uint8))[0]
        assert (out[i] == want[0]).all()
    assert E.episode_end(oracle, cs, st, done, elapsed, episode, max_steps=0, **kw)[3].tolist() == [0, 1, 0, 1, 0, 0]


@pytest.mark.parametrize("cs", [3, 2])
def test_env_case_has_terminated_and_truncated_episodes(oracle, cs):
    """The end-to-end case of the GPU test, on the reference alone: its seeds give both kinds of episode end, fresh cubes of every
    depth of the range, and cubes in their third episode or later."""
    run = E.env_run(oracle, cs)
    assert (run["ended"] == 1).any() and (run["ended"] == 2).any()
    assert ((run["ended"] == 1) == (run["done"] != 0)).all()
    assert (run["length"][run["ended"] == 2] == E.ENV_CASE["max_episode_steps"]).all()
    assert (run["ended"] != 0).sum(axis=0).max() >= 3


def test_vec_env_argument_errors_come_before_any_device_use():
    import torch
    from rubiks_cube_solver_amd.vec_env import VecCubeEnv
    with pytest.raises(ValueError, match="scramble_count"):
        VecCubeEnv(8, auto_reset=True)
    with pytest.raises(ValueError):
        VecCubeEnv(8, auto_reset=True, scramble_count=(3, 1))
    with pytest.raises(ValueError):
        VecCubeEnv(8, auto_reset=True, scramble_count=2, max_episode_steps=-1)
    env = object.__new__(VecCubeEnv)                                        # an env cannot be built without a device: only the flag
    env.auto_reset = True
    with pytest.raises(ValueError, match="active"):
        env.step(torch.zeros(8, dtype=torch.uint8), active=torch.ones(8, dtype=torch.bool))
