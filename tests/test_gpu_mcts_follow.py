"""The lockstep tree search (BatchedMCTS, config 5) on the GPU, stage by stage.

  * `leaves_step` -- the device half of a simulation -- as a stage of its own: a scripted sequence of ragged path sets whose depths
    cross every replay bucket and the capacity of the pinned path block, and fall back behind a long descent; after every call the
    five outputs against the CPU oracle and the eagerly evaluated model, bit for bit, plus what the call must leave alone.
  * whole searches driven half by half (select / leaves_step / update) with tests/tree_ref.py running alongside: paths, root
    statistics, sims_used and solutions after every simulation, for the native and the Python trees, with and without hipGraph.

The model has integer-valued weights (value and logits are small multiples of 1/4 and 1/8: every fp32 sum is exact whatever the
GEMM does), so nothing here needs a tolerance.  GPU only."""
import hashlib
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_cases  # noqa: E402
import tree_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEPTHS = (0, 1, 4, 5, 16, 17, 3, 33, 2, 0, 8)      # bucket edges 4 / 8 / 16, past the 16-row capacity twice, 17 -> 3 and 33 -> 2 fall back


@pytest.fixture(scope="module")
def ops():
    from rubiks_cube_solver_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from rubiks_cube_solver_amd import _lib
    return _lib


class ExactNet(torch.nn.Module):
    """Flatten -> 32 ReLU units -> value / A logits, every weight a small integer: hidden sums stay below 2^6 and head sums below 2^11,
    exact in fp32 in any order; the heads are scaled by powers of two."""

    def __init__(self, cs, seed=0):
        super().__init__()
        R, C = (20, 24) if cs == 3 else (7, 21)
        A = tree_cases.GEOMETRY[cs][0]
        g = np.random.default_rng([seed, cs])
        self.w1 = torch.nn.Parameter(torch.tensor(g.integers(-2, 3, (R * C, 32)).astype(np.float32)), requires_grad=False)
        self.wv = torch.nn.Parameter(torch.tensor(g.integers(-1, 2, (32, 1)).astype(np.float32)), requires_grad=False)
        self.wp = torch.nn.Parameter(torch.tensor(g.integers(-1, 2, (32, A)).astype(np.float32)), requires_grad=False)

    def forward(self, x):
        h = torch.relu(x.reshape(x.shape[0], -1) @ self.w1)
        return (h @ self.wv) * 0.25, (h @ self.wp) * 0.125


def eager(net, onehot_u8):
    """(value [n], policy [n, A]) of the model evaluated eagerly on [n, R, C] float32 one-hots built from the oracle's codes."""
    with torch.no_grad():
        x = torch.from_numpy(onehot_u8).to(DEV).float()
        value, logits = net(x)
        return value.reshape(-1).cpu().numpy(), torch.softmax(logits, dim=-1).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ragged_paths(rng, n, depth, A):
    """[n, depth] no-op padded descents of every length 0 .. depth: row 0 is a full one, row 1 (if any) all no-op -- a finished root."""
    lens = rng.integers(0, depth + 1, n)
    lens[0] = depth
    if n > 1:
        lens[1] = 0
    paths = rng.integers(0, A, (n, depth), dtype=np.uint8)
    paths[np.arange(depth)[None, :] >= lens[:, None]] = A
    return paths


def gaps_of(bm):
    """Mask of the bytes of the packed result block that belong to no result array (the 256-byte alignment gaps)."""
    block = bm._pack_host.numpy()
    base = block.__array_interface__["data"][0]
    free = np.ones(block.size, bool)
    for a in bm._host:
        off = a.__array_interface__["data"][0] - base
        assert 0 <= off and off + a.nbytes <= block.size and off % 256 == 0
        free[off:off + a.nbytes] = False
    return free


def check_outputs(out, n, cs, want, copy):
    A, SL = tree_cases.GEOMETRY[cs]
    code, cc, so, value, policy = out
    assert code.shape == (n, SL) and cc.shape == (n, A, SL) and so.shape == (n, A) and value.shape == (n,) and policy.shape == (n, A)
    assert code.dtype == np.uint8 and cc.dtype == np.uint8 and so.dtype == (bool if copy else np.uint8)
    assert value.dtype == np.float32 and policy.dtype == np.float32
    assert (code == want[0]).all() and (cc == want[1]).all() and (so.astype(np.uint8) == want[2]).all()
    assert (bits(value) == bits(want[3])).all(), ("value", int(np.abs(bits(value).astype(np.int64) - bits(want[3]).astype(np.int64)).max()))
    assert (bits(policy) == bits(want[4])).all(), ("policy ulps", int(np.abs(bits(policy).astype(np.int64) - bits(want[4]).astype(np.int64)).max()))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("n,tile", [(1, None), (3, 512), (513, None), (513, 512), (1029, None), (1029, 512)])
@pytest.mark.parametrize("cs", [3, 2])
def test_leaves_step_stage(ops, L, oracle, cs, n, tile, graph):
    from rubiks_cube_solver_amd.mcts_batched import BatchedMCTS
    A, SL = tree_cases.GEOMETRY[cs]
    cubes = tree_cases.Cubes(oracle, cs, n, seed=11, depths=[1 + r % 9 for r in range(n)])
    roots = ops.from_aos(cubes.roots, DEV, tile)
    assert roots.shape[-1] == (tile or L.pitch_for(n)) and roots.shape[0] == -(-n // roots.shape[-1])
    snap = roots.clone()
    net = ExactNet(cs).to(DEV)
    bm = BatchedMCTS(net, roots, n, cs, graph=graph, native=False)
    free = gaps_of(bm)
    rng = np.random.default_rng([cs, n, int(graph)])
    kept = None                                                  # (copy=True results of the call before, what they must still be)
    for i, depth in enumerate(DEPTHS):
        paths = ragged_paths(rng, n, depth, A)
        copy = i % 2 == 0
        out = bm.leaves_step(paths, copy=copy)
        st, code, cc, so, _ = cubes.leaves(paths, track=False)
        _, onehot = oracle.encode(cs, st)
        value, policy = eager(net, onehot)
        want = (code, cc, so, value, policy)
        check_outputs(out, n, cs, want, copy)                     # leaf code, child codes, flags, value, policy: bit for bit
        block = bm._pack_host.numpy()
        assert all(np.shares_memory(a, block) != copy for a in out)           # copy=False: views of the pinned block
        if kept is not None:                                      # the copies of the call before outlive this call
            check_outputs(kept[0], n, cs, kept[1], True)
        kept = (out, want) if copy else None
        assert torch.equal(bm.roots, snap)                        # the roots are read only
        assert (ops.to_aos(bm.work, n).cpu().numpy() == st).all()  # work holds the leaves
        assert not block[free].any() and not bm._pack_dev.cpu().numpy()[free].any()       # the gaps of the packed block
        assert (bm._paths_np[:, n:] == A).all()                   # pad columns of the pinned path block
        # the pinned block: 16 rows, doubled when a descent is longer -- and the graphs captured on the old block are gone
        cap = max(16, 1 << max(max(DEPTHS[:i + 1]) - 1, 0).bit_length())
        assert bm._paths.shape == (cap, L.pitch_for(n)) and bm._paths.is_pinned()
        if graph:
            bucket = 0 if depth == 0 else max(4, 1 << (depth - 1).bit_length())
            assert bucket in bm._graphs and all(b <= cap for b in bm._graphs)
            if depth in (17, 33):
                assert set(bm._graphs) == {bucket}
    assert L.read_status() == 0


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("cs", [3, 2])
def test_bad_action_is_reported_not_followed(ops, L, oracle, cs, native):
    """A byte above the no-op in a path: that cube's leaf is unspecified (include/rubikhip.h), every other row is untouched by it,
    RC_STATUS_BAD_ACTION is set, and simulate() raises IndexError at its next multiple of 16 simulations.  An ordinary error path."""
    from rubiks_cube_solver_amd.mcts_batched import BatchedMCTS
    A, SL = tree_cases.GEOMETRY[cs]
    n = 8
    cubes = tree_cases.Cubes(oracle, cs, n, seed=5, depths=[6] * n)
    bm = BatchedMCTS(ExactNet(cs).to(DEV), ops.from_aos(cubes.roots, DEV), n, cs, rngs=[random.Random(r) for r in range(n)], native=native)
    L.read_status()
    paths = np.full((n, 3), A, np.uint8)
    paths[:, 0] = np.arange(n) % A
    bm.leaves_step(paths)
    assert L.read_status() == 0
    paths[5, 1] = A + 1
    out = bm.leaves_step(paths)
    want = cubes.leaves(np.where(paths > A, A, paths).astype(np.uint8))
    others = np.arange(n) != 5
    assert (out[0][others] == want[1][others]).all() and (out[1][others] == want[2][others]).all()
    assert L.read_status() & L.STATUS_BAD_ACTION and L.read_status() == 0    # read and cleared
    bm.leaves_step(paths)                                                    # set again; the search finds it at simulation 16
    for _ in range(15):
        bm.simulate()
    with pytest.raises(IndexError):
        bm.simulate()
    assert L.read_status() == 0


_AGREE = {}          # (cube, constants) -> digest of everything compared in a followed search: the four tree / graph combinations agree


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
@pytest.mark.parametrize("consts", [(1.0, 150.0, -10.0), (0.3, 300.0, -10.0)], ids=["c1-vl150", "c0.3-vl300"])
@pytest.mark.parametrize("cs", [3, 2])
def test_lockstep_search_follows_the_rule(ops, L, oracle, cs, consts, native, graph):
    from rubiks_cube_solver_amd.mcts_batched import BatchedMCTS
    A, SL = tree_cases.GEOMETRY[cs]
    n, sims = 64, 60
    c, vl, vmin = consts
    cubes = tree_cases.Cubes(oracle, cs, n, seed=21)             # 6, 5, 4, 3, 2, 1, 6, ... moves from solved
    net = ExactNet(cs, seed=1).to(DEV)
    bm = BatchedMCTS(net, ops.from_aos(cubes.roots, DEV), n, cs, cpuct=c, virtual_loss=vl, value_min=vmin,
                     rngs=[random.Random(900 + r) for r in range(n)], graph=graph, native=native)
    ref = tree_ref.TreeRef(n, A, c, vl, vmin, [random.Random(900 + r) for r in range(n)])
    digest = hashlib.sha256()
    seen = {}
    if not native:
        step = bm.leaves_step

        def spy(paths, copy=True):                                # the Python tree runs its own halves: watch the device step
            seen["paths"] = paths.copy()
            seen["out"] = step(paths, copy=copy)
            return seen["out"]
        bm.leaves_step = spy
    L.read_status()
    for sim in range(sims):
        want_paths = ref.select()
        was_open = [ref.solution(r) is None for r in range(n)]
        if native:
            paths = bm.native.select()
            out = bm.leaves_step(paths, copy=False)
        else:
            bm.simulate()
            paths, out = seen["paths"], seen["out"]
        assert paths.dtype == np.uint8 and paths.shape == want_paths.shape and paths.tobytes() == want_paths.tobytes(), sim
        st, code, cc, so, _ = cubes.leaves(want_paths, track=False)
        value, policy = eager(net, oracle.encode(cs, st)[1])
        check_outputs(out, n, cs, (code, cc, so, value, policy), copy=not native)
        done = ref.update(code, cc, so, out[3], out[4])           # the oracle's codes and flags, the device's own value and policy
        if native:
            assert bm.native.update(*out) == done, sim
            sims_used = bm.native.sims_used().tolist()
        else:
            sims_used = list(bm.sims_used)
        assert sims_used == ref.sims_used(), sim
        for r in range(n):
            if native:
                visits, values, nodes = bm.native.root_stats(r)
                sol = bm.native.solution(r)
            else:
                root = bm.trees[r][b"root"]
                visits, values, nodes, sol = root.visits, root.value, len({id(v) for v in bm.trees[r].values()}), bm.solution[r]
            want = ref.root_stats(r)
            assert list(visits) == want[0] and [float(v) for v in values] == want[1] and nodes == want[2], (sim, r)
            assert sol == ref.solution(r), (sim, r)
            if was_open[r] and sol is not None:                   # finished by this simulation: its path plus the solved action
                path = [int(a) for a in want_paths[r] if a != A]
                assert sol[:-1] == path and len(sol) == len(path) + 1 and so[r, sol[-1]] and not so[r, :sol[-1]].any(), (sim, r)
            digest.update(repr((visits, [float(v) for v in values], nodes, sol)).encode())
        digest.update(paths.tobytes() + bits(out[3]).tobytes() + bits(out[4]).tobytes() + repr(sims_used).encode())
    assert L.read_status() == 0
    for r in range(n):
        sol = ref.solution(r)
        if cubes.depths[r] == 1:                                  # solved by the first expansion
            assert sol is not None and len(sol) == 1 and ref.sims_used()[r] == 1, r
        if sol is not None:
            assert cubes.replay_solves(r, sol), r
    k = ref.count
    assert k["transposition"] > 0 and k["cycle"] > 0 and k["finished_early"] > 0 and 0 < ref.finished() < n, (k, ref.finished())
    assert (k["residual"] > 0) == (vl != 150.0), k
    assert _AGREE.setdefault((cs, consts), digest.hexdigest()) == digest.hexdigest()
