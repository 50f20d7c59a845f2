"""The beam search where tests/test_gpu_search.py does not reach (rubiks-cube-solver_amd/search.py, librubiksearch.so):

  lockstep     a BeamPlan driven stage by stage next to beam_ref.Stepper, every buffer compared exactly after every stage; the
               restated select is fed the DEVICE's own scores, so a real net (fp32 / bf16) is followed bit for bit
  shapes       tiled roots (n > root_pitch), W = 32769 and 65536 (parent slots above 32767 in int16 storage), 1000 x 1024, 10 000 x 16
  scores       random bit patterns, neighbours a few ulps apart, blocks of equal scores, +-FLT_MAX, denormals (beam_ref.hard_scores)
  chunks       BeamPlan.score with several chunks and a ragged last one against the one-chunk plan and onehot @ w
  errors       every argument the header or the source rejects, and that a rejected call writes nothing
GPU only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import beam_ref  # noqa: E402
import test_gpu_search as base  # noqa: E402  (Stub, DeepCube, env_of, scrambles, replay_ok: helpers only, nothing is re-collected)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def search_mod():
    from rubiks_cube_solver_amd import search
    return search


def cand_j(plan, p, n_c):
    """flat index j = a * NBp + b of the candidates c = 0..n_c-1 of problem p (include/rubiksearch.h)."""
    c = np.arange(n_c)
    return (c % plan.A) * plan.nbp + p * plan.W + c // plan.A


def host_codes(plan):
    """plan.code -> [A * NBp, SLOTS] numpy, row j."""
    return plan.code.view(plan.A, plan.tiles, plan.SL, plan.pitch).permute(0, 1, 3, 2).reshape(plan.A * plan.nbp, plan.SL).cpu().numpy()


def u16(t):
    return t.cpu().numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------- the lockstep harness
class Lockstep:
    """One BeamPlan and one beam_ref.Stepper side by side.  Problem i of the stepper is problem sub[i] of the plan (problems are
    independent: a subset of a large batch is restated, the device runs all of them)."""

    def __init__(self, cs, roots_np, roots_dev, root_pitch, W, D, model, dtype=torch.float32, sub=None, budget=1 << 30):
        self.cube = beam_ref.Cube(cs)
        self.P = len(roots_np)
        self.sub = np.arange(self.P) if sub is None else np.asarray(sub)
        self.roots, self.model = roots_np, model
        self.plan = search_mod().BeamPlan(self.P, cs, W, D, DEV, dtype, budget)
        self.st = beam_ref.Stepper(self.cube, roots_np[self.sub], W, D)
        self.plan.init(roots_dev, root_pitch)
        self.check_init()
        self.trace = []                                             # (live, active) of the restated side after every depth

    def state(self):
        pl = self.plan
        return pl.live.cpu().numpy(), pl.active.cpu().numpy(), pl.length.cpu().numpy(), pl.solution.cpu().numpy()

    def check_init(self):
        pl, st, sub, A = self.plan, self.st, self.sub, self.cube.A
        torch.cuda.synchronize()
        beam = base.to_aos_beam(pl, pl.beams[0])
        assert (beam[sub * pl.W] == self.roots[sub]).all()
        assert (pl.last_action.cpu().numpy()[sub * pl.W] == A).all()
        live, active, length, sol = self.state()
        assert (live[sub] == st.live).all() and (active[sub] == st.active).all()
        assert (length[sub] == st.length).all() and (sol[sub] == -1).all() and (st.solution == -1).all()
        assert int(pl.depth) == 1

    def check_expand(self):
        pl, st, cube = self.plan, self.st, self.cube
        flags, codes = pl.flags.cpu().numpy().reshape(-1), host_codes(pl)
        keys = pl.keys.cpu().numpy().view(np.uint64).reshape(pl.keys.shape[0], -1)
        for i, p in enumerate(self.sub):
            cd = st.cand.get(i)
            n_live = len(cd["a"]) if cd else 0
            if cd:
                j = cand_j(pl, p, n_live)
                want = cd["valid"].astype(np.uint8) | (cd["solved"].astype(np.uint8) << 1)
                assert (flags[j] == want).all(), ("flags", st.depth, p)
                assert (codes[j] == cube.codes(cd["children"])).all(), ("codes", st.depth, p)
                assert (keys[:, j] == cd["keys"]).all(), ("keys", st.depth, p)
            dead = cand_j(pl, p, pl.W * pl.A)[n_live:]              # dead slots, inactive problems: never VALID
            assert not (flags[dead] & 1).any(), ("dead slot valid", st.depth, p)

    def host_scores(self):
        flat = self.plan.scores.cpu().numpy().reshape(-1)
        return {i: flat[cand_j(self.plan, self.sub[i], len(cd["a"]))] for i, cd in self.st.cand.items() if cd["hit"] < 0}

    def check_select(self):
        pl, st, sub = self.plan, self.st, self.sub
        flags = pl.flags.cpu().numpy().reshape(-1)
        cnt, par, act = pl.sel_count.cpu().numpy(), u16(pl.sel_parent), pl.sel_action.cpu().numpy()
        live, active, length, sol = self.state()
        assert (cnt[sub] == st.sel_count()).all(), ("sel_count", st.depth)
        assert (length[sub] == st.length).all() and (sol[sub] == st.solution).all() and (active[sub] == st.active).all(), st.depth
        for i, (kind, kept) in st.sel.items():
            if kind != "kept":
                continue
            p, cd = sub[i], st.cand[i]
            j = cand_j(pl, p, len(cd["a"]))
            assert (((flags[j] & 4) != 0) == cd["surv"]).all(), ("survivors", st.depth, p)
            assert ((flags[j] & 3) == (cd["valid"].astype(np.uint8) | (cd["solved"].astype(np.uint8) << 1))).all()
            n0 = p * pl.W
            assert (par[n0:n0 + len(kept)] == cd["w"][kept]).all() and (act[n0:n0 + len(kept)] == cd["a"][kept]).all(), ("kept", st.depth, p)

    def check_advance(self, parity, t):
        """after Stepper.advance: st.hist[t - 1] is the row of depth t."""
        pl, st, A = self.plan, self.st, self.cube.A
        out = base.to_aos_beam(pl, pl.beams[1 - parity])
        last, hp, ha = pl.last_action.cpu().numpy(), u16(pl.hist_parent[t - 1]), pl.hist_action[t - 1].cpu().numpy()
        assert (pl.live.cpu().numpy()[self.sub] == st.live).all(), ("live", t)
        for i, p in enumerate(self.sub):
            n0, n1, n2 = p * pl.W, p * pl.W + st.live[i], (p + 1) * pl.W
            assert (out[n0:n1] == st.beams[i]).all(), ("beam", t, p)
            assert (last[n0:n1] == st.last[i]).all() and (last[n1:n2] == A).all(), ("last_action", t, p)
            rp, ra = st.hist[t - 1][i]
            assert (hp[n0:n1] == rp).all() and (ha[n0:n1] == ra).all(), ("history", t, p)
            assert (hp[n1:n2] == 0).all() and (ha[n1:n2] == A).all(), ("history of dead slots", t, p)

    def run(self):
        """Every depth until nothing is active (on both sides), then backtrack.  -> what beam_search returns, from the plan."""
        pl, st = self.plan, self.st
        for t in range(1, pl.D + 1):
            parity = (t - 1) & 1
            if not st.active.any() and not bool(pl.active.any()):
                break
            st.expand()
            pl.expand(parity)
            self.check_expand()
            pl.score(self.model)
            st.select(self.host_scores())
            pl.select()
            self.check_select()
            st.advance()
            pl.advance(parity)
            self.check_advance(parity, t)
            pl.depth.add_(1)
            assert int(pl.depth) == st.depth
            self.trace.append((st.live.copy(), st.active.copy()))
        if pl.D:
            pl.backtrack()
        actions = pl.actions[:pl.D]
        assert (actions.cpu().numpy()[:, self.sub] == st.backtrack()).all(), "actions"
        return {"solved": pl.length >= 0, "length": pl.length, "actions": actions}


def same_result(a, b):
    for k in ("solved", "length", "actions"):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------- 1. real nets in lockstep
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_lockstep_random_net(dtype):
    """DeepCube with random weights, 3x3x3, 100 scrambles of 1..12 moves, W = 64, D = 12: every stage of every depth equals the
    restatement fed with the device's own scores; beam_search eager and graph=True then return exactly the lockstep result."""
    S = search_mod()
    scr = base.scrambles(3, [1 + i % 12 for i in range(100)], seed=21)
    model = base.DeepCube(base._random_deepcube(3)).to(DEV).to(dtype).eval()
    env = base.env_of(3, scr)
    with torch.no_grad():
        ls = Lockstep(3, beam_ref.Cube(3).scramble(scr), env.stickers, env.stickers.shape[-1], 64, 12, model, dtype)
        res = ls.run()
    assert max(int(l.max()) for l, _ in ls.trace) == 64 and len(ls.trace) >= 10         # the beam fills, the cut decides
    assert base.replay_ok(3, scr, res)
    same_result(res, S.beam_search(model, env, 64, 12))
    same_result(res, S.beam_search(model, env, 64, 12, graph=True))


def test_lockstep_shipped_checkpoint():
    """The authors' 2x2x2 checkpoint at W = 16 on the fixture's 40 depth-14 scrambles, in lockstep, then eager and graph."""
    S = search_mod()
    g = np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222.npz"))
    with np.load(os.path.join(ROOT, "tests", "golden", "crosscheck_222_weights.npz")) as z:
        sd = {k: z[k] for k in z.files}
    scr = g["scramble"][g["ks"] == 14].astype(np.uint8)
    assert len(scr) == 40
    model = base.DeepCube(sd).to(DEV).eval()
    env = base.env_of(2, scr)
    with torch.no_grad():
        ls = Lockstep(2, beam_ref.Cube(2).scramble(scr), env.stickers, env.stickers.shape[-1], 16, 30, model)
        res = ls.run()
    assert bool(res["solved"].all()) and base.replay_ok(2, scr, res)
    assert len(ls.trace) == int(res["length"].max()) >= 8                                 # every depth up to the last solution was compared
    same_result(res, S.beam_search(model, env, 16, 30))
    same_result(res, S.beam_search(model, env, 16, 30, graph=True))


# ------------------------------------------------------------------------------------------- 2. the scores themselves
def test_scores_match_float64_value_head():
    """fp32 DeepCube (random weights), 3x3x3, 100 scrambles of 4..12 moves, W = 256: nothing is cut before depth 3 (at most 12,
    then 132 slots), so the depth-3 candidates do not depend on any score.  plan.scores of every candidate of a live slot of an
    active problem (valid or not; dead slots and the padding are skipped) against the value head in float64 numpy on
    beam_ref.Cube.onehot of the restated children.

    Tolerance: 8 x the largest deviation of the same head in float32 numpy (beam_ref.value_head) from the float64 evaluation over
    these inputs -- a GEMM of K = 480 may sum in another order, no more.  Measured on the CPU over the 132 696 candidates (97
    active problems): float32 numpy deviates by at most 3.33e-07 (scores span -0.933 .. 0.686), so the device is allowed 2.66e-06."""
    S = search_mod()
    cube = beam_ref.Cube(3)
    sd = base._random_deepcube(3)
    scr = base.scrambles(3, [4 + i % 9 for i in range(100)], seed=22)
    roots = cube.scramble(scr)
    model = base.DeepCube(sd).to(DEV).eval()
    env = base.env_of(3, scr)
    plan = S.BeamPlan(100, 3, 256, 3, DEV)
    st = beam_ref.Stepper(cube, roots, 256, 3)
    with torch.no_grad():
        plan.init(env.stickers, env.stickers.shape[-1])
        for t in (1, 2):
            plan.step(model, (t - 1) & 1)
            st.expand()
            st.select({p: np.zeros(len(cd["a"]), np.float32) for p, cd in st.cand.items()})    # fewer than W survivors: all are kept
            assert all(len(kept) < 256 for kind, kept in st.sel.values() if kind == "kept")
            st.advance()
        plan.expand(0)
        plan.score(model)
    torch.cuda.synchronize()
    assert (plan.live.cpu().numpy() == st.live).all() and (plan.active.cpu().numpy() == st.active).all()
    st.expand()
    flat = plan.scores.cpu().numpy().reshape(-1)
    got = np.concatenate([flat[cand_j(plan, p, len(cd["a"]))] for p, cd in st.cand.items()])
    x = cube.onehot(np.concatenate([cd["children"] for cd in st.cand.values()]))
    want64 = beam_ref.value_head({k: v.astype(np.float64) for k, v in sd.items()}, x.astype(np.float64))
    ref32 = beam_ref.value_head(sd, x)
    assert want64.dtype == np.float64 and ref32.dtype == np.float32 and len(got) > 100000
    dev32 = float(np.abs(ref32.astype(np.float64) - want64).max())
    dev_gpu = float(np.abs(got.astype(np.float64) - want64).max())
    print(f"candidates {len(got)}  float32 numpy vs float64: {dev32:.3e}  device vs float64: {dev_gpu:.3e}  scores {want64.min():.3f} .. {want64.max():.3f}")
    assert 0 < dev32 < 1e-5
    assert dev_gpu <= 8 * dev32, (dev_gpu, dev32)


# ------------------------------------------------------------------------------------------- 3. the widest beam
def test_lockstep_width_65536():
    """Stub, 3x3x3, P = 2, W = 65536, D = 7, roots scrambled 14 moves: the beam is full from depth 5 on, so the parent slots above
    32767 are live from depth 6 and the history rows 5 and 6 hold them (uint16 on the device, int16 storage on the host)."""
    S = search_mod()
    scr = np.random.default_rng(4).integers(0, 12, (2, 14)).astype(np.uint8)
    model = base.Stub(3).to(DEV)
    env = base.env_of(3, scr)
    with torch.no_grad():
        ls = Lockstep(3, beam_ref.Cube(3).scramble(scr), env.stickers, env.stickers.shape[-1], 65536, 7, model)
        res = ls.run()
    assert len(ls.trace) == 7
    assert [int(l[0]) for l, _ in ls.trace[:2]] == [12, 114]                              # nothing is cut yet: every distinct state
    for t in (5, 6, 7):
        live, active = ls.trace[t - 1]
        assert (live == 65536).all() and active.all(), t                                  # full and still searching
    for t in (6, 7):
        assert all(int(ls.st.hist[t - 1][p][0].max()) > 32767 for p in range(2)), t       # parents above int16's range are live
    assert (res["length"].cpu().numpy() == -1).all()
    same_result(res, S.beam_search(model, env, 65536, 7))


# ------------------------------------------------------------------------------------------- 4. tiled roots
def test_lockstep_40000_problems_from_two_root_tiles():
    """Stub, P = 40 000, W = 2, D = 6, roots straight from a VecCubeEnv (two tiles of 32768: the n > root_pitch branch of
    rc_search_init).  The restated side follows the first 64, the last 64, the 128 around cube 32768 and 256 drawn at random;
    every one of the 40 000 solutions is replayed."""
    P = 40000
    rng = np.random.default_rng(40)
    counts = rng.integers(0, 7, P)
    counts[[0, 1, 32766, 32767, 32768, 32769, P - 1]] = [0, 3, 0, 2, 0, 1, 0]              # solved roots on both sides of the boundary
    scr = base.scrambles(3, counts.tolist(), seed=41)
    env = base.env_of(3, scr)
    assert env.stickers.shape[0] == 2 and env.stickers.shape[-1] == 32768
    sub = np.unique(np.concatenate([np.arange(64), np.arange(P - 64, P), np.arange(32768 - 64, 32768 + 64), rng.choice(P, 256, replace=False)]))
    roots = beam_ref.Cube(3).scramble(scr)
    with torch.no_grad():
        ls = Lockstep(3, roots, env.stickers, env.stickers.shape[-1], 2, 6, base.Stub(3).to(DEV), sub=sub)
        res = ls.run()
    L = res["length"].cpu().numpy()
    assert (L[counts == 0] == 0).all() and (L[counts == 1] <= 1).all()
    assert (L >= 0).sum() > P // 4 and (L < 0).sum() > 100 and (L[sub] < 0).sum() > 5 and (L[sub] > 1).sum() > 5
    assert base.replay_ok(3, scr, res)


@pytest.mark.parametrize("cs", [3, 2])
@pytest.mark.parametrize("root_pitch", [512, 1024])
def test_init_from_tiled_roots(cs, root_pitch):
    """rc_search_init on 1300 roots in tiles of 512 and of 1024, solved roots on both sides of the tile boundaries."""
    from rubiks_cube_solver_amd import ops
    S = search_mod()
    cube = beam_ref.Cube(cs)
    n, W = 1300, 3
    counts = np.random.default_rng(root_pitch).integers(1, 9, n)
    counts[[0, 511, 512, 513, 1023, 1024, 1025, 1299]] = 0
    roots = cube.scramble(base.scrambles(cs, counts.tolist(), seed=cs))
    dev = ops.alloc_states(n, cs, DEV, pitch=root_pitch)
    assert dev.shape == (-(-n // root_pitch), cube.S, root_pitch)
    dev.copy_(ops.from_aos(roots, DEV, root_pitch))
    plan = S.BeamPlan(n, cs, W, 1, DEV)
    for t in (plan.beams[0], plan.last_action, plan.live, plan.active, plan.length, plan.solution):
        t.view(torch.uint8).fill_(0x5A)
    plan.init(dev, root_pitch)
    torch.cuda.synchronize()
    st = beam_ref.Stepper(cube, roots, W, 1)
    beam, last = base.to_aos_beam(plan, plan.beams[0]), plan.last_action.cpu().numpy()
    slot0 = np.arange(n) * W
    assert (beam[slot0] == roots).all() and (last[slot0] == cube.A).all()
    assert (np.delete(beam, slot0, 0) == 0x5A).all() and (np.delete(last, slot0) == 0x5A).all()      # only slot 0 is written
    solved = cube.is_solved(roots)
    assert solved.sum() >= 8
    assert (plan.live.cpu().numpy() == st.live).all() and (st.live == ~solved).all()
    assert (plan.active.cpu().numpy() == st.active).all() and (plan.length.cpu().numpy() == st.length).all()
    assert (st.length == np.where(solved, 0, -1)).all() and (plan.solution.cpu().numpy() == -1).all()


# ------------------------------------------------------------------------------------------- 5. real-valued scores in the select
def run_select_case(cs, W, P, seed, force_last=False):
    """Synthetic candidates with beam_ref.hard_scores: problem p uses mode p % 5; duplicate keys, ragged live, an inactive problem,
    one with nothing live, one with a solved candidate.  force_last: the candidates of the last slot W - 1 are valid, distinct and
    score +inf, so the highest parent slot is certainly kept.  Every output of rc_search_select against beam_ref.select_problem."""
    S = search_mod()
    A = 12 if cs == 3 else 6
    plan = S.BeamPlan(P, cs, W, 4, DEV, dense_budget_bytes=1 << 20)
    rng = np.random.default_rng(seed)
    KW = plan.keys.shape[0]
    live = rng.integers(max(1, W // 2), W + 1, P).astype(np.int32)
    live[:5] = W                                                     # every mode once with a full beam: survivors > W, the radix passes run
    active = np.ones(P, np.uint8)
    if P >= 9:
        live[6], active[7] = 0, 0
    flags = np.zeros(A * plan.nbp, np.uint8)
    keys = np.zeros((KW, A * plan.nbp), np.uint64)
    scores = np.zeros(A * plan.nbp, np.float32)
    pool = rng.integers(0, 2 ** 48, (KW, max(4, W * A // 3)), dtype=np.uint64)
    for p in range(P):
        n = int(live[p]) * A
        j = cand_j(plan, p, n)
        flags[j] = (rng.random(n) < 0.85) * (active[p] == 1)
        keys[:, j] = pool[:, rng.integers(0, pool.shape[1], n)] if p % 2 else rng.integers(0, 2 ** 48, (KW, n), dtype=np.uint64)
        scores[j] = beam_ref.hard_scores(rng, n, W, p % 5)
        if force_last and live[p] == W:
            flags[j[-A:]], scores[j[-A:]] = 1, np.inf
            keys[:, j[-A:]] = np.arange(A, dtype=np.uint64) + np.uint64(1 << 50)           # outside the pool: survivors
    if P >= 9:
        flags[cand_j(plan, 8, A)[2]] |= 3                            # problem 8: a valid solved candidate
    plan.flags.copy_(torch.tensor(flags).view(A, -1))
    plan.keys.copy_(torch.tensor(keys.view(np.int64)).view(KW, A, -1))
    plan.scores.copy_(torch.tensor(scores).view(A, -1))
    plan.live.copy_(torch.tensor(live))
    plan.active.copy_(torch.tensor(active))
    plan.length.fill_(-1)
    plan.solution.fill_(-1)
    plan.depth.fill_(3)
    plan.sel_parent.fill_(-1)
    plan.select()
    torch.cuda.synchronize()
    got_flags = plan.flags.cpu().numpy().reshape(-1)
    cnt, par, act = plan.sel_count.cpu().numpy(), u16(plan.sel_parent), plan.sel_action.cpu().numpy()
    length, sol, act_after = plan.length.cpu().numpy(), plan.solution.cpu().numpy(), plan.active.cpu().numpy()
    cut = 0
    for p in range(P):
        if not active[p]:
            assert cnt[p] == 0 and length[p] == -1 and act_after[p] == 0
            continue
        j = cand_j(plan, p, int(live[p]) * A)
        kind, res, surv = beam_ref.select_problem(flags[j] & 1, flags[j] & 2, keys[:, j], scores[j], W)
        if kind == "solved":
            assert length[p] == 3 and sol[p] == res and act_after[p] == 0 and cnt[p] == 0, p
            continue
        assert act_after[p] == 1 and length[p] == -1 and sol[p] == -1
        assert (((got_flags[j] & 4) != 0) == surv).all(), p
        assert cnt[p] == len(res), (p, cnt[p], len(res))
        cut += int(surv.sum()) > W
        n0 = p * W
        assert (par[n0:n0 + cnt[p]] == res // A).all() and (act[n0:n0 + cnt[p]] == res % A).all(), ("kept", p, p % 5)
    assert cut >= min(P, 5), cut                                     # more survivors than W for every mode: the radix passes ran
    return plan


@pytest.mark.parametrize("cs,W", [(3, 1), (2, 255), (3, 256), (2, 257), (3, 4096)])
def test_select_real_valued_scores(cs, W):
    """rc_search_select with scores whose low mantissa bytes decide (beam_ref.hard_scores; beam_ref.rank_order, pinned on the CPU
    by tests/test_search_host.py, is the reference)."""
    run_select_case(cs, W, 11, seed=W)


# ------------------------------------------------------------------------------------------- 6. parent slots above 32767
@pytest.mark.parametrize("W", [32769, 65536])
def test_wide_select_advance_backtrack(W):
    """P = 3: select with hard scores, then advance and backtrack with sel_parent / hist_parent values over the whole range
    including 32768 and W - 1, written and read through the int16 tensors the plan owns; expectations in numpy on uint16 views."""
    cs, P, D = 3, 3, 3
    cube = beam_ref.Cube(cs)
    A = cube.A
    plan = run_select_case(cs, W, P, seed=W, force_last=True)
    assert plan.sel_parent.dtype == torch.int16 and plan.hist_parent.dtype == torch.int16
    cnt = plan.sel_count.cpu().numpy()
    assert (cnt == W).all() and (u16(plan.sel_parent)[np.arange(P) * W + W - 1] == W - 1).all()      # the select itself wrote slot W - 1
    plan = None
    torch.cuda.empty_cache()
    plan = search_mod().BeamPlan(P, cs, W, D, DEV, dense_budget_bytes=1 << 20)
    rng = np.random.default_rng(W)
    nb = P * W
    aos = np.zeros((plan.nbp, cube.S), np.uint8)
    aos[:nb] = cube.scramble(rng.integers(0, A, (nb, 5)))
    plan.beams[0].copy_(base.from_aos_beam(plan, aos))
    cnt = np.array([W, W - 1, W // 2 + 3], np.int32)
    par = rng.integers(0, W, plan.nbp).astype(np.uint16)
    par[[0, 1, 2, W, W + 1, 2 * W]] = [W - 1, 32768, 32767, 32768, W - 1, W - 1]
    act = rng.integers(0, A, plan.nbp).astype(np.uint8)
    plan.sel_count.copy_(torch.tensor(cnt))
    plan.sel_parent.copy_(torch.tensor(par.view(np.int16)))
    plan.sel_action.copy_(torch.tensor(act))
    plan.depth.fill_(2)
    plan.advance(0)
    torch.cuda.synchronize()
    out = base.to_aos_beam(plan, plan.beams[1])
    hp, ha, last = u16(plan.hist_parent), plan.hist_action.cpu().numpy(), plan.last_action.cpu().numpy()
    assert (plan.live.cpu().numpy() == cnt).all()
    for p in range(P):
        n = p * W + np.arange(cnt[p])
        assert (par[n] > 32767).sum() > (cnt[p] // 3 if W == 65536 else 0)
        assert (out[n] == cube.move(aos[p * W + par[n].astype(np.int64)], act[n])).all(), p
        assert (last[n] == act[n]).all() and (hp[1, n] == par[n]).all() and (ha[1, n] == act[n]).all(), p
        dead = np.arange(p * W + cnt[p], (p + 1) * W)
        assert (out[dead] == aos[dead]).all() and (last[dead] == A).all() and (hp[1, dead] == 0).all() and (ha[1, dead] == A).all(), p
    hp = rng.integers(0, W, (D, plan.nbp)).astype(np.uint16)
    ha = rng.integers(0, A, (D, plan.nbp)).astype(np.uint8)
    length = np.array([D, D, D - 1], np.int32)
    sol = np.array([(W - 1) * A + 5, 32768 * A, 40000 % W * A + 1], np.int32)
    hp[D - 2, 0 * W + W - 1] = W - 1                                  # problem 0 walks through slot W - 1 twice, problem 1 through 32768
    hp[D - 2, 1 * W + 32768] = 32768
    plan.hist_parent.copy_(torch.tensor(hp.view(np.int16)))
    plan.hist_action.copy_(torch.tensor(ha))
    plan.length.copy_(torch.tensor(length))
    plan.solution.copy_(torch.tensor(sol))
    plan.backtrack()
    got = plan.actions.cpu().numpy()
    for p in range(P):
        want = np.full(D, A, np.uint8)
        L = length[p]
        w, want[L - 1] = int(sol[p]) // A, sol[p] % A
        for t in range(L - 1, 0, -1):
            want[t - 1], w = ha[t - 1, p * W + w], int(hp[t - 1, p * W + w])
        assert (got[:, p] == want).all(), p


# ------------------------------------------------------------------------------------------- 7. the shapes the README quotes
@pytest.mark.parametrize("cs,P,W", [(3, 1000, 1024), (2, 10000, 16)])
def test_quoted_shapes_stage_by_stage(cs, P, W):
    """Expand, select and advance once each at 1000 x 1024 (12.6 M candidates) and 10 000 x 16 against the vectorised restatement;
    the select is compared for every problem.  Slots of a problem are drawn from a pool of W / 2 states, so equal children abound;
    some problems hold a slot one move from solved."""
    S = search_mod()
    cube = beam_ref.Cube(cs)
    A = cube.A
    plan = S.BeamPlan(P, cs, W, 2, DEV, dense_budget_bytes=1 << 20)   # nothing is scored by a net here
    KW = plan.keys.shape[0]
    rng = np.random.default_rng(P)
    nb = P * W
    states = cube.scramble(rng.integers(0, A, (nb, 6)))
    aos = np.zeros((plan.nbp, cube.S), np.uint8)
    aos[:nb] = states[np.arange(nb) // W * W + rng.integers(0, max(W // 2, 1), nb)]
    near = rng.choice(P, P // 20, replace=False)                      # one move from solved in slot 1
    aos[near * W + 1] = cube.scramble(rng.integers(0, A, (len(near), 1)))
    live = rng.integers(0, W + 1, P).astype(np.int32)
    live[0], live[-1], live[near] = 0, W, np.maximum(live[near], 2)
    active = (rng.random(P) < 0.9).astype(np.uint8)
    last = rng.integers(0, A + 1, plan.nbp).astype(np.uint8)
    plan.beams[0].copy_(base.from_aos_beam(plan, aos))
    plan.live.copy_(torch.tensor(live))
    plan.active.copy_(torch.tensor(active))
    plan.last_action.copy_(torch.tensor(last))
    plan.length.fill_(-1)
    plan.solution.fill_(-1)
    plan.depth.fill_(1)
    # expand
    plan.expand(0)
    torch.cuda.synchronize()
    b = np.arange(nb)
    pp, ww = b // W, b % W
    flags = plan.flags.cpu().numpy()[:, :nb]
    code = host_codes(plan).reshape(A, plan.nbp, plan.SL)[:, :nb]
    keys = plan.keys.cpu().numpy().view(np.uint64)[:, :, :nb]
    wflags, wkeys = np.zeros((A, nb), np.uint8), np.zeros((KW, A, nb), np.uint64)
    for a in range(A):
        ch = cube.move(aos[:nb], np.full(nb, a))
        valid = (active[pp] == 1) & (ww < live[pp]) & (last[:nb] != (a ^ 1))
        wflags[a] = valid.astype(np.uint8) | (cube.is_solved(ch).astype(np.uint8) << 1)
        wkeys[:, a] = cube.keys(ch)
        assert (code[a] == cube.codes(ch)).all(), a
    assert (flags == wflags).all() and (keys == wkeys).all()
    del code, keys
    # select on real-valued scores
    scores = np.zeros((A, plan.nbp), np.float32)
    for p in range(P):
        scores[:, p * W:(p + 1) * W] = beam_ref.hard_scores(rng, A * W, W, 4 if p % 3 else p // 3 % 4).reshape(A, W)
    plan.scores.copy_(torch.tensor(scores))
    plan.select()
    torch.cuda.synchronize()
    gflags = plan.flags.cpu().numpy()
    cnt, par, act = plan.sel_count.cpu().numpy(), u16(plan.sel_parent), plan.sel_action.cpu().numpy()
    length, sol, act_after = plan.length.cpu().numpy(), plan.solution.cpu().numpy(), plan.active.cpu().numpy()
    n_solved = n_cut = 0
    for p in range(P):
        if not active[p]:
            assert cnt[p] == 0 and length[p] == -1 and sol[p] == -1 and act_after[p] == 0, p
            continue
        c = np.arange(int(live[p]) * A)
        ia, ib = c % A, p * W + c // A
        kind, res, surv = beam_ref.select_problem(wflags[ia, ib] & 1, wflags[ia, ib] & 2, wkeys[:, ia, ib], scores[ia, ib], W)
        if kind == "solved":
            assert length[p] == 1 and sol[p] == res and act_after[p] == 0 and cnt[p] == 0, p
            n_solved += 1
            continue
        assert act_after[p] == 1 and length[p] == -1 and sol[p] == -1, p
        assert (((gflags[ia, ib] & 4) != 0) == surv).all(), p
        assert cnt[p] == len(res), (p, cnt[p], len(res))
        n_cut += int(surv.sum()) > W
        assert (par[p * W:p * W + cnt[p]] == res // A).all() and (act[p * W:p * W + cnt[p]] == res % A).all(), p
    assert n_solved >= P // 40 and n_cut >= P // 3, (n_solved, n_cut)
    # advance with what the device selected
    plan.advance(0)
    torch.cuda.synchronize()
    out = base.to_aos_beam(plan, plan.beams[1])[:nb]
    lastn, hp, ha = plan.last_action.cpu().numpy()[:nb], u16(plan.hist_parent)[0, :nb], plan.hist_action.cpu().numpy()[0, :nb]
    assert (plan.live.cpu().numpy() == cnt).all()
    kept = ww < cnt[pp]
    src = np.where(kept, pp * W + par[:nb].astype(np.int64), b)
    mv = np.where(kept, act[:nb], A)
    want = aos[src]
    want[kept] = cube.move(want[kept], mv[kept])
    assert (out == want).all() and (lastn == mv).all()
    assert (hp == np.where(kept, par[:nb], 0)).all() and (ha == mv).all()


# ------------------------------------------------------------------------------------------- 8. chunked scoring
def test_score_chunks_match_one_chunk_and_the_restatement():
    """BeamPlan.score alone, Stub (exact integer scores), 70 x 1000 (3 tiles, 36 candidate tiles): a budget that makes a chunk 5
    tiles (7 full chunks and one of 1 tile), a budget below one tile (36 chunks of one tile) and one chunk for everything --
    identical scores, equal to onehot(children) @ w for every candidate of a real slot."""
    S = search_mod()
    cs, P, W = 3, 70, 1000
    cube = beam_ref.Cube(cs)
    A, nb = cube.A, P * W
    w = beam_ref.stub_weights(cs)
    model = base.Stub(cs).to(DEV)
    rng = np.random.default_rng(8)
    row = cube.R * cube.C * 4
    aos = None
    got = {}
    for name, budget, chunks in (("five tiles", 5 * 32768 * row + 1000, 8), ("below one tile", 1000, 36), ("one chunk", 3 << 30, 1)):
        plan = S.BeamPlan(P, cs, W, 1, DEV, dense_budget_bytes=budget)
        assert plan.tiles == 3 and plan.pitch == 32768 and -(-A * plan.nbp // plan.chunk) == chunks, (name, plan.chunk)
        if aos is None:
            aos = np.zeros((plan.nbp, cube.S), np.uint8)
            aos[:nb] = cube.scramble(rng.integers(0, A, (nb, 7)))
            live = rng.integers(0, W + 1, P).astype(np.int32)
        plan.beams[0].copy_(base.from_aos_beam(plan, aos))
        plan.live.copy_(torch.tensor(live))
        plan.active.fill_(1)
        plan.last_action.fill_(A)
        plan.scores.fill_(float("nan"))
        plan.expand(0)
        with torch.no_grad():
            plan.score(model)
        torch.cuda.synchronize()
        got[name] = plan.scores.cpu().numpy()
        plan = None
        torch.cuda.empty_cache()
    for a in range(A):
        want = cube.onehot(cube.move(aos[:nb], np.full(nb, a))).reshape(nb, -1) @ w
        assert want.dtype == np.float32 and len(np.unique(want)) > 100
        for name, sc in got.items():
            assert (sc[a, :nb] == want).all(), (name, a, np.flatnonzero(sc[a, :nb] != want)[:5])
    assert (got["five tiles"][:, :nb] == got["one chunk"][:, :nb]).all() and (got["below one tile"][:, :nb] == got["one chunk"][:, :nb]).all()


@pytest.mark.parametrize("cs,W", [(3, 64), (2, 16)])
def test_search_equals_restatement_exactly_with_small_chunks(cs, W):
    """test_search_equals_restatement_exactly with a dense budget below one tile: every depth is scored in A one-tile chunks."""
    S = search_mod()
    scr = base.scrambles(cs, [k for k in range(1, 9) for _ in range(32)], seed=cs)
    res = S.beam_search(base.Stub(cs).to(DEV), base.env_of(cs, scr), W, 10, dense_budget_bytes=1000)
    want = base.ref_search(cs, scr, W, 10)
    assert (res["solved"].cpu().numpy() == want["solved"]).all()
    assert (res["length"].cpu().numpy() == want["length"]).all()
    assert (res["actions"].cpu().numpy() == want["actions"]).all()
    assert base.replay_ok(cs, scr, res)


# ------------------------------------------------------------------------------------------- 9. sync_every
def test_sync_every_does_not_change_the_result():
    """sync_every 1, 3 and 1000 (never): the early break only skips depths at which nothing is active."""
    S = search_mod()
    counts = [k for k in range(0, 9) for _ in range(6)]
    scr = base.scrambles(3, counts, seed=9)
    model = base.Stub(3).to(DEV)
    want = base.ref_search(3, scr, 8, 6)
    assert (want["length"] == -1).sum() >= 5 and (want["length"] == 0).sum() >= 6 and want["length"].max() >= 3
    for s in (1, 3, 1000):
        res = S.beam_search(model, base.env_of(3, scr), 8, 6, sync_every=s)
        L, act = res["length"].cpu().numpy(), res["actions"].cpu().numpy()
        assert act.shape == (6, len(scr))
        assert (res["solved"].cpu().numpy() == want["solved"]).all() and (L == want["length"]).all() and (act == want["actions"]).all(), s
        for p in range(len(scr)):
            assert (act[max(L[p], 0):, p] == 12).all(), (s, p)
        assert base.replay_ok(3, scr, res)
    # every cube solved at depth 2: the break at depth 2 (sync_every 1, 2) against running all 9 depths
    scr2 = base.scrambles(3, [1, 2] * 10, seed=10)
    runs = [S.beam_search(model, base.env_of(3, scr2), 64, 9, sync_every=s) for s in (1, 2, 1000)]
    assert int(runs[0]["length"].max()) <= 2 and bool(runs[0]["solved"].all())
    same_result(runs[0], runs[1])
    same_result(runs[0], runs[2])
    assert bool((runs[0]["actions"][2:] == 12).all())


# ------------------------------------------------------------------------------------------- 10. error returns
def _entry_points(plan, roots, root_pitch):
    """name -> (argument list of a valid call, {argument name: index})."""
    ptr = lambda t: t.data_ptr()                                     # plain integers: the cases below offset them
    pl = plan
    P, W, cs, pitch, D = pl.P, pl.W, pl.cs, pl.pitch, max(pl.D, 1)
    return {
        "rc_search_init": ([ptr(roots), P, root_pitch, cs, W, ptr(pl.beams[0]), pitch, ptr(pl.last_action), ptr(pl.live), ptr(pl.active),
                            ptr(pl.length), ptr(pl.solution), None],
                           dict(roots=0, n_problems=1, root_pitch=2, cube_size=3, width=4, beam=5, pitch=6, last_action=7, live=8, active=9,
                                length=10, solution=11)),
        "rc_search_expand": ([ptr(pl.beams[0]), P, W, pitch, cs, ptr(pl.last_action), ptr(pl.live), ptr(pl.active), ptr(pl.code), ptr(pl.flags),
                              ptr(pl.keys), None],
                             dict(beam=0, n_problems=1, width=2, pitch=3, cube_size=4, last_action=5, live=6, active=7, code=8, flags=9, keys=10)),
        "rc_search_select": ([ptr(pl.flags), ptr(pl.keys), ptr(pl.scores), P, W, pitch, cs, ptr(pl.live), ptr(pl.active), ptr(pl.length),
                              ptr(pl.solution), ptr(pl.depth), ptr(pl.sel_parent), ptr(pl.sel_action), ptr(pl.sel_count), ptr(pl.workspace),
                              pl.workspace.numel(), None],
                             dict(flags=0, keys=1, scores=2, n_problems=3, width=4, pitch=5, cube_size=6, live=7, active=8, length=9, solution=10,
                                  depth=11, sel_parent=12, sel_action=13, sel_count=14, workspace=15, workspace_bytes=16)),
        "rc_search_advance": ([ptr(pl.beams[0]), ptr(pl.beams[1]), P, W, pitch, cs, ptr(pl.sel_parent), ptr(pl.sel_action), ptr(pl.sel_count),
                               ptr(pl.live), ptr(pl.last_action), ptr(pl.hist_parent), ptr(pl.hist_action), ptr(pl.depth), D, None],
                              dict(beam_in=0, beam_out=1, n_problems=2, width=3, pitch=4, cube_size=5, sel_parent=6, sel_action=7, sel_count=8,
                                   live=9, last_action=10, hist_parent=11, hist_action=12, depth=13, max_depth=14)),
        "rc_search_backtrack": ([ptr(pl.hist_parent), ptr(pl.hist_action), P, W, pitch, cs, D, ptr(pl.length), ptr(pl.solution), ptr(pl.actions),
                                 None],
                                dict(hist_parent=0, hist_action=1, n_problems=2, width=3, pitch=4, cube_size=5, max_depth=6, length=7, solution=8,
                                     actions=9)),
    }


POINTERS = {"rc_search_init": ["roots", "beam", "last_action", "live", "active", "length", "solution"],
            "rc_search_expand": ["beam", "last_action", "live", "active", "code", "flags", "keys"],
            "rc_search_select": ["flags", "keys", "scores", "live", "active", "length", "solution", "depth", "sel_parent", "sel_action", "sel_count",
                                 "workspace"],
            "rc_search_advance": ["beam_in", "beam_out", "sel_parent", "sel_action", "sel_count", "live", "last_action", "hist_parent",
                                  "hist_action", "depth"],
            "rc_search_backtrack": ["hist_parent", "hist_action", "length", "solution", "actions"]}
MISALIGNED = {"rc_search_expand": ["code", "flags", "keys", "beam", "last_action"], "rc_search_select": ["workspace"],
              "rc_search_advance": ["beam_out"]}


@pytest.mark.parametrize("cs", [3, 2])
def test_argument_errors_of_every_entry_point(cs):
    """Every condition include/rubiksearch.h or the host side of rc_search.hip rejects: -1, a message that names the entry point or
    the argument, and no byte of any buffer written (all pre-filled with 0x5A).  A valid sequence of calls afterwards works."""
    from rubiks_cube_solver_amd import _search_lib, ops
    S = search_mod()
    L = _search_lib.search_lib()
    cube = beam_ref.Cube(cs)
    n, W, rp = 1300, 3, 512
    roots_np = cube.scramble(base.scrambles(cs, [i % 5 for i in range(n)], seed=6))
    roots = ops.from_aos(roots_np, DEV, rp)
    plan = S.BeamPlan(n, cs, W, 2, DEV, dense_budget_bytes=1 << 20)
    bufs = [plan.beams[0], plan.beams[1], plan.last_action, plan.live, plan.active, plan.length, plan.solution, plan.code, plan.flags, plan.keys,
            plan.scores, plan.sel_parent, plan.sel_action, plan.sel_count, plan.hist_parent, plan.hist_action, plan.actions, plan.depth,
            plan.workspace]
    for t in bufs:
        t.view(torch.uint8).fill_(0x5A)
    eps = _entry_points(plan, roots, rp)
    big_pitch = 1 << 27 if cs == 3 else 1 << 28                       # S * pitch >= 2^32 (24 * 2^27 is still below)
    tried = 0

    def refused(name, changes, token):
        nonlocal tried
        args, index = eps[name]
        args = list(args)
        for k, v in changes.items():
            args[index[k]] = v
        rc = getattr(L, name)(*args)
        msg = L.rc_search_last_error().decode()
        assert rc == -1, (name, changes, rc, msg)
        assert token in msg and (token == name or token in index or token == "null"), (name, changes, msg)
        tried += 1

    for name, (args, index) in eps.items():
        for width in (0, 65537, -1):
            refused(name, {"width": width}, "width")
        for np_ in (0, -5):
            refused(name, {"n_problems": np_}, "n_problems")
        for pitch in (256, 768, big_pitch, 0):
            refused(name, {"pitch": pitch}, "pitch")
        if cs == 2:
            assert 24 * (1 << 27) < 1 << 32                           # ... which is why 2^27 itself is a legal pitch for the 2x2x2
        for bad_cs in (4, 0):
            refused(name, {"cube_size": bad_cs}, "cube_size")
        for k in POINTERS[name]:
            refused(name, {k: None}, name)
        for k in MISALIGNED.get(name, []):
            refused(name, {k: args[index[k]] + 8}, name)
    refused("rc_search_select", {"workspace_bytes": plan.workspace.numel() - 1}, "workspace")
    refused("rc_search_select", {"workspace_bytes": 0}, "workspace")
    a, ix = eps["rc_search_advance"]
    refused("rc_search_advance", {"beam_out": a[ix["beam_in"]] + 16}, "beam_out")                     # inside beam_in's extent
    refused("rc_search_advance", {"beam_out": a[ix["beam_in"]]}, "beam_out")
    refused("rc_search_advance", {"beam_in": a[ix["beam_out"]] + plan.nbp * cube.S - 16}, "beam_out")  # beam_in starts inside beam_out
    for name in ("rc_search_advance", "rc_search_backtrack"):
        for d in (0, -1):
            refused(name, {"max_depth": d}, "max_depth")
    for bad in (0, 24, 768, -512, 520):                              # 24: not a multiple of 16; 768 / 520 < n: several tiles need a power of two
        refused("rc_search_init", {"root_pitch": bad}, "root_pitch" if bad in (0, 24, -512) else "rc_search_init")
    refused("rc_search_init", {"root_pitch": big_pitch}, "root_pitch")
    assert tried > 100
    torch.cuda.synchronize()
    for i, t in enumerate(bufs):
        assert bool((t.view(torch.uint8) == 0x5A).all()), i          # nothing was launched
    assert torch.equal(ops.to_aos(roots, n).cpu(), torch.as_tensor(roots_np))
    assert L.rc_search_workspace_bytes(cs, 0, 3) == -1 and L.rc_search_workspace_bytes(cs, 3, 0) == -1
    # a valid sequence still works
    plan.scores.zero_()
    plan.init(roots, rp)
    plan.expand(0)
    plan.select()
    plan.advance(0)
    plan.depth.add_(1)
    plan.backtrack()
    torch.cuda.synchronize()
    st = beam_ref.Stepper(cube, roots_np, W, 2)
    st.expand()
    st.select({p: np.zeros(len(cd["a"]), np.float32) for p, cd in st.cand.items()})
    st.advance()
    assert (plan.live.cpu().numpy() == st.live).all() and (plan.length.cpu().numpy() == st.length).all()
    assert (plan.actions.cpu().numpy()[:2] == st.backtrack()).all()
