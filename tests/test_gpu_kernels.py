"""HIP kernels (through the C ABI) against the CPU oracle and the golden fixtures.  GPU only.

Bit-exact everywhere: stickers, codes, one-hot bytes, done flags, rewards (+-1.0f exactly)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CS = [3, 2]
S_OF = {2: 24, 3: 54}
A_OF = {2: 6, 3: 12}
SL_OF = {2: 7, 3: 20}
RC_OF = {2: (7, 21), 3: (20, 24)}


@pytest.fixture(scope="module")
def ops():
    from rubiks_cube_solver_amd import ops as o
    return o


@pytest.fixture(scope="module")
def L():
    from rubiks_cube_solver_amd import _lib
    return _lib


def to_dev(states_aos, pitch=None):
    """[n,S] numpy -> tiled device buffer [tiles,S,pitch] (pad columns are zero)."""
    from rubiks_cube_solver_amd import ops
    return ops.from_aos(states_aos, "cuda", pitch)


def st_host(t, n):
    """tiled state / code buffer -> [n, rows] numpy."""
    from rubiks_cube_solver_amd import ops
    return ops.to_aos(t, n).cpu().numpy()


def to_host(t, n):
    """plain buffer [..., rows, pitch] -> [..., n, rows] numpy."""
    return np.ascontiguousarray(t[..., :n].cpu().numpy().swapaxes(-1, -2))


def untile(t, n, lead):
    """[*lead, tiles, rows, pitch] (or [*lead, rows, pitch]) -> numpy [*lead, n, rows]."""
    from rubiks_cube_solver_amd import ops
    if t.dim() == lead + 2:
        t = t.unsqueeze(lead)
    flat = t.reshape(-1, *t.shape[lead:])
    out = torch.stack([ops.to_aos(x, n) for x in flat]).reshape(*t.shape[:lead], n, t.shape[-2])
    return out.cpu().numpy()


def code_buf(ops, n, cs, like):
    """zeroed code buffer with the same tiling as the state buffer `like`."""
    return torch.zeros((like.shape[0], SL_OF[cs], like.shape[2]), dtype=torch.uint8, device="cuda")


def random_states(oracle, cs, n, depth, seed):
    rng = np.random.default_rng(seed)
    acts = rng.integers(0, A_OF[cs], (n, depth), dtype=np.uint8)
    out = oracle.adi(cs, n, depth, actions_in=acts, want_children=False)
    return out["parents"][:, -1].copy()


def dense_from_code(cs, code):
    """oracle-side dense one-hot from codes (uint8 [n,R,C])."""
    n = len(code)
    R, C = RC_OF[cs]
    oh = np.zeros((n, R, C), np.uint8)
    idx = np.arange(n)
    for slot in range(SL_OF[cs]):
        c = code[:, slot].astype(np.int64)
        if cs == 3:
            oh[idx, slot, c] = 1
        else:
            oh[idx, c // 3, slot * 3 + c % 3] = 1
    return oh


def test_library_tables_match_package(L):
    import rubiks_cube_solver_amd as r
    for cs in CS:
        t, p = L.get_tables(cs), r.get_tables(cs)
        assert (t["perm"] == p.perm).all() and (t["solved"] == p.solved).all()
        assert (t["corner_defs"] == p.corner_defs).all() and (t["corner_code"] == p.corner_code).all()
        assert (t["edge_code"] == p.edge_code).all()
        if cs == 3:
            assert (t["edge_defs"] == p.edge_defs).all()


@pytest.mark.parametrize("cs", CS)
@pytest.mark.parametrize("n,pitch", [(1, None), (3, None), (4, 16), (63, None), (257, 1024), (1000, None), (4099, 1024), (4099, 512),
                                     (40000, None), (40000, 2048)])
def test_fill_and_is_solved(ops, oracle, cs, n, pitch):
    st = ops.alloc_states(n, cs, "cuda", pitch)
    st.fill_(7)
    ops.fill_solved(st, n, cs)
    assert (st_host(st, n) == oracle.solved(cs, n)).all()
    done = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    rew = torch.zeros(n, dtype=torch.float32, device="cuda")
    ops.is_solved(st, n, cs, done, rew)
    assert (done.cpu().numpy() == 1).all() and (rew.cpu().numpy() == 1.0).all()


@pytest.mark.parametrize("cs", CS)
@pytest.mark.parametrize("variant", [0, 1, 2, 11, 12, 21, 22, 31, 32])   # pack width x row-traffic policy (per-call override)
@pytest.mark.parametrize("n,pitch", [(1, None), (5, None), (64, 64), (255, None), (1021, None), (16384 + 3, None),
                                     (16384 + 3, 1024), (16384 + 3, 32768)])
def test_apply_moves_vs_oracle(ops, L, oracle, cs, variant, n, pitch):
    S, A = S_OF[cs], A_OF[cs]
    states = random_states(oracle, cs, n, 17, seed=n + cs)
    rng = np.random.default_rng(n * 7 + cs)
    acts = rng.integers(0, A, n, dtype=np.uint8)
    # make some cubes one move from solved so done/reward see both values
    k = max(1, n // 5)
    states[:k] = oracle.solved(cs, k)
    exp_st, exp_code, exp_done, exp_rew = oracle.step(cs, states, acts)
    back = np.array([a ^ 1 for a in acts[:k]], np.uint8)
    src = to_dev(states, pitch)
    dst = torch.zeros_like(src)
    a_d = torch.from_numpy(acts).cuda()
    rew = torch.zeros(n, dtype=torch.float32, device="cuda")
    done = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    code = code_buf(ops, n, cs, src)
    ops.apply_moves(src, dst, a_d, n, cs, rew, done, code, L.FMT_CODE, variant=variant)
    assert (st_host(dst, n) == exp_st).all()
    assert (st_host(code, n) == exp_code).all()
    assert (done.cpu().numpy() == exp_done).all()
    assert (rew.cpu().numpy() == exp_rew).all()
    # second step in place undoes the first k cubes -> solved
    acts2 = acts.copy()
    acts2[:k] = back
    exp2, _, exp_done2, exp_rew2 = oracle.step(cs, exp_st, acts2)
    ops.apply_moves(dst, dst, torch.from_numpy(acts2).cuda(), n, cs, rew, done, variant=variant)
    assert (st_host(dst, n) == exp2).all()
    assert (done.cpu().numpy() == exp_done2).all() and exp_done2[:k].all()
    assert (rew.cpu().numpy() == exp_rew2).all()
    assert L.read_status() == 0


@pytest.mark.parametrize("cs", CS)
@pytest.mark.parametrize("fmt_name", ["U8", "F16", "BF16", "F32"])
@pytest.mark.parametrize("n,pitch", [(1, None), (6, None), (1023, None), (1024, None), (1025, None), (5000, None), (5000, 1024), (5000, 512)])
def test_apply_moves_dense_onehot(ops, L, oracle, cs, fmt_name, n, pitch):
    fmt = getattr(L, "FMT_" + fmt_name)
    R, C = RC_OF[cs]
    states = random_states(oracle, cs, n, 9, seed=100 + n)
    acts = np.random.default_rng(n).integers(0, A_OF[cs], n, dtype=np.uint8)
    exp_st, exp_code, exp_done, exp_rew = oracle.step(cs, states, acts)
    src = to_dev(states, pitch)
    dst = torch.zeros_like(src)
    oh = torch.full((n, R, C), 3, dtype=L.dense_dtype(fmt), device="cuda")
    rew = torch.zeros(n, dtype=torch.float32, device="cuda")
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ops.apply_moves(src, dst, torch.from_numpy(acts).cuda(), n, cs, rew, done, oh, fmt)
    assert (st_host(dst, n) == exp_st).all()
    exp_oh = dense_from_code(cs, exp_code)
    _, oracle_oh = oracle.encode(cs, exp_st)
    assert (exp_oh == oracle_oh).all()
    got = oh.float().cpu().numpy()                      # (numpy has no bfloat16; 0 and 1 are exact in every format)
    assert (got == exp_oh.astype(np.float32)).all()
    assert (done.cpu().numpy() == exp_done).all() and (rew.cpu().numpy() == exp_rew).all()
    # standalone encode and code -> dense agree
    oh2 = torch.full_like(oh, 5)
    ops.encode(dst, n, cs, oh2, fmt)
    assert torch.equal(oh, oh2)
    code = code_buf(ops, n, cs, src)
    ops.encode(dst, n, cs, code, L.FMT_CODE)
    assert (st_host(code, n) == exp_code).all()
    oh3 = torch.full_like(oh, 5)
    ops.onehot_from_code(code, n, cs, oh3)
    assert torch.equal(oh, oh3)


@pytest.mark.parametrize("n", [150_000, 600_000])          # dense tile size 256 (small n uses 64)
def test_dense_onehot_large_tiles(ops, L, n):
    st = ops.alloc_states(n, 3, "cuda")
    ops.fill_solved(st, n, 3)
    ops.scramble(st, n, 3, 13, seed=n)
    code = ops.alloc_code(n, 3, "cuda")
    ops.encode(st, n, 3, code, L.FMT_CODE)
    want = torch.nn.functional.one_hot(ops.to_aos(code, n).long(), 24).to(torch.uint8)     # [n, 20, 24]
    for fmt in (L.FMT_U8, L.FMT_F32):
        oh = torch.empty((n, 20, 24), dtype=L.dense_dtype(fmt), device="cuda")
        ops.encode(st, n, 3, oh, fmt)
        assert torch.equal(oh.to(torch.uint8), want)
        oh.fill_(3)
        ops.onehot_from_code(code, n, 3, oh)
        assert torch.equal(oh.to(torch.uint8), want)
    acts = torch.randint(0, 12, (n,), dtype=torch.uint8, device="cuda")
    st2, oh2 = torch.empty_like(st), torch.empty((n, 20, 24), dtype=torch.float16, device="cuda")
    ops.apply_moves(st, st2, acts, n, 3, None, None, oh2, L.FMT_F16)
    ops.encode(st2, n, 3, code, L.FMT_CODE)
    assert torch.equal(oh2.to(torch.uint8), torch.nn.functional.one_hot(ops.to_aos(code, n).long(), 24).to(torch.uint8))


def test_golden_walks_on_gpu(ops, L, golden):
    """G3 replayed step by step through rc_apply_moves: stickers, one-hot column, done, reward."""
    g = golden("walks_333")
    W, D = g["actions"].shape
    st = ops.alloc_states(W, 3, "cuda")
    ops.fill_solved(st, W, 3)
    code = code_buf(ops, W, 3, st)
    rew = torch.zeros(W, dtype=torch.float32, device="cuda")
    done = torch.zeros(W, dtype=torch.uint8, device="cuda")
    acts = torch.from_numpy(np.ascontiguousarray(g["actions"].T)).cuda()
    for d in range(D):
        ops.apply_moves(st, st, acts[d].contiguous(), W, 3, rew, done, code, L.FMT_CODE)
        assert (st_host(st, W) == g["stickers"][:, d]).all()
        assert (st_host(code, W) == g["cols"][:, d]).all()
        assert (done.cpu().numpy() == g["done"][:, d]).all()
        assert (rew.cpu().numpy() == g["reward"][:, d]).all()


def test_golden_encode_arbitrary_colourings(ops, L, golden):
    g = golden("encode_333")
    n = len(g["stickers"])
    st = to_dev(g["stickers"])
    code = code_buf(ops, n, 3, st)
    ops.encode(st, n, 3, code, L.FMT_CODE)
    assert (st_host(code, n) == g["cols"]).all()
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ops.is_solved(st, n, 3, done)
    assert (done.cpu().numpy() == g["solved"]).all()
    rec = to_dev(g["recoloured"])
    done = torch.zeros(len(g["recoloured"]), dtype=torch.uint8, device="cuda")
    ops.is_solved(rec, len(g["recoloured"]), 3, done)
    assert (done.cpu().numpy() == g["recoloured_solved"]).all()


@pytest.mark.parametrize("cs", CS)
@pytest.mark.parametrize("n,pitch", [(1, None), (37, None), (512, None), (4096, None), (4096, 1024), (4096, 512), (70000, None), (70000, 2048)])
def test_expand_children(ops, L, oracle, cs, n, pitch):
    S, A, SL = S_OF[cs], A_OF[cs], SL_OF[cs]
    if pitch is not None:
        return _expand_tiled(ops, oracle, cs, n, pitch)
    states = random_states(oracle, cs, n, 20, seed=n)
    states[: max(1, n // 7)] = oracle.step(cs, oracle.solved(cs, max(1, n // 7)), np.arange(max(1, n // 7)) % A)[0]
    ch, cc, cso = oracle.expand(cs, states, threads=4)
    src = to_dev(states)
    p = L.pitch_for(n)
    children = torch.zeros((A, S, p), dtype=torch.uint8, device="cuda")
    solved = torch.zeros((A, p), dtype=torch.uint8, device="cuda")
    code = torch.zeros((A, SL, p), dtype=torch.uint8, device="cuda")
    ops.expand_children(src, n, cs, children, solved, code)
    assert (to_host(children, n).transpose(1, 0, 2) == ch).all()      # [n, A, S]
    assert (solved[:, :n].cpu().numpy().T == cso).all() and cso.any()
    assert (to_host(code, n).transpose(1, 0, 2) == cc).all()
    solved2 = torch.zeros_like(solved)
    ops.expand_children(src, n, cs, child_solved=solved2)
    assert torch.equal(solved[:, :n], solved2[:, :n])


def _expand_tiled(ops, oracle, cs, n, pitch):
    A = A_OF[cs]
    states = random_states(oracle, cs, n, 20, seed=n)
    ch, cc, cso = oracle.expand(cs, states, threads=4)
    out = ops.expand_buffers(n, cs, "cuda", pitch, children=True, codes=True)
    for v in out.values():
        v.fill_(9)
    ops.expand_children(to_dev(states), n, cs, out["children"], out["child_solved"], out["child_code"], pitch=pitch)
    assert out["children"].shape[1] > 1
    assert (untile(out["children"], n, 1).transpose(1, 0, 2) == ch).all()
    assert (untile(out["child_code"], n, 1).transpose(1, 0, 2) == cc).all()
    assert (out["child_solved"][:, :n].cpu().numpy().T == cso).all()


def test_golden_expand(ops, L, golden):
    g = golden("expand_333")
    n = len(g["leaves"])
    src = to_dev(g["leaves"])
    p = L.pitch_for(n)
    children = torch.zeros((12, 54, p), dtype=torch.uint8, device="cuda")
    solved = torch.zeros((12, p), dtype=torch.uint8, device="cuda")
    code = torch.zeros((12, 20, p), dtype=torch.uint8, device="cuda")
    ops.expand_children(src, n, 3, children, solved, code)
    assert (to_host(children, n).transpose(1, 0, 2) == g["child_stickers"]).all()
    assert (to_host(code, n).transpose(1, 0, 2) == g["child_cols"]).all()
    assert (solved[:, :n].cpu().numpy().T == g["child_done"]).all()


@pytest.mark.parametrize("cs", CS)
@pytest.mark.parametrize("n_walks,depth,pitch", [(1, 1, None), (5, 3, None), (300, 30, None), (5000, 7, None), (5000, 7, 1024),
                                                 (3000, 4, 2048)])
@pytest.mark.parametrize("replay", [False, True])
def test_adi_generate(ops, L, oracle, cs, n_walks, depth, pitch, replay):
    S, A, SL = S_OF[cs], A_OF[cs], SL_OF[cs]
    pitch, bufs = ops.adi_buffers(n_walks, depth, cs, "cuda", pitch or L.pitch_for(n_walks), parents=True, parent_code=True,
                                  children=True, child_code=True)
    for v in bufs.values():
        v.fill_(7)
    wp = bufs["actions_out"].shape[1]
    kw = {}
    exp_kw = dict(seed=2024, stream=3, walk0=11)
    if replay:
        acts = np.random.default_rng(5).integers(0, A, (n_walks, depth), dtype=np.uint8)
        a_in = torch.zeros((depth, wp), dtype=torch.uint8, device="cuda")
        a_in[:, :n_walks] = torch.from_numpy(np.ascontiguousarray(acts.T)).cuda()
        kw["actions_in"] = a_in
        exp_kw["actions_in"] = acts
    exp = oracle.adi(cs, n_walks, depth, threads=4, **exp_kw)
    ops.adi_generate(n_walks, depth, cs, pitch, "cuda", seed=2024, stream_id=3, walk_offset=11, **kw, **bufs)
    assert L.read_status() == 0
    assert (bufs["actions_out"][:, :n_walks].cpu().numpy().T == exp["actions"]).all()
    assert (untile(bufs["parents"], n_walks, 1).transpose(1, 0, 2) == exp["parents"]).all()
    assert (untile(bufs["parent_code"], n_walks, 1).transpose(1, 0, 2) == exp["parent_code"]).all()
    assert (untile(bufs["children"], n_walks, 2).transpose(2, 0, 1, 3) == exp["children"]).all()
    assert (untile(bufs["child_code"], n_walks, 2).transpose(2, 0, 1, 3) == exp["child_code"]).all()
    assert (bufs["child_solved"][..., :n_walks].cpu().numpy().transpose(2, 0, 1) == exp["child_solved"]).all()
    # subsets of outputs give the same bytes
    cs2 = torch.zeros_like(bufs["child_solved"])
    ops.adi_generate(n_walks, depth, cs, pitch, "cuda", seed=2024, stream_id=3, walk_offset=11, child_solved=cs2, **kw)
    assert torch.equal(cs2[..., :n_walks], bufs["child_solved"][..., :n_walks])


@pytest.mark.parametrize("cs", CS)
def test_scramble_matches_adi_and_reset_golden(ops, L, oracle, golden, cs):
    n, depth = 777, 25
    st = ops.alloc_states(n, cs, "cuda")
    ops.fill_solved(st, n, cs)
    p = L.pitch_for(n)
    a_out = torch.zeros((depth, p), dtype=torch.uint8, device="cuda")
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ops.scramble(st, n, cs, depth, seed=9, stream_id=1, walk_offset=5, actions_out=a_out, done=done)
    exp = oracle.adi(cs, n, depth, seed=9, stream=1, walk0=5, want_children=False)
    assert (a_out[:, :n].cpu().numpy().T == exp["actions"]).all()
    assert (st_host(st, n) == exp["parents"][:, -1]).all()
    assert (done.cpu().numpy() == oracle.is_solved(cs, exp["parents"][:, -1])).all()
    if cs == 3:  # G4: the reference's reset(seed, k) action draws replayed on the device
        g = golden("reset_333")
        ns, nk = g["actions"].shape[:2]
        for j in (0, 4, 29):
            k = int(g["ks"][j])
            st = ops.alloc_states(ns, 3, "cuda")
            ops.fill_solved(st, ns, 3)
            a_in = torch.zeros((k, L.pitch_for(ns)), dtype=torch.uint8, device="cuda")
            a_in[:, :ns] = torch.from_numpy(np.ascontiguousarray(g["actions"][:, j, :k].T)).cuda()
            ops.scramble(st, ns, 3, k, actions_in=a_in)
            assert (st_host(st, ns) == g["stickers"][:, j]).all()


def test_bad_action_sets_status(ops, L):
    n = 100
    st = ops.alloc_states(n, 3, "cuda")
    ops.fill_solved(st, n, 3)
    for bad in (13, 14, 200, 255):            # 12 is the no-op
        acts = torch.zeros(n, dtype=torch.uint8, device="cuda")
        acts[37] = bad
        ops.apply_moves(st, st, acts, n, 3)
        assert L.read_status() & L.STATUS_BAD_ACTION
        assert L.read_status() == 0
    st2 = ops.alloc_states(n, 2, "cuda")
    ops.fill_solved(st2, n, 2)
    for bad in (7, 8, 11, 12, 13, 99):         # 6 is the no-op
        acts = torch.zeros(n, dtype=torch.uint8, device="cuda")
        acts[5] = bad
        ops.apply_moves(st2, st2, acts, n, 2)
        assert L.read_status() & L.STATUS_BAD_ACTION


def test_argument_errors(ops, L):
    st = ops.alloc_states(10, 3, "cuda")
    with pytest.raises(NotImplementedError):
        ops.alloc_states(10, 4, "cuda")
    with pytest.raises(L.RubikHipError):
        ops.fill_solved(st[:, :, :7], 7, 3)         # non-contiguous / bad pitch
    with pytest.raises(L.RubikHipError):
        ops.fill_solved(torch.zeros((4, 54, 48), dtype=torch.uint8, device="cuda"), 100, 3)  # tiles need pow2 pitch >= 1024
    with pytest.raises(L.RubikHipError):
        ops.apply_moves(st, st, torch.zeros(10, dtype=torch.int64, device="cuda"), 10, 3)
    with pytest.raises(L.RubikHipError):
        ops.fill_solved(torch.zeros((54, 256), dtype=torch.uint8), 10, 3)   # host tensor
    assert L.lib().rc_fill_solved(None, 1, 256, 3, None) == -1
    assert b"rc_fill_solved" in L.lib().rc_last_error()
    assert L.lib().rc_fill_solved(L.ptr(st), 1, 256, 5, None) == -1
    assert L.lib().rc_fill_solved(L.ptr(st), 2000, 48, 3, None) == -1
    assert L.lib().rc_fill_solved(L.ptr(st), 1, 1 << 27, 3, None) == -1      # rows * pitch >= 2^32: single tiles stop at ~79 M cubes
    assert L.lib().rc_facade_step(L.ptr(st), 256, 3, 0, None, 1, 1, None) == -1 and b"rc_facade_step" in L.lib().rc_last_error()
    dev_buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")             # the result buffer must be HOST memory: refused, not a crash
    assert L.lib().rc_facade_step(L.ptr(st), 256, 3, 0, L.ptr(dev_buf), 1, 1, None) == -1 and b"pinned" in L.lib().rc_last_error()


@pytest.mark.parametrize("cs", CS)
def test_adi_targets(ops, cs):
    A = A_OF[cs]
    n, p = 1000, 1024
    g = torch.Generator().manual_seed(1)
    cv = torch.randn((A, p), generator=g)
    cv[:, 5] = 0.25                      # all equal -> first index
    cv[3, 6] = cv[7 % A, 6] = 9.0        # tie -> lowest index
    solved = (torch.rand((A, p), generator=g) < 0.05).to(torch.uint8)
    pv = torch.randn(n, generator=g)
    d = torch.randint(1, 31, (n,), generator=g)
    w = torch.tensor([float(int(x) ** (-0.3)) for x in d], dtype=torch.float64)
    tv, tp, err = ops.adi_targets(cv.cuda(), solved.cuda(), n, cs, pv.cuda(), w.cuda())
    cvn, sn = cv.numpy()[:, :n], solved.numpy()[:, :n].astype(bool)
    v = cvn + np.float32(-1.0)
    exp_tp = np.where(sn.any(0), np.argmax(sn, 0), np.argmax(v, 0))
    exp_tv = np.where(sn.any(0), np.float32(1.0), v.max(0)).astype(np.float32)
    assert (tp.cpu().numpy() == exp_tp).all()
    assert (tv.cpu().numpy() == exp_tv).all()
    exp_err = np.abs(pv.numpy().astype(np.float64) - exp_tv.astype(np.float64)) * w.numpy()
    assert (err.cpu().numpy() == exp_err).all()


@pytest.mark.parametrize("cs", CS)
def test_adi_targets_nonfinite(ops, cs):
    """Non-finite child values (tests/adi_cases.py: NaN at every index, at several, everywhere; +-inf; -0 / +0 ties; solved children
    next to NaN; NaN parent values) against the reference's own operator, torch.max on CPU float32 tensors: NaN propagates with the
    index of the first NaN, otherwise the first maximal index; a solved child wins over both."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import adi_cases
    adi_cases.check_oracle()
    A = A_OF[cs]
    cv, solved, pv = adi_cases.edge_columns(A, seed=cs)
    n = cv.shape[1]
    p = -(-n // 256) * 256
    cvp, sp = torch.zeros((A, p)), torch.zeros((A, p), dtype=torch.uint8)
    cvp[:, :n], sp[:, :n] = cv, solved
    w = np.array([float(1 + i % 30) ** -0.3 for i in range(n)])
    tv, tp, err = ops.adi_targets(cvp.cuda(), sp.cuda(), n, cs, pv.cuda(), torch.tensor(w, dtype=torch.float64).cuda())
    e_tv, e_tp, e_err = adi_cases.expected(cv, solved, pv, w)
    assert np.isnan(e_tv).sum() > 100 and np.isinf(e_tv).sum() > 50 and (e_tv == 1.0).sum() > 20      # the cases are there
    adi_cases.assert_same(tp.cpu().numpy(), e_tp, "target_policy")
    adi_cases.assert_same(tv.cpu().numpy(), e_tv, "target_value")
    adi_cases.assert_same(err.cpu().numpy(), e_err, "error")
    tv2, tp2, none = ops.adi_targets(cvp.cuda(), sp.cuda(), n, cs)                                    # without the error output
    assert none is None
    adi_cases.assert_same(tv2.cpu().numpy(), e_tv, "target_value")
    adi_cases.assert_same(tp2.cpu().numpy(), e_tp, "target_policy")


def test_full_size_properties(ops, L):
    """BASELINE sizes (4M cubes): order-4 and inverse identities, checksum of checksums."""
    n = 1 << 22
    st = ops.alloc_states(n, 3, "cuda")
    ops.fill_solved(st, n, 3)
    ops.scramble(st, n, 3, 20, seed=1234)
    ref = st.clone()
    g = torch.Generator(device="cuda").manual_seed(1)
    acts = torch.randint(0, 12, (n,), generator=g, device="cuda", dtype=torch.uint8)
    tmp = torch.empty_like(st)
    ops.apply_moves(st, tmp, acts, n, 3)
    assert st.shape[0] > 1                                         # tiled layout at this size
    assert not torch.equal(tmp, ref)
    assert torch.equal(tmp.to(torch.int32).sum(1), ref.to(torch.int32).sum(1))  # a move permutes stickers
    ops.apply_moves(tmp, st, acts ^ 1, n, 3)                      # X then X' = identity
    assert torch.equal(st, ref)
    for _ in range(4):                                             # X^4 = identity
        ops.apply_moves(st, st, acts, n, 3)
    assert torch.equal(st, ref)
    done = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ops.is_solved(st, n, 3, done)
    assert int(done.sum()) < n // 1000
    assert L.read_status() == 0


def test_empty_batches_are_noops(ops, L):
    st = ops.alloc_states(16, 3, "cuda")
    st.fill_(3)
    acts = torch.zeros(16, dtype=torch.uint8, device="cuda")
    done = torch.full((16,), 9, dtype=torch.uint8, device="cuda")
    ops.fill_solved(st, 0, 3)
    ops.apply_moves(st, st, acts, 0, 3, None, done)
    ops.scramble(st, 0, 3, 5)
    ops.is_solved(st, 0, 3, done)
    assert bool((st == 3).all()) and bool((done == 9).all())
    pt, bufs = ops.adi_buffers(16, 2, 3, "cuda", parents=True)
    ops.adi_generate(0, 2, 3, pt, "cuda", **bufs)
    ops.adi_generate(16, 0, 3, pt, "cuda")
    assert L.read_status() == 0


def test_sixteen_million_cubes_identities(ops, L):
    """Largest batch exercised (2^24 cubes, 906 MB of stickers, 512 tiles): X then X' and the checksum of checksums."""
    n = 1 << 24
    st = ops.alloc_states(n, 3, "cuda")
    ops.fill_solved(st, n, 3)
    ops.scramble(st, n, 3, 12, seed=99)
    ref_sum = st.sum(dim=(0, 2), dtype=torch.int64)               # per-row checksums
    assert int(ref_sum.sum()) == n * sum(9 * c for c in range(6))  # every cube still has 9 stickers of each colour
    acts = torch.randint(0, 12, (n,), dtype=torch.uint8, device="cuda")
    tmp = torch.empty_like(st)
    ops.apply_moves(st, tmp, acts, n, 3)
    assert int(tmp.sum(dtype=torch.int64)) == int(ref_sum.sum())
    ops.apply_moves(tmp, tmp, acts ^ 1, n, 3)
    assert torch.equal(tmp, st)
    assert L.read_status() == 0


@pytest.mark.parametrize("cs", CS)
def test_legacy_numpy_rng_on_device(ops, L, golden, cs):
    """rc_legacy_scramble_actions == np.random.seed(s); np.random.randint(A, size=k) (numpy's legacy MT19937 with
    masked rejection), bit for bit: short and long draws (k = 1000 crosses two state twists), per-env counts."""
    A = A_OF[cs]
    saved = np.random.get_state()
    try:
        seeds = [0, 1, 5, 10, 90, 12345, 777, 2 ** 31, 2 ** 32 - 1] + list(range(100, 100 + 150))
        for k in (1, 5, 30, 227, 1000):
            buf, kk = ops.legacy_scramble_actions(torch.tensor(seeds, dtype=torch.int64), cs, k, device="cuda")
            got = buf[:k, :len(seeds)].cpu().numpy().T
            for i, s in enumerate(seeds):
                np.random.seed(s)
                assert (got[i] == np.random.randint(A, size=k)).all(), (s, k)
        counts = [1 + (7 * i) % 40 for i in range(len(seeds))]
        buf, kk = ops.legacy_scramble_actions(torch.tensor(seeds, dtype=torch.int64), cs, counts, device="cuda")
        got = buf[:, :len(seeds)].cpu().numpy().T
        assert kk == max(counts)
        for i, (s, k) in enumerate(zip(seeds, counts)):
            np.random.seed(s)
            assert (got[i, :k] == np.random.randint(A, size=k)).all() and (got[i, k:kk] == A).all()
    finally:
        np.random.set_state(saved)
    if cs == 3:
        g = golden("reset_333")                                   # the reference's own reset(seed, k) draws
        buf, _ = ops.legacy_scramble_actions(torch.tensor([int(s) for s in g["seeds"]]), 3, 30, device="cuda")
        assert (buf[:30, :len(g["seeds"])].cpu().numpy().T == g["actions"][:, 29, :]).all()
    with pytest.raises(ValueError):
        ops.legacy_scramble_actions(torch.tensor([-1]), cs, 3, device="cuda")


def test_empty_batches_are_no_ops(ops, L):
    """n = 0 (and depth = 0) through every batched entry point: RC_OK, nothing launched, nothing written (the reference's loops
    over zero cubes / zero scramble moves do nothing either: cube_env.py:177-194 with sample_cube_count = 0)."""
    st = ops.alloc_states(256, 3, "cuda")
    st.fill_(9)
    acts = torch.zeros(256, dtype=torch.uint8, device="cuda")
    done = torch.full((256,), 9, dtype=torch.uint8, device="cuda")
    rew = torch.full((256,), 9.0, dtype=torch.float32, device="cuda")
    code = ops.alloc_code(256, 3, "cuda").fill_(9)
    oh = torch.full((256, 20, 24), 9, dtype=torch.float32, device="cuda")
    ops.fill_solved(st, 0, 3)
    ops.apply_moves(st, st, acts, 0, 3, rew, done, code, L.FMT_CODE)
    ops.apply_moves(st, st, acts, 0, 3, rew, done, oh, L.FMT_F32)
    ops.scramble(st, 0, 3, 5, seed=1)
    ops.scramble(st, 256, 3, 0, seed=1)                              # zero moves: the states stay as they are
    ops.is_solved(st, 0, 3, done, rew)
    ops.encode(st, 0, 3, code, L.FMT_CODE)
    ops.onehot_from_code(code, 0, 3, oh)
    ex = ops.expand_buffers(256, 3, "cuda", children=True, codes=True)
    for t in ex.values():
        t.fill_(9)
    ops.expand_children(st, 0, 3, ex["children"], ex["child_solved"], ex["child_code"], pitch=ex["children"].shape[-1])
    pt, bufs = ops.adi_buffers(256, 4, 3, "cuda", parents=True, children=True, parent_code=True, child_code=True)
    for t in bufs.values():
        t.fill_(9)
    ops.adi_generate(0, 4, 3, pt, "cuda", seed=1, **bufs)
    ops.adi_generate(256, 0, 3, pt, "cuda", seed=1, **{k: v[:0] for k, v in bufs.items()})
    torch.cuda.synchronize()
    for t in (st, done, code, *ex.values(), *bufs.values()):
        assert bool((t == 9).all())
    assert bool((rew == 9.0).all()) and bool((oh == 9.0).all())
    tv, tp, err = ops.adi_targets(torch.zeros((12, 256), device="cuda"), torch.zeros((12, 256), dtype=torch.uint8, device="cuda"), 0, 3)
    assert tv.numel() == 0 and tp.numel() == 0 and err is None
    assert L.read_status() == 0
