"""Columns of child values with non-finite entries for the ADI target rule (rc_adi_targets, cube_env.py:229-251), and what the
reference's own operator makes of them: torch.max on CPU float32 tensors.  Test infrastructure only."""
import numpy as np
import torch

NAN, INF = float("nan"), float("inf")


def check_oracle():
    """The semantics of torch.max the expectation rests on: a torch that orders NaN or ties differently is noticed here."""
    m = torch.max(torch.tensor([1.0, 3.0, NAN, 5.0, NAN]), -1)
    assert bool(torch.isnan(m.values)) and int(m.indices) == 2              # NaN propagates: the index of the FIRST NaN
    assert int(torch.max(torch.tensor([0.0, -0.0, 0.0, -0.0, -1.0]), -1).indices) == 0   # -0 == +0: the first of the tie
    m = torch.max(torch.tensor([INF, 1.0, INF, 2.0, 3.0]), -1)
    assert float(m.values) == INF and int(m.indices) == 0


def edge_columns(A, seed=0):
    """-> child_value float32 [A, n], child_solved uint8 [A, n], parent_value float32 [n] (host tensors), built by hand and at random."""
    g = torch.Generator().manual_seed(seed)
    cols, solved, parent = [], [], []

    def add(col, sol=(), pv=0.5):
        cols.append(torch.as_tensor(col, dtype=torch.float32).clone())
        s = torch.zeros(A, dtype=torch.uint8)
        for k in sol:
            s[k] = 1
        solved.append(s)
        parent.append(pv)

    rnd = lambda: torch.randn(A, generator=g)
    for k in range(A):                                                       # NaN at each single child index
        c = rnd(); c[k] = NAN; add(c)
        c = rnd() + 5.0; c[k] = NAN; c[(k + 1) % A] = 50.0; add(c)           # next to a large finite maximum
    for _ in range(24):                                                      # NaN at several
        c = rnd(); c[torch.rand(A, generator=g) < 0.4] = NAN; add(c)
    add(torch.full((A,), NAN))                                               # all NaN
    add(-torch.full((A,), NAN))
    for k in range(A):                                                       # +inf at one / two indices
        c = rnd(); c[k] = INF; add(c)
        c = rnd(); c[k] = INF; c[(k + 2) % A] = INF; add(c)
    add(torch.full((A,), -INF))                                              # all -inf
    c = torch.full((A,), -INF); c[A - 1] = -1e38; add(c)
    for k in range(A):                                                       # +inf and NaN together, either one first
        c = rnd(); c[k] = INF; c[(k + 1) % A] = NAN; add(c)
        c = rnd(); c[k] = NAN; c[(k + 1) % A] = -INF; add(c)
    z = torch.tensor([0.0, -0.0] * (A // 2))                                 # -0 / +0 ties, as values and after the reward is added
    add(z); add(-z); add(z + 1.0); add(torch.cat([torch.full((A - 2,), -7.0), torch.tensor([-0.0, 0.0])]))
    for k in range(A):                                                       # a solved child together with NaN values: the solved rule wins
        c = rnd(); c[(k + 1) % A] = NAN; add(c, sol=(k,))
        c = torch.full((A,), NAN); add(c, sol=(k, A - 1))
    c = rnd(); c[0] = NAN; add(c, sol=(3, 1))
    add(rnd(), pv=NAN)                                                       # NaN parent value
    add(rnd(), sol=(2,), pv=NAN)
    c = rnd(); c[1] = NAN; add(c, pv=NAN)
    add(rnd(), pv=INF); add(torch.full((A,), INF), pv=INF)                  # inf - inf in the error
    pool = torch.tensor([NAN, INF, -INF, 0.0, -0.0, 1.0, 3.4028234663852886e38, -3.4028234663852886e38])
    for _ in range(400):                                                     # at random
        c = rnd()
        pick = torch.rand(A, generator=g) < 0.45
        c[pick] = pool[torch.randint(0, len(pool), (int(pick.sum()),), generator=g)]
        sol = [k for k in range(A) if float(torch.rand((), generator=g)) < 0.03]
        add(c, sol=sol, pv=float(torch.randn((), generator=g)))
    return torch.stack(cols, 1).contiguous(), torch.stack(solved, 1).contiguous(), torch.tensor(parent, dtype=torch.float32)


def expected(child_value, child_solved, parent_value, weight):
    """cube_env.py:229-251 on the host: torch.max(child_value + (-1.0), 0) unless a child is solved; error in float64 (include/rubikhip.h).
    child_value / child_solved [A, n], parent_value [n] CPU tensors, weight float64 numpy [n] -> numpy tv, tp, err."""
    assert child_value.device.type == "cpu" and child_value.dtype == torch.float32
    m = torch.max(child_value + (-1.0), 0)
    any_solved = child_solved.bool().any(0)
    s = child_solved.numpy().astype(bool)
    first = torch.as_tensor(np.array([int(np.flatnonzero(s[:, i])[0]) if s[:, i].any() else 0 for i in range(s.shape[1])]))
    tv = torch.where(any_solved, torch.tensor(1.0), m.values).numpy().astype(np.float32)
    tp = torch.where(any_solved, first, m.indices).numpy().astype(np.int32)
    with np.errstate(invalid="ignore"):
        err = np.abs(parent_value.numpy().astype(np.float64) - tv.astype(np.float64)) * np.asarray(weight, np.float64)
    return tv, tp, err


def assert_same(got, want, what):
    """NaN positions as a mask, everything else for equality."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    if got.dtype.kind == "f":
        gn, wn = np.isnan(got), np.isnan(want)
        assert (gn == wn).all(), (what, "NaN positions differ at", np.flatnonzero(gn != wn)[:10].tolist())
        bad = np.flatnonzero(~wn & (got != want))
    else:
        bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, bad[:10].tolist(), got[bad[:10]].tolist(), want[bad[:10]].tolist())
