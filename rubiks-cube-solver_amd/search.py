"""Batched beam search guided by the value head (DeepCubeA-style; DESIGN.md "Beam search"): the solver behind the solve rates
test.py and train.py:167-198 report, for thousands of cubes at once.

One depth step, all on the device and without a host synchronisation:
  rc_search_expand     all A children of every beam slot: compact codes, valid / solved flags, exact sticker keys
  rc_onehot_from_code  + ONE forward of the caller's net per chunk of candidates (dense_budget_bytes), scores = model(x)[0][:, 0]
  rc_search_select     solved check, exact removal of duplicate states, the W best per cube (score desc, candidate index asc)
  rc_search_advance    the kept children become the next beam (ping-pong buffers) + one history row
The solutions are read back from the history by rc_search_backtrack at the end.

front="codes" (opt-in; DESIGN.md "Net front") replaces the second line: rc_net_first_layer sums the first layer's rows straight from
the candidate codes into a [chunk, H1] buffer, and the rest of the encoder and the value head run on that; no dense one-hot exists.
front="table" (DESIGN.md "Corner pattern database") replaces it by ONE launch and no net: the `model` is a pattern.CornerTable and
rcp_score_keys writes scores = -table[corner index] from the candidate keys.  In astar_search it also adds rcp_relax after rca_merge (an
open node reached again by fewer moves takes the lower g): with batch = 1 and weight = 1 the table-guided search is A* proper.
On the 3x3x3 the `model` may also be a pattern.MaxTable (DESIGN.md "Edge pattern databases"): the maximum of a corner table and edge
tables, one rce_score_codes(combine=1) launch per edge table over the candidate codes after rcp_score_keys.

astar_search / AStarPlan (DESIGN.md "A* search"): batch-weighted A* around the same expand and score.  Per cube a persistent node pool
with an exact hash set; an iteration is rca_pop (the B best open nodes -> the beam), rc_search_expand, the score above, rca_merge (the
states the pool has not seen become nodes); rca_backtrack follows the parent links.  The rule: include/rubiksearch.h.
"""
from __future__ import annotations

import torch

from . import _lib, _search_lib, ops
from ._lib import ptr, stream_ptr
from ._search_lib import check
from .tables import get_env_config

MAX_WIDTH = 65536
FRONTS = ("dense", "codes", "table")
KEY_WORDS = {3: 3, 2: 2}


def beam_pitch(n_slots):
    """Tile pitch of the beam and candidate buffers: a power of two >= 512 (the A candidate blocks then form ONE tiled code buffer)
    and at most ops.DEFAULT_TILE."""
    p = ops.MIN_TILE
    while p < n_slots and p < ops.DEFAULT_TILE:
        p *= 2
    return p


class BeamPlan:
    """Device buffers of one search shape (P problems, width W, max_depth D) and the launches of one depth step.
    Layouts: include/rubiksearch.h.  The methods wrap one entry point each; tests drive them one by one."""

    def __init__(self, n_problems, cube_size, width, max_depth, device, dtype=torch.float32, dense_budget_bytes=1 << 30, front="dense",
                 hidden=None):
        """front="codes": `hidden` = H1, the width of the net's first layer; the plan then holds a [chunk, H1] buffer of `dtype` instead of
        the dense one-hot, sized by the same dense_budget_bytes rule.  front="table": neither buffer exists; score() takes a CornerTable."""
        if front not in FRONTS:
            raise ValueError(f"front must be 'dense', 'codes' or 'table', got {front!r}")
        if front == "codes" and (hidden is None or dtype not in (torch.float32, torch.bfloat16)):
            raise ValueError("front='codes' needs hidden = the first layer's width and a float32 or bfloat16 model "
                             f"(the kernel takes no other format), got hidden = {hidden}, dtype = {dtype}")
        self.front = front
        if not 1 <= int(width) <= MAX_WIDTH:
            raise ValueError(f"width must be in 1..{MAX_WIDTH}")
        if int(max_depth) < 0 or int(n_problems) < 1:
            raise ValueError("need n_problems >= 1 and max_depth >= 0")
        self.P, self.W, self.D, self.cs = int(n_problems), int(width), int(max_depth), int(cube_size)
        S, A, SL = ops._size(cube_size)
        self.S, self.A, self.SL = S, A, SL
        self.dev = dev = torch.device(device)
        (self.R, self.C), _ = get_env_config(cube_size)
        self.pitch = beam_pitch(self.P * self.W)
        self.tiles = -(-self.P * self.W // self.pitch)
        self.nbp = nbp = self.tiles * self.pitch
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.beams = [z((self.tiles, S, self.pitch), torch.uint8) for _ in range(2)]
        self.last_action = z(nbp, torch.uint8)
        self.live, self.active = z(self.P, torch.int32), z(self.P, torch.uint8)
        self.length, self.solution = z(self.P, torch.int32), z(self.P, torch.int32)
        self.code = z((A * self.tiles, SL, self.pitch), torch.uint8)
        self.flags = z((A, nbp), torch.uint8)
        self.keys = z((KEY_WORDS[cube_size], A, nbp), torch.int64)           # uint64 words
        self.scores = z((A, nbp), torch.float32)
        self.sel_parent, self.sel_action = z(nbp, torch.int16), z(nbp, torch.uint8)   # uint16 slots
        self.sel_count = z(self.P, torch.int32)
        self.hist_parent, self.hist_action = z((max(self.D, 1), nbp), torch.int16), z((max(self.D, 1), nbp), torch.uint8)
        self.actions = z((max(self.D, 1), self.P), torch.uint8)
        self.depth = z(1, torch.int32)
        L = _search_lib.search_lib()
        self.workspace = torch.empty(int(L.rc_search_workspace_bytes(self.cs, self.P, self.W)), dtype=torch.uint8, device=dev)
        self.dtype = dtype
        total = A * nbp
        if front == "table":
            self.chunk = total
            return
        row_bytes = (self.R * self.C if front == "dense" else int(hidden)) * torch.empty((), dtype=dtype).element_size()
        self.chunk = min(total, max(self.pitch, int(dense_budget_bytes) // row_bytes // self.pitch * self.pitch))
        if front == "dense":
            self.dense = torch.empty((self.chunk, self.R, self.C), dtype=dtype, device=dev)
        else:
            self.hidden = torch.empty((self.chunk, int(hidden)), dtype=dtype, device=dev)
            self._net = None

    # ------------------------------------------------------------------ one entry point each
    def init(self, roots, root_pitch):
        _lib.init(self.dev)
        check(_search_lib.search_lib().rc_search_init(ptr(roots), self.P, root_pitch, self.cs, self.W, ptr(self.beams[0]), self.pitch,
                                                      ptr(self.last_action), ptr(self.live), ptr(self.active), ptr(self.length),
                                                      ptr(self.solution), stream_ptr(self.dev)))
        self.depth.fill_(1)

    def expand(self, parity):
        check(_search_lib.search_lib().rc_search_expand(ptr(self.beams[parity]), self.P, self.W, self.pitch, self.cs, ptr(self.last_action),
                                                        ptr(self.live), ptr(self.active), ptr(self.code), ptr(self.flags), ptr(self.keys),
                                                        stream_ptr(self.dev)))

    def score(self, model):
        """scores = model(dense one-hot)[0][:, 0] for every candidate, one forward per chunk (chunks start on tile boundaries)."""
        if self.front == "codes":
            return self.score_codes(model)
        if self.front == "table":
            return self.score_table(model)
        total, flat = self.A * self.nbp, self.scores.view(-1)
        for j0 in range(0, total, self.chunk):
            m = min(self.chunk, total - j0)
            t0 = j0 // self.pitch
            ops.onehot_from_code(self.code[t0:t0 + m // self.pitch], m, self.cs, self.dense[:m])
            flat[j0:j0 + m].copy_(model(self.dense[:m])[0][:, 0])

    def code_net(self, model):
        """The CodeNet of `model` (a CodeNet passes through), checked against the plan: cube size, H1, dtype, device."""
        from .codenet import CodeNet
        if isinstance(model, CodeNet):
            net = model
        else:
            if self._net is None or self._net.model is not model:
                self._net = CodeNet(model, self.cs)
            net = self._net
        if net.cube_size != self.cs or net.hidden != self.hidden.shape[1]:
            raise ValueError(f"front='codes': the plan was built for a {self.cs}x{self.cs}x{self.cs} net with H1 = {self.hidden.shape[1]}, "
                             f"the model is {net.cube_size}x{net.cube_size}x{net.cube_size} with H1 = {net.hidden}")
        if net.dtype != self.dtype or net.device != self.code.device:
            raise ValueError(f"front='codes': the model is {net.dtype} on {net.device}, the plan {self.dtype} on {self.code.device}")
        return net

    def score_codes(self, model):
        """scores = value head from the candidate CODES, per chunk: rc_net_first_layer -> hidden, then the rest of the encoder and
        value_net (codenet.CodeNet.value_codes).  The policy head is not run."""
        net = self.code_net(model)
        total, flat = self.A * self.nbp, self.scores.view(-1)
        for j0 in range(0, total, self.chunk):
            m = min(self.chunk, total - j0)
            t0 = j0 // self.pitch
            flat[j0:j0 + m].copy_(net.value_codes(self.code[t0:t0 + m // self.pitch], m, out=self.hidden)[:, 0])

    def score_table(self, table):
        """scores = -table[corner index] of every candidate KEY: one rcp_score_keys launch over all A * NBp slots, no net."""
        _check_table(table, self.cs, self.keys.device)
        if hasattr(table, "edge_tables"):                      # a pattern.MaxTable: the maximum, one further launch per edge table
            return table.score(self.keys, self.code, self.P, self.W, self.pitch, self.scores)
        table.score_keys(self.keys, self.P, self.W, self.pitch, self.scores)

    def select(self):
        check(_search_lib.search_lib().rc_search_select(ptr(self.flags), ptr(self.keys), ptr(self.scores), self.P, self.W, self.pitch, self.cs,
                                                        ptr(self.live), ptr(self.active), ptr(self.length), ptr(self.solution), ptr(self.depth),
                                                        ptr(self.sel_parent), ptr(self.sel_action), ptr(self.sel_count), ptr(self.workspace),
                                                        self.workspace.numel(), stream_ptr(self.dev)))

    def advance(self, parity):
        check(_search_lib.search_lib().rc_search_advance(ptr(self.beams[parity]), ptr(self.beams[1 - parity]), self.P, self.W, self.pitch,
                                                         self.cs, ptr(self.sel_parent), ptr(self.sel_action), ptr(self.sel_count), ptr(self.live),
                                                         ptr(self.last_action), ptr(self.hist_parent), ptr(self.hist_action), ptr(self.depth),
                                                         max(self.D, 1), stream_ptr(self.dev)))

    def backtrack(self):
        check(_search_lib.search_lib().rc_search_backtrack(ptr(self.hist_parent), ptr(self.hist_action), self.P, self.W, self.pitch, self.cs,
                                                           max(self.D, 1), ptr(self.length), ptr(self.solution), ptr(self.actions),
                                                           stream_ptr(self.dev)))

    def step(self, model, parity):
        """One depth: beam `parity` -> beam 1 - parity.  Stream-ordered, no host synchronisation (capturable as a linear hipGraph)."""
        self.expand(parity)
        self.score(model)
        self.select()
        self.advance(parity)
        self.depth.add_(1)


def _check_table(table, cube_size, device=None):
    """front="table": the ValueErrors of a `model` that is no CornerTable (or MaxTable, the 3x3x3's maximum of a corner table and edge
    tables) of this cube size on this device (before any launch; the device is looked at last, and only where one is given)."""
    from .pattern import CornerTable, MaxTable
    if not isinstance(table, (CornerTable, MaxTable)):
        raise ValueError(f"front='table' scores with a pattern.CornerTable in the model position, got {type(table).__name__}")
    if table.cube_size != cube_size:
        raise ValueError(f"front='table': the table is a {table.cube_size}x{table.cube_size}x{table.cube_size}'s, the cubes are "
                         f"{cube_size}x{cube_size}x{cube_size}")
    if device is not None and table.device != device:
        raise ValueError(f"front='table': the table is on {table.device}, the cubes on {device}")


def _net_front(model, front, env):
    """(model, dtype, hidden) a plan scores the cubes of `env` with: for front="codes" the model's CodeNet and its H1; for
    front="table" the CornerTable itself (scores are float32, there is no net)."""
    if front not in FRONTS:
        raise ValueError(f"front must be 'dense', 'codes' or 'table', got {front!r}")
    if front == "table":
        _check_table(model, env.cube_size)                     # what needs no device first: the env's stickers are not touched yet
        _check_table(model, env.cube_size, env.stickers.device)
        return model, torch.float32, None
    from .adi import _module_dtype
    if front == "dense":
        return model, _module_dtype(model), None
    from .codenet import CodeNet
    model = model if isinstance(model, CodeNet) else CodeNet(model, env.cube_size)      # ValueError for a float16 model
    if model.device != env.stickers.device:
        raise ValueError(f"front='codes': the model is on {model.device}, the cubes on {env.stickers.device}")
    return model, model.dtype, model.hidden


def _run_steps(step, n_steps, active, dev, graph, sync_every, key=lambda t: 0):
    """The step loop of a search: step(key(t)) for t = 1..n_steps, until a host check every `sync_every` steps finds no problem
    `active`.  graph=True: step 1 runs eagerly on a side stream (warm-up outside capture: libraries pick their kernels there), every
    later step replays a hipGraph captured once per key.  Returns how many steps ran."""
    graphs, ran = {}, 0
    for t in range(1, n_steps + 1):
        k = key(t)
        if not graph:
            step(k)
        elif t == 1:
            s = torch.cuda.Stream(dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                step(k)
            torch.cuda.current_stream(dev).wait_stream(s)
        else:
            if k not in graphs:
                graphs[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[k]):              # capture does not execute
                    step(k)
            graphs[k].replay()
        ran = t
        if t % sync_every == 0 and not bool(active.any()):
            break
    return ran


@torch.no_grad()
def beam_search(model, env, width, max_depth, *, dense_budget_bytes=1 << 30, sync_every=4, graph=False, front="dense"):
    """Beam search from every cube of `env` (a VecCubeEnv, any observation mode; its state is left unchanged).

    Each depth expands the beam, scores the children with the value head model(onehot)[0][:, 0] in the model's dtype, and keeps the
    `width` best distinct children per cube (ties: the lower candidate index c = slot * A + action); a cube is solved at the first
    depth where a child is solved.  "All cubes done" is checked on the host every `sync_every` depths.  graph=True replays one
    depth step as a hipGraph (two captures: the two directions of the beam ping-pong); the results equal the eager run's.
    front="codes": the net's first layer is summed from the candidate codes by rc_net_first_layer (codenet.CodeNet; the model must have
    the reference's layout, be float32 or bfloat16 and live on the cubes' device); the default "dense" feeds model() dense one-hots.

    Returns dict(solved bool [P], length int32 [P] (0: the root was solved, -1: not solved within max_depth), actions uint8
    [max_depth, P]: the solution's moves, then the no-op action_dim)."""
    model, dtype, hidden = _net_front(model, front, env)
    plan = BeamPlan(env.num_envs, env.cube_size, width, max_depth, env.device, dtype, dense_budget_bytes, front, hidden)
    plan.init(env.stickers, env.stickers.shape[-1])
    _run_steps(lambda parity: plan.step(model, parity), plan.D, plan.active, plan.dev, graph, sync_every, key=lambda t: (t - 1) & 1)
    if plan.D:
        plan.backtrack()
    actions = plan.actions[:plan.D]
    return {"solved": plan.length >= 0, "length": plan.length, "actions": actions}


POOL_BUDGET_BYTES = 8 << 30           # astar_search's default capacity keeps pool + table under this many bytes


def pool_node_bytes(cube_size):
    """Bytes one pool node costs: stickers, key words, parent, action, g, score, prio, state, and its share of the persistent table
    (2 to 4 slots of 8 bytes: a power of two >= 2 * P * C; 4 is counted)."""
    S = ops._size(cube_size)[0]
    return S + 8 * KEY_WORDS[cube_size] + 4 + 1 + 4 + 4 + 4 + 1 + 32


def _check_astar(n_problems, batch, weight, capacity):
    """The ValueErrors of an A* shape; capacity None: astar_capacity() will choose it, within these limits by construction."""
    import math
    if not 1 <= int(batch) <= MAX_WIDTH:
        raise ValueError(f"batch must be in 1..{MAX_WIDTH}")
    if int(n_problems) < 1 or (capacity is not None and (int(capacity) < 1 or int(n_problems) * int(capacity) >= 1 << 31)):
        raise ValueError("need n_problems >= 1, capacity >= 1 and n_problems * capacity < 2^31")
    if not (math.isfinite(float(weight)) and float(weight) >= 0.0):
        raise ValueError(f"weight must be finite and >= 0, got {weight!r}")


class AStarPlan:
    """Device buffers of one batch-weighted A* shape (P problems, B nodes popped per iteration, pool capacity C) and the launches of one
    iteration.  Layouts and THE RULE: include/rubiksearch.h "Batch-weighted A*".  It owns a BeamPlan of width B (self.beam: expand,
    score, the candidate arrays) plus the node pool.  One method per entry point; tests drive them one by one."""

    def __init__(self, n_problems, cube_size, batch, capacity, device, dtype=torch.float32, dense_budget_bytes=1 << 30, front="dense",
                 hidden=None, weight=1.0):
        _check_astar(n_problems, batch, weight, capacity)
        if cube_size not in KEY_WORDS:
            raise ValueError(f"cube_size must be 2 or 3, got {cube_size!r}")
        self.beam = BeamPlan(n_problems, cube_size, batch, 0, device, dtype, dense_budget_bytes, front, hidden)   # its ValueErrors too
        b = self.beam
        self.P, self.B, self.C, self.cs, self.weight = b.P, b.W, int(capacity), b.cs, float(weight)
        self.S, self.A, self.dev = b.S, b.A, b.dev
        self.np = n = self.P * self.C
        self.ppitch = beam_pitch(n)
        self.ptiles = -(-n // self.ppitch)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
        self.stickers = z((self.ptiles, self.S, self.ppitch), torch.uint8)
        self.keys = z((KEY_WORDS[self.cs], n), torch.int64)                     # uint64 words
        self.parent, self.g = z(n, torch.int32), z(n, torch.int32)
        self.action, self.state = z(n, torch.uint8), z(n, torch.uint8)
        self.node_score, self.prio = z(n, torch.float32), z(n, torch.float32)   # node_score: the rule's `score` (score() is the net)
        self.count, self.overflow = z(self.P, torch.int32), z(self.P, torch.uint8)
        self.ended = z(self.P, torch.int32)
        self.solution = z((self.P, 2), torch.int32)                             # (parent node, action)
        self.pop_node = z(self.P * self.B, torch.int32)
        self.iteration = z(1, torch.int32)
        self.actions = None
        from . import _astar_lib
        self.table = torch.empty(_astar_lib.workspace_bytes(self.cs, self.P, self.C), dtype=torch.uint8, device=self.dev)

    # ------------------------------------------------------------------ one entry point each
    def _pool(self):
        return (ptr(self.stickers), ptr(self.keys), ptr(self.parent), ptr(self.action), ptr(self.g), ptr(self.node_score), ptr(self.prio),
                ptr(self.state))

    def init(self, roots, root_pitch):
        from ._astar_lib import astar_lib
        _lib.init(self.dev)
        b = self.beam
        check(astar_lib().rca_init(ptr(roots), self.P, root_pitch, self.cs, self.C, self.ppitch, *self._pool(), ptr(self.count),
                                   ptr(self.overflow), ptr(b.live), ptr(b.active), ptr(b.length), ptr(self.solution), ptr(self.ended),
                                   ptr(self.table), self.table.numel(), stream_ptr(self.dev)))
        self.iteration.fill_(1)

    def pop(self):
        from ._astar_lib import astar_lib
        b = self.beam
        check(astar_lib().rca_pop(self.P, self.cs, self.B, self.C, self.ppitch, ptr(self.stickers), ptr(self.action), ptr(self.prio),
                                  ptr(self.state), ptr(self.count), ptr(self.iteration), ptr(b.beams[0]), b.pitch, ptr(b.last_action),
                                  ptr(b.live), ptr(b.active), ptr(self.ended), ptr(self.pop_node), stream_ptr(self.dev)))

    def expand(self):
        self.beam.expand(0)

    def score(self, model):
        self.beam.score(model)

    def merge(self):
        from ._astar_lib import astar_lib
        b = self.beam
        check(astar_lib().rca_merge(self.P, self.cs, self.B, b.pitch, self.C, self.ppitch, self.weight, ptr(b.flags), ptr(b.keys),
                                    ptr(b.scores), ptr(b.live), ptr(b.active), ptr(b.length), ptr(self.solution), ptr(self.ended),
                                    ptr(self.iteration), ptr(self.pop_node), *self._pool(), ptr(self.count), ptr(self.overflow),
                                    ptr(self.table), self.table.numel(), ptr(b.workspace), b.workspace.numel(), stream_ptr(self.dev)))

    def relax(self):
        """rcp_relax (front="table" only): an OPEN node that this iteration's candidates reach by fewer moves takes the lower g, the new
        parent and the prio that follows -- what makes the table-guided search A* proper (include/rubiksearch.h)."""
        from ._pattern_lib import pattern_lib
        b = self.beam
        check(pattern_lib().rcp_relax(self.P, self.cs, self.B, b.pitch, self.C, self.weight, ptr(b.flags), ptr(b.keys), ptr(b.live),
                                      ptr(b.active), ptr(self.pop_node), ptr(self.keys), ptr(self.parent), ptr(self.action), ptr(self.g),
                                      ptr(self.node_score), ptr(self.prio), ptr(self.state), ptr(self.count), ptr(self.table),
                                      self.table.numel(), stream_ptr(self.dev)))

    def backtrack(self, max_length):
        """actions uint8 [max_length, P] (kept as self.actions): the solutions' moves, then the no-op."""
        from ._astar_lib import astar_lib
        b = self.beam
        self.actions = torch.zeros((max(int(max_length), 1), self.P), dtype=torch.uint8, device=self.dev)
        check(astar_lib().rca_backtrack(self.P, self.cs, self.C, ptr(self.parent), ptr(self.action), ptr(b.length), ptr(self.solution),
                                        ptr(self.actions), self.actions.shape[0], stream_ptr(self.dev)))
        return self.actions

    def step(self, model):
        """One iteration.  Stream-ordered, no host synchronisation (capturable as a linear hipGraph; there is no ping-pong)."""
        self.pop()
        self.expand()
        self.score(model)
        self.merge()
        if self.beam.front == "table":
            self.relax()
        self.iteration.add_(1)


def astar_capacity(n_problems, cube_size, batch, max_iterations, budget_bytes=POOL_BUDGET_BYTES):
    """astar_search's default pool capacity: 1 + batch * (A - 1) * max_iterations nodes per problem (the root, and at most A - 1 new
    states per popped node: one child undoes the parent's move), capped so that P * C * pool_node_bytes stays under budget_bytes and
    P * C under 2^31; never below 1."""
    A = ops._size(cube_size)[1]
    want = 1 + int(batch) * (A - 1) * int(max_iterations)
    cap = min(int(budget_bytes) // (pool_node_bytes(cube_size) * int(n_problems)), ((1 << 31) - 1) // int(n_problems))
    return max(1, min(want, cap))


@torch.no_grad()
def astar_search(model, env, batch, max_iterations, *, weight=1.0, capacity=None, front="dense", dense_budget_bytes=1 << 30, sync_every=4,
                 graph=False):
    """Batch-weighted A* (DeepCubeA's search without its re-opening rule; include/rubiksearch.h has THE RULE) from every cube of `env`
    (a VecCubeEnv, any observation mode; its state is left unchanged).

    Per cube a pool holds every state ever generated.  Each iteration pops the `batch` open nodes with the best value - weight * g
    (ties: the newer node), expands them, scores the children with the value head as beam_search does (front as there) and appends the
    states the pool has not seen; a cube is solved at the first iteration a child is solved.  capacity: nodes per cube, default
    astar_capacity(...) (pool and table under POOL_BUDGET_BYTES); a full pool drops new states and sets overflow.  "All cubes done"
    is checked on the host every `sync_every` iterations.  front="table" (a pattern.CornerTable as the model) adds rcp_relax to every
    iteration: an open node reached again by fewer moves takes the lower g, so that with batch = 1 and weight = 1 the solution is optimal
    under the table's admissible bound; the net fronts keep the rule as it is.  graph=True replays one iteration as a hipGraph (one capture, after a warm-up
    iteration on a side stream); the results equal the eager run's.

    Returns dict(solved bool [P], length int32 [P] (0: the root was solved, -1: not solved), actions uint8 [L, P] with
    L = max(1, length.max()): the solution's moves, then the no-op action_dim, iterations int32 [P]: the iteration at which the cube
    was solved or found exhausted (0: solved root; the number of iterations run for a cube still active at the end), nodes int32 [P],
    overflow bool [P], capacity int)."""
    P, cs = env.num_envs, env.cube_size
    _check_astar(P, batch, weight, capacity)                   # before astar_capacity() and the model are touched; the plan repeats it
    if int(max_iterations) < 0 or int(sync_every) < 1:
        raise ValueError("need max_iterations >= 0 and sync_every >= 1")
    if capacity is None:
        capacity = astar_capacity(P, cs, batch, max_iterations)
    model, dtype, hidden = _net_front(model, front, env)
    plan = AStarPlan(P, cs, batch, capacity, env.device, dtype, dense_budget_bytes, front, hidden, weight)
    plan.init(env.stickers, env.stickers.shape[-1])
    ran = _run_steps(lambda _: plan.step(model), int(max_iterations), plan.beam.active, plan.dev, graph, sync_every)
    length = plan.beam.length
    actions = plan.backtrack(max(1, int(length.max())))
    iterations = torch.where(plan.beam.active != 0, torch.full_like(plan.ended, ran), plan.ended)
    return {"solved": length >= 0, "length": length, "actions": actions, "iterations": iterations, "nodes": plan.count,
            "overflow": plan.overflow != 0, "capacity": int(capacity)}


def symmetry_indices(symmetries, cube_size):
    """beam_search_symmetric's `symmetries` -> list of indices into tables.get_symmetries(cube_size)."""
    from .tables import get_symmetries
    K = get_symmetries(cube_size).count
    if isinstance(symmetries, str):
        if symmetries not in ("rotations", "all"):
            raise ValueError(f"symmetries must be 'rotations', 'all' or a sequence of indices, got {symmetries!r}")
        return list(range(K // 2 if symmetries == "rotations" else K))
    idx = [int(s) for s in symmetries]
    if not idx or any(not 0 <= s < K for s in idx):
        raise IndexError(f"symmetries must be a non-empty sequence of indices in 0..{K - 1}")
    return idx


@torch.no_grad()
def beam_search_symmetric(model, env, width, max_depth, symmetries="rotations", return_all=False, **beam_kwargs):
    """beam_search from several orientations of every cube of `env`, keeping the shortest answer (`env` is left as it is).

    A symmetry maps a cube at distance d to a cube at distance d and a solution to a solution, but the net is not symmetry-invariant:
    the images of one cube get different beams.  symmetries: "rotations" (the first half of tables.get_symmetries), "all", or a
    sequence of indices.  ONE VecCubeEnv of k * P cubes is built, image-major -- cube j * P + p is image symmetries[j] of cube p (one
    rcs_sym_apply launch) -- and beam_search(model, that env, width, max_depth, **beam_kwargs) runs once.  Every action list is
    mapped back to the original cube with amap[inverse[s]]; per cube the shortest solved image wins, ties to the lowest j.

    Returns beam_search's dict (solved bool [P], length int32 [P], actions uint8 [max_depth, P]) plus symmetry int32 [P]: the chosen
    index, -1 where no image was solved.  return_all=True adds all_length int32 [k, P] and all_actions uint8 [k, max_depth, P], the
    latter mapped back as well."""
    from .tables import get_symmetries
    from .vec_env import VecCubeEnv
    if beam_kwargs.get("front") == "table":
        _check_table(model, env.cube_size)                     # before the images are built on the device
    P, cs, dev = env.num_envs, env.cube_size, env.device
    y = get_symmetries(cs)
    idx = symmetry_indices(symmetries, cs)
    k, A = len(idx), env.action_dim
    big = VecCubeEnv(k * P, dev, cs, obs=None)
    tiles, S, pitch = big.stickers.shape
    rows = torch.zeros((tiles * pitch, S), dtype=torch.uint8, device=dev)
    rows[:k * P] = ops.to_aos(env.stickers, P).repeat(k, 1)
    src = rows.view(tiles, pitch, S).permute(0, 2, 1).contiguous()
    sym = torch.tensor(idx, dtype=torch.uint8).repeat_interleave(P).to(dev)
    ops.apply_symmetry(src, k * P, None, cs, sym, out=big.stickers, bad=torch.zeros(1, dtype=torch.uint8, device=dev))   # indices checked above
    res = beam_search(model, big, width, max_depth, **beam_kwargs)
    D = res["actions"].shape[0]
    back = torch.from_numpy(y.amap[y.inverse[idx]].astype("int64")).to(dev)              # [k, A + 1]: image j's action -> the cube's own
    all_actions = back[torch.arange(k, device=dev)[None, :, None], res["actions"].view(D, k, P).long()].to(torch.uint8)
    all_length = res["length"].view(k, P)
    # the shortest solved image, ties to the lowest j: one key per (length, j), unsolved images last
    key = torch.where(all_length >= 0, all_length.long(), torch.full_like(all_length, max_depth + 1, dtype=torch.long)) * k + \
        torch.arange(k, device=dev)[:, None]
    j = key.argmin(0)
    solved = (all_length >= 0).any(0)
    length = torch.where(solved, all_length.gather(0, j[None])[0], torch.full_like(all_length[0], -1))
    actions = all_actions.gather(1, j[None, None, :].expand(D, 1, P))[:, 0]
    actions = torch.where(solved[None], actions, torch.full_like(actions, A))
    symmetry = torch.where(solved, torch.tensor(idx, dtype=torch.int32, device=dev)[j], torch.full((P,), -1, dtype=torch.int32, device=dev))
    out = {"solved": solved, "length": length, "actions": actions, "symmetry": symmetry}
    if return_all:
        out["all_length"], out["all_actions"] = all_length, all_actions.permute(1, 0, 2).contiguous()
    return out


def _solve_percentage(solve, cube_size, sample_scramble_count, sample_cube_count, device, seeds):
    """For scramble_count = 1..sample_scramble_count, the percentage of the sample_cube_count cubes (seeds i * 10, train.py:180) that
    solve(env)["solved"] reports solved.  All (k, seed) pairs run as ONE batch."""
    from .vec_env import VecCubeEnv
    seeds = list(seeds) if seeds is not None else [i * 10 for i in range(sample_cube_count)]
    ks = [k for k in range(1, sample_scramble_count + 1) for _ in seeds]
    env = VecCubeEnv(len(ks), device, cube_size, obs=None)
    env.reset(seeds=seeds * sample_scramble_count, scramble_count=ks)
    solved = solve(env)["solved"].view(sample_scramble_count, len(seeds)).float().mean(1) * 100.0
    return [float(x) for x in solved.cpu()]


@torch.no_grad()
def beam_solve_percentage(model, cube_size, sample_scramble_count, sample_cube_count, width, max_depth, device="cuda", seeds=None,
                          graph=False, front="dense"):
    """rollout.solve_percentage with the beam search as the solver: for scramble_count = 1..sample_scramble_count, the percentage
    of the sample_cube_count cubes (seeds i * 10, train.py:180) solved within max_depth.  All (k, seed) pairs run as ONE batch."""
    if front == "table":
        _check_table(model, cube_size)                         # before the cubes are scrambled on the device
    return _solve_percentage(lambda env: beam_search(model, env, width, max_depth, graph=graph, front=front), cube_size,
                             sample_scramble_count, sample_cube_count, device, seeds)


@torch.no_grad()
def astar_solve_percentage(model, cube_size, sample_scramble_count, sample_cube_count, batch, max_iterations, device="cuda", seeds=None,
                           weight=1.0, capacity=None, graph=False, front="dense"):
    """beam_solve_percentage with astar_search as the solver: for scramble_count = 1..sample_scramble_count, the percentage of the
    sample_cube_count cubes (seeds i * 10, train.py:180) solved within max_iterations.  All (k, seed) pairs run as ONE batch."""
    if front == "table":
        _check_table(model, cube_size)                         # before the cubes are scrambled on the device
    return _solve_percentage(lambda env: astar_search(model, env, batch, max_iterations, weight=weight, capacity=capacity, graph=graph,
                                                      front=front), cube_size, sample_scramble_count, sample_cube_count, device, seeds)


def chain_solve(tables, env, graph=False):
    """Solve every cube of a 3x3x3 env by Thistlethwaite's subgroup chain (include/rubikhip.h "Subgroup chain", DESIGN.md "Subgroup
    chain"): rcc_cubies once, then one rct_descend per stage of `tables`, a pattern.ChainTables -- no net, no search, at most 87
    quarter turns.  The env is left as it is.  A cube whose legality() is nonzero is not walked: between the two, one mask sets its
    entry length to -1, which rct_descend refuses.

    Returns dict(solved bool [P], length int32 [P] (-1: not solved), actions uint8 [L, P] (padded with the no-op 12; L = max(1,
    length.max())), stage_moves uint8 [4, P] (each table's value at entry, 0xFF where the stage did not see the cube in its domain),
    status uint8 [P] (the OR of the stages' RCT_* bytes; RCT_ILLEGAL alone for an illegal cube)).
    graph=True captures the launches in one hipGraph and replays it."""
    from . import _chain_lib
    from .pattern import ChainTables
    if not isinstance(tables, ChainTables):
        raise ValueError(f"chain_solve(tables, env): tables is a pattern.ChainTables, got {type(tables).__name__}")
    if not hasattr(env, "stickers") or env.cube_size != 3:
        raise ValueError(f"chain_solve needs a 3x3x3 VecCubeEnv, got {'a ' + str(env.cube_size) + 'x' + str(env.cube_size) + 'x' + str(env.cube_size) + ' one' if hasattr(env, 'cube_size') else type(env).__name__}")
    if env.stickers.device != tables.device:
        raise ValueError(f"the tables are on {tables.device}, the cubes on {env.stickers.device}")
    n, dev, ML = env.num_envs, tables.device, _chain_lib.MAX_LENGTH
    vec = lambda dtype, rows=1: torch.empty((rows, _lib.pitch_for(n, 16)), dtype=dtype, device=dev)
    cub = ops.alloc_code(n, 3, dev, env.stickers.shape[-1])
    legal, length = vec(torch.uint8)[0], vec(torch.int32)[0]
    actions, moves, status = vec(torch.uint8, ML), vec(torch.uint8, 4), vec(torch.uint8, 4)
    p_c, ap = ops._state_arg(cub, 20, n, None, "chain_solve cubies"), actions.shape[1]
    _lib.init(dev)
    L = _chain_lib.chain_lib()

    def launches():
        ops.cubies(env.stickers, n, 3, cubies=cub, status=legal)
        actions.fill_(12)                                      # fill kernels, no memset: a captured memset is not replayed in order
        length.copy_(legal.ne(0).to(torch.int32).neg())
        for s in range(_chain_lib.STAGES):
            _lib.check(L.rct_descend(ptr(cub), n, p_c, s, ptr(tables.tables[s]), tables.tables[s].numel(), ptr(actions), ML, ap, ptr(length),
                                     ptr(moves[s]), ptr(status[s]), stream_ptr(dev)))

    if graph:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            launches()                                         # warm-up outside the capture
        torch.cuda.current_stream(dev).wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            launches()
        g.replay()
    else:
        launches()
    bad = legal[:n] != 0
    st = status[0, :n] | status[1, :n] | status[2, :n] | status[3, :n]
    st = torch.where(bad, torch.full_like(st, _chain_lib.ILLEGAL), st)
    solved = st == 0
    out_len = torch.where(solved, length[:n], torch.full_like(length[:n], -1))
    rows = max(1, int(out_len.max()))
    acts = torch.where(solved[None, :], actions[:rows, :n], torch.full_like(actions[:rows, :n], 12))
    return dict(solved=solved, length=out_len, actions=acts.contiguous(), stage_moves=moves[:, :n].contiguous(), status=st)


def _ida_members(table):
    """(corner table or None, edge tables, device or None) of ida_search's `table`: a CornerTable, an EdgeTable, a MaxTable or None."""
    from . import _ida_lib
    from .pattern import CornerTable, EdgeTable, MaxTable
    if table is None:
        return None, (), None
    if isinstance(table, CornerTable):
        corner, edges = table, ()
    elif isinstance(table, EdgeTable):
        corner, edges = None, (table,)
    elif isinstance(table, MaxTable):
        corner, edges = table.corner, table.edge_tables
    else:
        raise ValueError(f"ida_search(table, env): table is a pattern.CornerTable, EdgeTable, MaxTable or None, got {type(table).__name__}")
    if corner is not None and corner.cube_size != 3:
        raise ValueError(f"ida_search is the 3x3x3's; the corner table is a {corner.cube_size}x{corner.cube_size}x{corner.cube_size}'s")
    if len(edges) > _ida_lib.MAX_EDGE_TABLES:
        raise ValueError(f"ida_search takes at most {_ida_lib.MAX_EDGE_TABLES} edge tables, got {len(edges)}")
    return corner, tuple(edges), table.device


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _steps_args(max_steps, steps_per_call, cap, cap_name):
    """The two budgets of a depth-first search checked -> steps_per_call (None: the cap, `cap_name`() of the library)."""
    if not _is_int(max_steps) or max_steps < 1:
        raise ValueError(f"max_steps must be a positive integer, got {max_steps!r}")
    if steps_per_call is None:
        steps_per_call = cap
    if not _is_int(steps_per_call) or not 1 <= steps_per_call <= cap:
        raise ValueError(f"steps_per_call must be an integer in 1..{cap_name}() = {cap}, got {steps_per_call!r}")
    return steps_per_call


def _cube3_env(env, who):
    if not hasattr(env, "stickers") or env.cube_size != 3:
        raise ValueError(f"{who} needs a 3x3x3 VecCubeEnv, got {'a ' + str(env.cube_size) + 'x' + str(env.cube_size) + 'x' + str(env.cube_size) + ' one' if hasattr(env, 'cube_size') else type(env).__name__}")


def _cube3_cubies(env, who, dev=None):
    """The prologue of the depth-first solvers, after their argument checks (_cube3_env is the first of them): the env is on `dev`
    (None: anywhere) -> (its cubie rows from rcc_cubies, their pitch, uint8 [>= N] nonzero where the stickers are no cube)."""
    if dev is not None and env.stickers.device != dev:
        raise ValueError(f"the tables are on {dev}, the cubes on {env.stickers.device}")
    n, dev = env.num_envs, env.stickers.device
    _lib.init(dev)
    cub = ops.alloc_code(n, 3, dev, env.stickers.shape[-1])
    legal = torch.empty(_lib.pitch_for(n, 16), dtype=torch.uint8, device=dev)
    ops.cubies(env.stickers, n, 3, cubies=cub, status=legal)
    return cub, ops._state_arg(cub, 20, n, None, f"{who} cubies"), legal


class _DepthFirstFrame:
    """What the caller-owned frames of the depth-first searches share (include/rubikhip.h "Iterative-deepening A*", "Two-phase"): the
    per-lane fields, the `running` word and the loop over the launching call.  A subclass names its two exports and sets L and _args."""
    INIT = SEARCH = None

    def _alloc(self, pitch, dev):
        vec = lambda dtype: torch.zeros(pitch, dtype=dtype, device=dev)
        self.trail = torch.zeros((pitch, 2), dtype=torch.int64, device=dev)
        self.cursor, self.status = vec(torch.uint8), vec(torch.uint8)
        self.depth, self.bound, self.next = vec(torch.int32), vec(torch.int32), vec(torch.int32)
        self.nodes = vec(torch.int64)
        self.running = torch.zeros(4, dtype=torch.int32, device=dev)       # one uint32, 16-byte aligned

    def init(self):
        _lib.check(getattr(self.L, self.INIT)(*self._args, stream_ptr(self.dev)))

    def search(self, steps):
        _lib.check(getattr(self.L, self.SEARCH)(*self._args, int(steps), ptr(self.running), stream_ptr(self.dev)))

    def run(self, max_steps, steps_per_call):
        """search() until no lane runs or max_steps passes per lane are spent; one read-back per call."""
        spent = 0
        while spent < max_steps:
            k = min(steps_per_call, max_steps - spent)
            self.search(k)
            spent += k
            if int(self.running[0]) == 0:
                break
        return spent


class IdaFrame(_DepthFirstFrame):
    """The caller-owned frame of n cubes (include/rubikhip.h "Iterative-deepening A*") and the two launching calls on it.  cubies: a
    tiled cubie buffer of n cubes with pitch p_c; prefix: None or uint8 [k, n], written into path's first k rows with floor = k."""
    INIT, SEARCH = "ida_init", "ida_search"

    def __init__(self, table, cubies, n, p_c, max_depth, limit, prefix=None):
        from ctypes import c_int, c_int64, c_void_p
        from . import _ida_lib
        corner, edges, _ = _ida_members(table)
        dev = cubies.device
        self.n, self.dev, self.max_depth, self.L = n, dev, int(max_depth), _ida_lib.ida_lib()
        pitch = _lib.pitch_for(max(n, 1), 16)
        self._alloc(pitch, dev)
        self.path = torch.full((self.max_depth, pitch), _ida_lib.NOOP, dtype=torch.uint8, device=dev)
        self.floor = None
        if prefix is not None and prefix.shape[0]:
            self.path[:prefix.shape[0], :n] = prefix
            self.floor = torch.full((pitch,), prefix.shape[0], dtype=torch.int32, device=dev)
        self.limit = torch.zeros(pitch, dtype=torch.int32, device=dev)
        self.limit[:n] = limit
        k = len(edges)
        self._keep = (corner, edges, cubies)
        self._args = (ptr(cubies), n, p_c, ptr(corner.table) if corner is not None else None, corner.table.numel() if corner is not None else 0, k,
                      (c_int * max(k, 1))(*[e.mask for e in edges]), (c_void_p * max(k, 1))(*[ptr(e.table) for e in edges]),
                      (c_int64 * max(k, 1))(*[e.table.numel() for e in edges]), ptr(self.path), self.max_depth, pitch,
                      ptr(self.floor) if self.floor is not None else None, ptr(self.limit), ptr(self.trail), ptr(self.cursor), ptr(self.depth),
                      ptr(self.bound), ptr(self.next), ptr(self.nodes), ptr(self.status))


def ida_search(table, env, *, limit=20, max_steps=1 << 22, steps_per_call=None, split=0):
    """The OPTIMAL solution of every cube of a 3x3x3 env by iterative-deepening A* (include/rubikhip.h "Iterative-deepening A*" has THE
    RULE, DESIGN.md "IDA*" the numbers): depth-first under a cost bound that grows from h(start), with h the maximum of the tables
    given -- a pattern.CornerTable, EdgeTable, MaxTable, or None for h = 0.  No node is ever stored: a search is a trail of moves, so it
    keeps answering where astar_search stops for want of iterations or of pool.  The env is left as it is.  rcc_cubies runs once; a cube whose legality() is nonzero is
    not searched (status ILLEGAL).

    limit: the largest length looked for (<= 32).  max_steps: the passes (children generated + levels gone back) every cube may spend;
    steps_per_call: how many of them one launch makes (default and cap: ida_max_steps()); after each launch one uint32 is read back.
    split = k in 1..3, for batches far smaller than the device: cubes farther than k moves from solved are searched once per canonical
    move sequence of length k (12 | 114 | 1068 lanes per cube) with the limit held at the cube's bound, round by round; the answer is
    that of the lowest sequence that solved, the unsplit path byte for byte.  A round runs ONE iteration, at the cube's bound, per
    sequence; max_steps then bounds every round's searches, and nodes counts every round's.

    Returns dict(solved bool [N], length int32 [N] (-1: not solved), actions uint8 [L, N] (padded with the no-op 12; L = max(1,
    length.max())), nodes int64 [N], bound int32 [N] (solved: the length; else a PROVEN lower bound on the distance: every f below it
    was excluded), status uint8 [N] (IDA_SOLVED 1, IDA_EXHAUSTED 2: no solution within limit, IDA_ILLEGAL 4, 0: the budget ran out))."""
    from . import _ida_lib
    corner, edges, dev = _ida_members(table)
    _cube3_env(env, "ida_search")
    if not _is_int(limit) or not 0 <= limit <= _ida_lib.MAX_DEPTH:
        raise ValueError(f"limit must be an integer in 0..{_ida_lib.MAX_DEPTH}, got {limit!r}")
    if not _is_int(split) or not 0 <= split <= 3:
        raise ValueError(f"split must be an integer in 0..3, got {split!r}")
    steps_per_call = _steps_args(max_steps, steps_per_call, _ida_lib.max_steps(), "ida_max_steps")
    cub, p_c, legal = _cube3_cubies(env, "ida_search", dev)
    n, dev = env.num_envs, env.stickers.device
    max_depth = max(1, limit)

    fr = IdaFrame(table, cub, n, p_c, max_depth, min(limit, split) if split else limit)
    fr.init()
    fr.status[:n] = torch.where(legal[:n] != 0, torch.full_like(legal[:n], _ida_lib.ILLEGAL), fr.status[:n])   # not a cube: not searched
    fr.run(max_steps, steps_per_call)
    status, nodes = fr.status[:n].clone(), fr.nodes[:n].clone()
    depth, path = fr.depth[:n].clone(), fr.path[:, :n].clone()
    bound = torch.where(status == _ida_lib.EXHAUSTED, fr.next[:n], fr.bound[:n])

    if split and limit > split:
        P = torch.as_tensor(_ida_lib.prefixes(split), device=dev)          # [np, k]
        n_p = P.shape[0]
        todo = torch.nonzero(status == _ida_lib.EXHAUSTED)[:, 0]            # farther than `split` moves: bound = next > split
        todo = todo[bound[todo] <= limit]
        status[todo] = 0
        aos = ops.to_aos(cub, n)
        while todo.numel():
            m = todo.numel() * n_p
            cub2 = torch.empty((20, _lib.pitch_for(m, 16)), dtype=torch.uint8, device=dev)
            cub2[:, :m] = aos[todo].repeat_interleave(n_p, 0).T
            sub = IdaFrame(table, cub2, m, cub2.shape[1], max_depth, bound[todo].repeat_interleave(n_p), prefix=P.T.repeat(1, todo.numel()))
            sub.init()
            # every f below the cube's bound is excluded already: a sub-search starts its first iteration at that bound, not at its own
            sub.bound[:m] = torch.where(sub.status[:m] == 0, sub.limit[:m], sub.bound[:m])
            sub.run(max_steps, steps_per_call)
            st = sub.status[:m].view(-1, n_p)
            nodes[todo] += sub.nodes[:m].view(-1, n_p).sum(1)
            won = st == _ida_lib.SOLVED
            first = won.to(torch.uint8).argmax(1)                          # the lowest prefix that solved
            col = torch.arange(todo.numel(), device=dev) * n_p + first
            stuck = (st == 0).any(1) | ((st & (_ida_lib.ILLEGAL | _ida_lib.BAD_FRAME)) != 0).any(1)
            below = torch.arange(n_p, device=dev)[None, :] < first[:, None]
            hit = won.any(1) & ~((st != _ida_lib.EXHAUSTED) & below).any(1)    # no lower prefix is undecided: the unsplit search's answer
            status[todo[hit]] = _ida_lib.SOLVED
            depth[todo[hit]] = sub.depth[col[hit]]
            path[:, todo[hit]] = sub.path[:, col[hit]]
            bound[todo[hit]] = sub.depth[col[hit]]
            nxt = torch.where(st == _ida_lib.EXHAUSTED, sub.next[:m].view(-1, n_p), torch.full_like(st, 0, dtype=torch.int32) + _ida_lib.INF).min(1).values
            go = ~hit & ~stuck
            bound[todo[go]] = nxt[go]
            over = go & (nxt > limit)
            status[todo[over]] = _ida_lib.EXHAUSTED
            todo = todo[go & ~over]

    solved = status == _ida_lib.SOLVED
    length = torch.where(solved, depth, torch.full_like(depth, -1))
    bound = torch.where(solved, depth, bound)
    rows = max(1, int(length.max())) if n else 1
    acts = torch.where(solved[None, :], path[:rows], torch.full_like(path[:rows], _ida_lib.NOOP))
    return dict(solved=solved, length=length, actions=acts.contiguous(), nodes=nodes, bound=bound, status=status)


class TwoPhase1Frame(_DepthFirstFrame):
    """The caller-owned frame of phase 1 over n cubes (include/rubikhip.h "Two-phase") and its two launching calls.  cubies: a tiled
    cubie buffer of n cubes with pitch p_c; candidate (j, c) lives in column j * stride + c of path, cand_length and cand_cubies."""
    INIT, SEARCH = "tp_phase1_init", "tp_phase1_search"

    def __init__(self, tables, cubies, n, p_c, candidates, limit, max_depth=None):
        from . import _twophase_lib as T
        dev = cubies.device
        self.n, self.dev, self.K, self.L = n, dev, int(candidates), T.twophase_lib()
        self.max_depth = T.MAX_DEPTH if max_depth is None else int(max_depth)
        self.stride = stride = _lib.pitch_for(max(n, 1), 16)
        self.cols = cols = self.K * stride
        self._alloc(stride, dev)
        self.path = torch.full((self.max_depth, cols), T.NOOP, dtype=torch.uint8, device=dev)
        self.cand_length = torch.zeros(cols, dtype=torch.int32, device=dev)
        self.cand_cubies = torch.zeros((20, cols), dtype=torch.uint8, device=dev)
        self.cand_cubies += torch.tensor([3 * q for q in range(8)] + [2 * q for q in range(12)], dtype=torch.uint8, device=dev)[:, None]
        self.limit = torch.zeros(stride, dtype=torch.int32, device=dev)
        self.limit[:n] = limit
        self.found = torch.zeros(stride, dtype=torch.int32, device=dev)
        a, b = tables.tables[0], tables.tables[1]
        self._keep = (tables, cubies)
        self._args = (ptr(cubies), n, p_c, ptr(a), a.numel(), ptr(b), b.numel(), ptr(self.limit), self.K, stride, ptr(self.path), self.max_depth,
                      cols, ptr(self.cand_length), ptr(self.cand_cubies), cols, ptr(self.trail), ptr(self.cursor), ptr(self.depth),
                      ptr(self.bound), ptr(self.next), ptr(self.nodes), ptr(self.found), ptr(self.status))


class TwoPhase2Frame(_DepthFirstFrame):
    """The caller-owned frame of phase 2 over n columns and its two launching calls.  cubies [20, pitch >= n]: the G1 roots; path
    uint8 [max_depth, pitch]: the prefixes (rows below floor) and the room for the answers; floor, limit: int32 [>= n]."""
    INIT, SEARCH = "tp_phase2_init", "tp_phase2_search"

    def __init__(self, tables, cubies, n, p_c, path, floor, limit):
        from . import _twophase_lib as T
        dev = cubies.device
        self.n, self.dev, self.L, self.path, self.floor, self.limit = n, dev, T.twophase_lib(), path, floor, limit
        self._alloc(_lib.pitch_for(max(n, 1), 16), dev)
        a, b = tables.tables[2], tables.tables[3]
        self._keep = (tables, cubies)
        self._args = (ptr(cubies), n, p_c, ptr(a), a.numel(), ptr(b), b.numel(), ptr(path), path.shape[0], path.shape[1],
                      ptr(floor) if floor is not None else None, ptr(limit), ptr(self.trail), ptr(self.cursor), ptr(self.depth), ptr(self.bound),
                      ptr(self.next), ptr(self.nodes), ptr(self.status))


TWO_PHASE_DESCENT_ROWS = 58        # quarter turns of the chain's stages 2 and 3 at the most: 2 * 14 + 2 * 15


def two_phase_select(K, chain_length, cand_length, found, descent, status2, depth2):
    """Step 7 of two_phase_solve in torch indexing: per cube the candidate with the smallest total -- its phase-2 length where the
    column is SOLVED, else its phase-1 length plus its descent; index K is chain_solve's answer; the FIRST minimum in index order wins.
    cand_length, descent, status2, depth2: [K, N]; chain_length, found: [N].  -> (candidate int64 [N], total int32 [N], source uint8
    [N]: 0 chain, 1 descent, 2 phase 2)."""
    from . import _twophase_lib as T
    dev = chain_length.device
    big = torch.full((), T.INF, dtype=torch.int32, device=dev)
    slot = torch.arange(K, device=dev)[:, None]
    won = status2 == T.SOLVED
    total = torch.where(won, depth2, cand_length + descent)
    total = torch.where(slot < found[None, :], total, big)
    total = torch.cat([total, chain_length[None, :].to(torch.int32)])          # [K + 1, N]
    best = total.min(0).values
    index = torch.arange(K + 1, device=dev)[:, None].expand_as(total)
    cand = torch.where(total == best[None, :], index, torch.full_like(index, K + 1)).min(0).values
    pick = won.gather(0, cand.clamp(max=K - 1)[None, :])[0]
    source = torch.where(cand == K, 0, torch.where(pick, 2, 1)).to(torch.uint8)
    return cand, best, source


def two_phase_solve(tables, chain, env, *, candidates=64, phase1_limit=16, phase2_limit=20, max_steps=100000, steps_per_call=None):
    """A SHORT solution of every cube of a 3x3x3 env by Kociemba's two-phase algorithm (include/rubikhip.h "Two-phase" has THE RULE,
    DESIGN.md "Two-phase" the numbers).  tables: a pattern.TwoPhaseTables; chain: a pattern.ChainTables.  The env is left as it is.
      1  rcc_cubies and legality; an illegal cube is not searched;
      2  phase 1: up to `candidates` ways into G1 per cube, none longer than phase1_limit, within max_steps passes per cube;
      3  the chain's stages 2 and 3 (rct_descend) finish EVERY candidate: a guaranteed completion;
      4  chain_solve's own answer is candidate number `candidates`;
      5  phase 2 looks, per candidate, for something strictly shorter than the cube's shortest guaranteed length G: its limit is
         min(48, phase-1 length + phase2_limit, G - 1), within max_steps passes per candidate;
      6  per cube the shortest of all wins, the first in candidate order among equals.
    steps_per_call: passes per launch (default and cap: tp_max_steps()); one uint32 is read back per launch.

    Returns dict(solved bool [N], length int32 [N] (-1: not solved), actions uint8 [L, N] (padded with the no-op 12; L = max(1,
    length.max())), source uint8 [N] (0 chain, 1 phase 1 + descent, 2 phase 1 + phase 2), candidate int64 [N] (the winner's slot,
    `candidates` for the chain, -1 unsolved), phase1_length int32 [N] (-1 for the chain), chain_length int32 [N], nodes int64 [2, N]
    (children generated by phase 1, and by phase 2 over the cube's candidates), status uint8 [N] (phase 1's: 0 the budget ran out,
    TP_FULL 1, TP_EXHAUSTED 2: every way within phase1_limit was seen, TP_ILLEGAL 4))."""
    return two_phase_frames(tables, chain, env, candidates=candidates, phase1_limit=phase1_limit, phase2_limit=phase2_limit, max_steps=max_steps,
                            steps_per_call=steps_per_call)[0]


def two_phase_frames(tables, chain, env, *, candidates=64, phase1_limit=16, phase2_limit=20, max_steps=100000, steps_per_call=None):
    """two_phase_solve, and what it chose from: (its result, dict(one: the TwoPhase1Frame, two: the TwoPhase2Frame, descent int32
    [K, N]: every candidate's guaranteed completion beyond its phase-1 length, limit2 int32 [K, N], chain: chain_solve's result))."""
    from . import _chain_lib, _twophase_lib as T
    from .pattern import ChainTables, TwoPhaseTables
    if not isinstance(tables, TwoPhaseTables):
        raise ValueError(f"two_phase_solve(tables, chain, env): tables is a pattern.TwoPhaseTables, got {type(tables).__name__}")
    if not isinstance(chain, ChainTables):
        raise ValueError(f"two_phase_solve(tables, chain, env): chain is a pattern.ChainTables, got {type(chain).__name__}")
    _cube3_env(env, "two_phase_solve")
    if not _is_int(candidates) or not 1 <= candidates <= T.MAX_CANDIDATES:
        raise ValueError(f"candidates must be an integer in 1..{T.MAX_CANDIDATES}, got {candidates!r}")
    if not _is_int(phase1_limit) or not 0 <= phase1_limit <= T.MAX_TRAIL:
        raise ValueError(f"phase1_limit must be an integer in 0..{T.MAX_TRAIL}, got {phase1_limit!r}")
    if not _is_int(phase2_limit) or not 0 <= phase2_limit <= T.MAX_TRAIL:
        raise ValueError(f"phase2_limit must be an integer in 0..{T.MAX_TRAIL}, got {phase2_limit!r}")
    steps_per_call = _steps_args(max_steps, steps_per_call, T.max_steps(), "tp_max_steps")
    if chain.device != tables.device:
        raise ValueError(f"the two-phase tables are on {tables.device}, the chain's on {chain.device}")
    cub, p_c, legal = _cube3_cubies(env, "two_phase_solve", tables.device)
    n, dev, K = env.num_envs, tables.device, candidates
    bad = legal[:n] != 0

    one = TwoPhase1Frame(tables, cub, n, p_c, K, phase1_limit)
    one.init()
    one.status[:n] = torch.where(bad, torch.full_like(one.status[:n], T.ILLEGAL), one.status[:n])    # not a cube: not searched
    one.found[:n] = torch.where(bad, torch.zeros_like(one.found[:n]), one.found[:n])
    one.run(max_steps, steps_per_call)
    stride, cols = one.stride, one.cols
    found = one.found[:n]
    emitted = (torch.arange(K, device=dev)[:, None] < one.found[None, :]).reshape(cols)

    # the guaranteed completion of every candidate: the chain's stages 2 and 3 on a copy of the candidates' rows
    walk = one.cand_cubies.clone()
    d_act = torch.full((TWO_PHASE_DESCENT_ROWS, cols), T.NOOP, dtype=torch.uint8, device=dev)
    d_len = emitted.to(torch.int32) - 1                                        # 0, and -1 for an empty slot: rct_descend refuses it
    d_moves, d_status = torch.empty(cols, dtype=torch.uint8, device=dev), torch.empty((2, cols), dtype=torch.uint8, device=dev)
    CL = _chain_lib.chain_lib()
    for i, s in enumerate((2, 3)):
        _lib.check(CL.rct_descend(ptr(walk), cols, cols, s, ptr(chain.tables[s]), chain.tables[s].numel(), ptr(d_act), TWO_PHASE_DESCENT_ROWS,
                                  cols, ptr(d_len), ptr(d_moves), ptr(d_status[i]), stream_ptr(dev)))
    walked = emitted & (d_status[0] == 0) & (d_status[1] == 0)
    ch = chain_solve(chain, env)
    chain_length = torch.where(ch["solved"], ch["length"], torch.full_like(ch["length"], T.INF))

    len1 = one.cand_length.view(K, stride)[:, :n]
    descent = torch.where(walked, d_len, torch.full_like(d_len, T.INF // 2)).view(K, stride)[:, :n]
    slot = torch.arange(K, device=dev)[:, None]
    sure = torch.where(slot < found[None, :], len1 + descent, torch.full_like(len1, T.INF))
    G = torch.minimum(sure.min(0).values, chain_length.to(torch.int32))       # the cube's shortest guaranteed length
    limit2 = torch.full((K, stride), -1, dtype=torch.int32, device=dev)
    limit2[:, :n] = torch.where(slot < found[None, :], torch.minimum(len1 + phase2_limit, (G - 1)[None, :]).clamp(max=T.MAX_DEPTH),
                                torch.full_like(len1, -1))
    two = TwoPhase2Frame(tables, one.cand_cubies, cols, cols, one.path, one.cand_length, limit2.view(cols))
    two.init()
    two.run(max_steps, steps_per_call)

    cand, total, source = two_phase_select(K, chain_length.to(torch.int32), len1, found, descent, two.status.view(K, stride)[:, :n],
                                           two.depth.view(K, stride)[:, :n])
    solved = ~bad & (total < T.INF // 2)
    length = torch.where(solved, total, torch.full_like(total, -1))
    rows = max(1, int(length.max())) if n else 1
    col = cand.clamp(max=K - 1) * stride + torch.arange(n, device=dev)
    p1 = torch.where(cand < K, one.cand_length[col], torch.full_like(total, -1))
    r = torch.arange(rows, device=dev)[:, None]
    head = one.path[:, col][:rows] if rows <= one.path.shape[0] else torch.cat(
        [one.path[:, col], torch.full((rows - one.path.shape[0], n), T.NOOP, dtype=torch.uint8, device=dev)])
    tail = d_act[:, col].gather(0, (r - p1[None, :]).clamp(0, TWO_PHASE_DESCENT_ROWS - 1))
    acts = torch.where((source == 2)[None, :] | (r < p1[None, :]), head, tail)
    ca = ch["actions"]
    ca = ca[:rows] if ca.shape[0] >= rows else torch.cat([ca, torch.full((rows - ca.shape[0], n), T.NOOP, dtype=torch.uint8, device=dev)])
    acts = torch.where((source == 0)[None, :], ca, acts)
    acts = torch.where(solved[None, :] & (r < length[None, :]), acts, torch.full_like(acts, T.NOOP))
    nodes = torch.stack([one.nodes[:n], two.nodes.view(K, stride)[:, :n].sum(0)])
    res = dict(solved=solved, length=length, actions=acts.contiguous(), source=torch.where(solved, source, torch.zeros_like(source)),
               candidate=torch.where(solved, cand, torch.full_like(cand, -1)), phase1_length=torch.where(solved, p1, torch.full_like(p1, -1)),
               chain_length=ch["length"], nodes=nodes, status=one.status[:n].clone())
    return res, dict(one=one, two=two, descent=descent, limit2=limit2[:, :n], chain=ch)


# ------------------------------------------------------------------------------------------------------------------- cube group
# include/rubikhip.h "Cube group", DESIGN.md "Cube group": what the solvers gain from products and inverses of whole cubes.
def _goal_cubies(env, goal, who):
    SL = ops.N_SLOTS[env.cube_size]
    if hasattr(goal, "stickers"):
        if (goal.num_envs, goal.cube_size, goal.device) != (env.num_envs, env.cube_size, env.device):
            raise ValueError(f"{who}: the goal env must have the same num_envs, cube_size and device")
        return goal.cubies()
    if isinstance(goal, torch.Tensor) and goal.dim() == 3 and goal.shape[1] == SL and goal.dtype == torch.uint8:
        return goal.to(env.device)
    raise ValueError(f"{who}: goal must be a VecCubeEnv or a tiled uint8 cubie tensor [tiles, {SL}, pitch]")


def relative_to(env, goal):
    """A new env whose cube i is goal_i^-1 o x_i: any solver's answer for it, played on x_i, ends at goal_i instead of at solved.
    goal: a VecCubeEnv of the same size and device, or a tiled cubie tensor.  env and goal are left as they are; a goal or a cube
    that is no permutation of the pieces raises ValueError."""
    n, cs = env.num_envs, env.cube_size
    g = _goal_cubies(env, goal, "relative_to")
    inv = ops.group_inverse(g, n, cs)
    out = env.clone()
    out.from_cubies(ops.group_product(inv, env.cubies(), n, cs))
    return out


def invert_actions(actions, cube_size=3):
    """The inverse of a solver's `actions` uint8 [L, N] (padded with the no-op at the end): per column the moves in reverse order, each
    replaced by its inverse a ^ 1, padded again at the end -- a solution turned into a scramble, or the answer for the inverse cube
    mapped back (one cg_invert_actions launch).  Returns uint8 [L, N]."""
    if not isinstance(actions, torch.Tensor) or actions.dtype != torch.uint8 or actions.dim() != 2 or not actions.is_cuda:
        raise ValueError("invert_actions: actions is a uint8 HIP tensor [L, N]")
    L, n = actions.shape
    buf = torch.full((L, _lib.pitch_for(n, 16)), get_env_config(cube_size)[1], dtype=torch.uint8, device=actions.device)
    buf[:, :n] = actions
    return ops.invert_actions(buf, n, cube_size, out=buf)[:, :n].contiguous()


def _rows_to(actions, rows, noop=12):
    L, n = actions.shape
    if L >= rows:
        return actions[:rows]
    return torch.cat([actions, torch.full((rows - L, n), noop, dtype=torch.uint8, device=actions.device)])


def two_phase_solve_both(tables, chain, env, **kw):
    """two_phase_solve on every cube AND on its inverse (Kociemba's standard trick: the two searches see different cubes): the inverse
    cube's answer, inverted by invert_actions, solves the cube itself; per cube the shorter one wins, the plain one among equals, so
    `length` is never above two_phase_solve's.  kw: two_phase_solve's keywords.  The env is left as it is.
    Returns two_phase_solve's keys, each taken from the winning side (nodes: the sum of both sides, the work done), and side uint8
    [N]: 0 plain, 1 inverse.  An illegal cube is side 0 and unsolved, as in two_phase_solve."""
    _cube3_env(env, "two_phase_solve_both")
    n, dev = env.num_envs, env.stickers.device
    plain = two_phase_solve(tables, chain, env, **kw)
    c = ops.cubies(env.stickers, n, 3)
    flag = torch.zeros(1, dtype=torch.uint8, device=dev)          # set for cubes that are no cube; those stay on the plain side
    other = env.clone()
    other.stickers.copy_(ops.from_cubies(ops.group_inverse(c["cubies"], n, 3, bad=flag), n, 3, out=torch.empty_like(env.stickers)))
    inv = two_phase_solve(tables, chain, other, **kw)
    big = torch.full_like(plain["length"], 2 ** 30)
    use = (c["status"][:n] == 0) & inv["solved"] & (torch.where(inv["solved"], inv["length"], big) < torch.where(plain["solved"], plain["length"], big))
    out = {}
    for k, a in plain.items():
        b = inv[k]
        if k == "actions":
            rows = max(a.shape[0], b.shape[0])
            out[k] = torch.where(use[None, :], _rows_to(invert_actions(b), rows), _rows_to(a, rows))
        elif k == "nodes":
            out[k] = a + b
        else:
            out[k] = torch.where(use, b, a)
    out["actions"] = out["actions"][:max(1, int(out["length"].max())) if n else 1].contiguous()
    out["side"] = use.to(torch.uint8)
    return out


def random_state_scramble(tables, chain, n, seed, device="cuda", **kw):
    """n random-state scrambles, the way a competition scrambler makes them: n cubes drawn uniformly from the group (cg_random, seed),
    solved by two_phase_solve (kw: its keywords), the answers inverted.  Returns dict(cubies: the drawn cubes' tiled cubie tensor,
    actions uint8 [L, n]: played from solved they give exactly those cubes, length int32 [n])."""
    from .vec_env import VecCubeEnv
    env = VecCubeEnv(n, device=device, cube_size=3, obs=None)
    env.reset_uniform(seed)
    res = two_phase_solve(tables, chain, env, **kw)
    return dict(cubies=env.cubies(), actions=invert_actions(res["actions"]), length=res["length"])
