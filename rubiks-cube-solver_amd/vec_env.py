"""VecCubeEnv: N independent cubes resident in HBM, stepped by one HIP launch.

The batched counterpart of the reference's CubeEnv (gym-cube/gym_cube/envs/cube_env.py:12-111):
same action order, reward (+1.0 solved / -1.0 otherwise), done flag and one-hot state
convention, for millions of cubes at once.  All cube arithmetic runs in librubikhip.so; this
class only owns tensors and forwards pointers.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from .tables import ACTION_NAMES, get_env_config


def legacy_scramble_actions(seeds, scramble_count, action_dim):
    """The reference's reset() draw for each seed: np.random.seed(s); randint(A, size=k), with the
    caller's global legacy RNG state saved and restored (cube_env.py:62-68).  -> uint8 [len(seeds), k]."""
    saved = np.random.get_state()
    try:
        out = np.empty((len(seeds), scramble_count), np.uint8)
        for i, s in enumerate(seeds):
            np.random.seed(int(s))
            out[i] = np.random.randint(action_dim, size=scramble_count)
    finally:
        np.random.set_state(saved)
    return out


class VecCubeEnv:
    """num_envs cubes on one GPU.

    obs: "onehot" -> step/reset return the dense one-hot [N, R, C] (`onehot_dtype`), the layout
         model.py:31-45 consumes;  "code" -> the compact uint8 code buffer [tiles, SLOTS, pitch]
         (lossless, 20 B per cube instead of 1920);  None -> no observation is produced.
    seed / stream_id: device RNG stream for reset() without explicit seeds (stream_id = rank in
         multi-GPU jobs gives every rank an independent stream, no communication).
    auto_reset: a cube whose episode ended -- solved (terminated), or `max_episode_steps` > 0 steps without being solved
         (truncated) -- starts a new episode within the same step(): a fresh scramble of `scramble_count` moves (an int k >= 0, or
         (lo, hi): the depth is drawn per episode), see step().  `scramble_count` is required then.  Off (the default) nothing
         changes: no further tensors, the same single launch per step.
    """

    def __init__(self, num_envs, device="cuda", cube_size=3, obs="onehot", onehot_dtype=torch.float32,
                 seed=0, stream_id=0, debug_check_every=0, auto_reset=False, max_episode_steps=0, scramble_count=None):
        self.auto_reset = bool(auto_reset)
        self._reset_depth = None
        if self.auto_reset:
            if scramble_count is None:
                raise ValueError("auto_reset=True needs scramble_count (an int or (lo, hi)): the depth of the fresh scrambles")
            self._reset_depth = ops.depth_range(scramble_count)
        elif scramble_count is not None or max_episode_steps:
            raise ValueError("scramble_count / max_episode_steps belong to auto_reset=True")
        self.max_episode_steps = int(max_episode_steps)
        if self.max_episode_steps < 0:
            raise ValueError("max_episode_steps must be >= 0 (0 = no time limit)")
        self.state_dim, self.action_dim = get_env_config(cube_size)
        self.cube_size = cube_size
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.RubikHipError("VecCubeEnv runs on a HIP device only (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if obs not in ("onehot", "code", None):
            raise ValueError("obs must be 'onehot', 'code' or None")
        self.obs = obs
        self.action_names = list(ACTION_NAMES[cube_size])
        self.seed, self.stream_id = int(seed), int(stream_id)
        self._resets = 0
        self._steps, self.debug_check_every = 0, int(debug_check_every)
        n, dev = self.num_envs, self.device
        self.stickers = ops.alloc_states(n, cube_size, dev)
        self.reward = torch.empty(n, dtype=torch.float32, device=dev)
        self.done = torch.empty(n, dtype=torch.uint8, device=dev)
        self._fmt = _lib.FMT_NONE
        self._obs_buf = None
        if obs == "onehot":
            self._fmt = _lib.fmt_of(onehot_dtype)
            self._obs_buf = torch.empty((n, *self.state_dim), dtype=onehot_dtype, device=dev)
        elif obs == "code":
            self._fmt = _lib.FMT_CODE
            self._obs_buf = ops.alloc_code(n, cube_size, dev)
        if self.auto_reset:
            # steps taken in the running episode, episodes started by auto-reset so far (it numbers the walks), and the two outputs
            self.elapsed = torch.zeros(n, dtype=torch.int32, device=dev)
            self.episode = torch.zeros(n, dtype=torch.int32, device=dev)
            self.ended = torch.zeros(n, dtype=torch.uint8, device=dev)
            self.episode_length = torch.zeros(n, dtype=torch.int32, device=dev)
        self._sym_buf = self._sym_bad = None         # apply_symmetry's scratch state buffer and bad-index flag, made on first use
        self.init_state()

    # ------------------------------------------------------------------ reference surface
    def init_state(self):
        """All cubes solved (cube_env.py:33-42)."""
        ops.fill_solved(self.stickers, self.num_envs, self.cube_size)
        self._new_episodes()
        return self._observe()

    def reset(self, seeds=None, scramble_count=2, actions=None):
        """Solved, then `scramble_count` random face turns per cube (cube_env.py:50-69).

        seeds   : one int per env -> each env i gets exactly the reference's reset(seed=seeds[i],
                  scramble_count[i]) move sequence; numpy's legacy generator runs on the device;
        actions : explicit uint8 [N, K] moves (overrides seeds); the value `action_dim` is a no-op,
                  so rows may be padded to a common length;
        neither : moves drawn on the device from (seed, stream_id, reset counter) -- reproducible,
                  rank-independent streams, no host work.
        scramble_count may be one int or (with seeds) one int per env.
        Returns the observation of the scrambled cubes."""
        n = self.num_envs
        counts = np.broadcast_to(np.asarray(scramble_count, dtype=np.int64), (n,)) if np.ndim(scramble_count) else None
        kmax = int(counts.max()) if counts is not None else int(scramble_count)
        if kmax <= 0 or (counts is not None and int(counts.min()) <= 0):
            # the reference returns an unbound `state` here (UnboundLocalError, cube_env.py:69)
            raise UnboundLocalError("reset(scramble_count=0): the reference has no state to return")
        ops.fill_solved(self.stickers, n, self.cube_size)
        self._new_episodes()
        if actions is None and seeds is not None:
            if len(seeds) != n:
                raise ValueError("need one seed per env")
            # the reference's np.random.seed(s); randint(A, size=k) per env, generated on the device
            # (rc_legacy_scramble_actions): bit-exact and independent of the host's global RNG state
            s_t = seeds if isinstance(seeds, torch.Tensor) else torch.as_tensor(np.asarray(seeds, dtype=np.int64))
            buf, kk = ops.legacy_scramble_actions(s_t, self.cube_size,
                                                  kmax if counts is None else counts.tolist(), device=self.device)
            ops.scramble(self.stickers, n, self.cube_size, kk, actions_in=buf, done=self.done, reward=self.reward)
            return self._observe()
        elif counts is not None:
            raise ValueError("per-env scramble counts need seeds (or pad explicit actions with the no-op)")
        if actions is not None:
            a = torch.as_tensor(actions, dtype=torch.uint8)
            if a.dim() != 2 or a.shape[0] != n:
                raise ValueError(f"actions must be [{n}, K]")
            if int(a.max()) > self.action_dim:
                raise IndexError("action out of range")  # cube_env.py:86,96
            k = a.shape[1]
            buf = torch.full((k, _lib.pitch_for(n)), self.action_dim, dtype=torch.uint8)
            buf[:, :n] = a.t()
            ops.scramble(self.stickers, n, self.cube_size, k, actions_in=buf.to(self.device),
                         done=self.done, reward=self.reward)
        else:
            self._resets += 1
            ops.scramble(self.stickers, n, self.cube_size, kmax, seed=self.seed, stream_id=self.stream_id,
                         walk_offset=self._resets * n, done=self.done, reward=self.reward)
        return self._observe()

    def step(self, actions, active=None):
        """One face turn per cube.  actions: uint8 tensor [N] on the env's device (anything else is
        converted and range-checked).  active: optional bool tensor [N]; cubes where it is False get
        the no-op (they keep their state; used by batched rollouts to park solved cubes).
        Returns (obs, reward float32 [N] of +-1.0, done uint8 [N], {}) -- cube_env.py:71-111.

        The three returned tensors are the env's OWN buffers, overwritten by the next step / reset: clone what
        must outlive it.  A uint8 device tensor is not range-checked on the host (that would synchronise): an
        action > action_dim leaves that cube unspecified and raises IndexError at the next check_actions()
        (`debug_check_every=K` in the constructor runs that check every K steps).

        auto_reset=True: three launches -- the move in place (reward, done), rcx_episode_end (include/rubikepisode.h), the
        observation.  Returns (obs of the states AFTER any reset, reward and done of the step taken, {"ended": uint8 [N]: 0 | 1
        terminated | 2 truncated, "episode_length": int32 [N]: the steps of the episode that ended, else 0}).  A cube that ended
        already holds the first state of its next episode; the TERMINAL observation of a truncated episode is not returned (for a
        terminated one it is the solved cube).  Fresh scrambles draw from `seed`, stream `stream_id + 2**32` -- never a stream
        reset() uses -- walk `episode * num_envs + i`, where `episode` counts the auto-resets of cube i; reset() and init_state()
        start new episodes (elapsed = 0) and leave that count running.  `active` contradicts auto-reset: ValueError.  Everything
        stays on the device, so a step can be captured as a hipGraph and replayed; the counters advance on replay."""
        if self.auto_reset and active is not None:
            raise ValueError("step(active=...) parks cubes; an auto_reset env restarts them instead")
        a = self._actions(actions)
        self._steps += 1
        if self.debug_check_every and self._steps % self.debug_check_every == 0:
            self.check_actions()
        if active is not None:
            a = torch.where(active.to(self.device), a, torch.full_like(a, self.action_dim))
        if self.auto_reset:
            n, lo_hi = self.num_envs, self._reset_depth
            ops.apply_moves(self.stickers, self.stickers, a, n, self.cube_size, self.reward, self.done, None, _lib.FMT_NONE)
            ops.episode_end(self.stickers, n, self.cube_size, self.done, self.elapsed, self.episode, self.ended, self.episode_length,
                            max_steps=self.max_episode_steps, depth=lo_hi, seed=self.seed, stream_id=self.stream_id + 2 ** 32,
                            walk_offset=0, walk_stride=n)
            return self._observe(), self.reward, self.done, {"ended": self.ended, "episode_length": self.episode_length}
        ops.apply_moves(self.stickers, self.stickers, a, self.num_envs, self.cube_size, self.reward, self.done,
                        self._obs_buf, self._fmt)
        return self._obs_buf, self.reward, self.done, {}

    def is_solved(self):
        ops.is_solved(self.stickers, self.num_envs, self.cube_size, self.done, self.reward)
        return self.done

    def sim_state_to_state(self, stickers=None, out=None, dtype=None):
        """Dense one-hot of the given (default: current) sticker buffer (cube_env.py:132-152)."""
        st = self.stickers if stickers is None else stickers
        if out is None:
            out = torch.empty((self.num_envs, *self.state_dim), dtype=dtype or torch.float32, device=self.device)
        ops.encode(st, self.num_envs, self.cube_size, out, _lib.fmt_of(out.dtype))
        return out

    # ------------------------------------------------------------------------- batched extras
    @property
    def sim_cube(self):
        """[N, S] uint8 tensor: one row per cube (a copy; the live buffer is `stickers`)."""
        return ops.to_aos(self.stickers, self.num_envs).contiguous()

    def set_sim_cube(self, states, check=False):
        """Load [N, S] sticker rows (host or device).  check=True: refuse states that are no cube reachable from solved (legality());
        ValueError names the first offending cube, its status bits and how many cubes failed, and the env keeps its old cubes.
        check=False (the default) loads any uint8 array, as before."""
        t = torch.as_tensor(states, dtype=torch.uint8).cpu()
        if check and tuple(t.shape) != (self.num_envs, self.stickers.shape[1]):
            raise ValueError(f"states must be [{self.num_envs}, {self.stickers.shape[1]}], got {tuple(t.shape)}")
        buf = ops.from_aos(t, self.device, self.stickers.shape[2])
        if check:
            status = ops.cubies(buf, self.num_envs, self.cube_size, cubies=False)["status"].cpu().numpy()
            failed = np.flatnonzero(status)
            if len(failed):
                from .tables import rcc_status_names
                first = int(failed[0])
                raise ValueError(f"set_sim_cube: cube {first} is not reachable from the solved cube (status {int(status[first])}: "
                                 f"{' | '.join(rcc_status_names(int(status[first])))}); {len(failed)} of {self.num_envs} cubes failed")
        self.stickers.copy_(buf)

    def cubies(self, index=False):
        """The cubes as pieces (ops.cubies; the rule: include/rubikhip.h "Cubie coordinates"): the cubie tensor uint8 [tiles, SLOTS,
        pitch] -- ops.to_aos(t, N) gives [N, SLOTS] --, or with index=True (cubies, corner_index int32 [N][, edge_index int64 [N] on
        the 3x3x3]); an index is all-ones (-1) where the cube is not legal."""
        out = ops.cubies(self.stickers, self.num_envs, self.cube_size, status=False, index=bool(index))
        if not index:
            return out["cubies"]
        return (out["cubies"], out["corner_index"]) + ((out["edge_index"],) if self.cube_size == 3 else ())

    def legality(self):
        """uint8 [N]: 0 where the cube can be reached from solved by the env's moves, else the RCC_* bits that say why not."""
        return ops.cubies(self.stickers, self.num_envs, self.cube_size, cubies=False)["status"]

    def corner_distance(self, table):
        """uint8 [N]: the exact distance of every cube's CORNER state from a pattern.CornerTable (one rcp_lookup launch) -- the optimal
        solution length on the 2x2x2, an admissible lower bound with the right parity on the 3x3x3; 0xFF for illegal corners."""
        return table.distance(self)

    def edge_distance(self, table):
        """uint8 [N]: the exact distance of every cube's tracked EDGE pieces from a pattern.EdgeTable (3x3x3; one encode and one
        rce_lookup launch), an admissible lower bound on the cube's; a pattern.MaxTable gives the maximum over its members."""
        return table.distance(self)

    def chain_solve(self, tables, graph=False):
        """search.chain_solve(tables, self): every cube solved through a pattern.ChainTables (3x3x3 only); the env is left as it is."""
        from .search import chain_solve
        return chain_solve(tables, self, graph=graph)

    def ida_search(self, table, **kwargs):
        """search.ida_search(table, self, ...): the optimal solution of every cube by IDA* under a CornerTable, an EdgeTable, a MaxTable
        or None (3x3x3 only); the env is left as it is."""
        from .search import ida_search
        return ida_search(table, self, **kwargs)

    def two_phase_solve(self, tables, chain, **kwargs):
        """search.two_phase_solve(tables, chain, self, ...): a short solution of every cube by Kociemba's two phases under a
        pattern.TwoPhaseTables, never longer than chain_solve's through the pattern.ChainTables `chain` (3x3x3 only); the env is left
        as it is."""
        from .search import two_phase_solve
        return two_phase_solve(tables, chain, self, **kwargs)

    def from_cubies(self, cubies):
        """Set every cube from its cubie bytes: [N, SLOTS] rows (host or device) or a tiled cubie tensor as cubies() returns it.  The
        assembly need not be legal (legality() tells); a byte that names no (piece, orientation) raises ValueError and the env keeps
        its old cubes.  Starts new episodes like reset(); returns the observation."""
        n, SL = self.num_envs, ops.N_SLOTS[self.cube_size]
        c = cubies if isinstance(cubies, torch.Tensor) else torch.as_tensor(np.asarray(cubies), dtype=torch.uint8)
        if c.dim() == 2 and tuple(c.shape) == (n, SL):
            c = ops.from_aos(c.cpu(), self.device, self.stickers.shape[2])
        elif not (c.dim() == 3 and c.shape[1] == SL and c.dtype == torch.uint8):
            raise ValueError(f"cubies must be [{n}, {SL}] rows or a tiled uint8 tensor [tiles, {SL}, pitch]")
        self.stickers.copy_(ops.from_cubies(c.to(self.device), n, self.cube_size, out=torch.empty_like(self.stickers)))
        self._new_episodes()
        return self._observe()

    def _set_cubies(self, cub, bad, what):
        """The tail of compose / invert / reset_uniform: the flag raised with the env untouched, else the stickers of the cubie rows."""
        if bad is not None and int(bad):
            raise ValueError(f"{what}: a cube's cubie rows name no (piece, orientation), or are no permutation of the pieces")
        self.stickers.copy_(ops.from_cubies(cub, self.num_envs, self.cube_size, out=torch.empty_like(self.stickers)))
        self._new_episodes()
        return self._observe()

    def compose(self, other):
        """Cube i becomes x_i o y_i, "this cube, then other's" (include/rubikhip.h "Cube group"): the cube reached from x_i by any move
        sequence that takes solved to y_i.  other: a VecCubeEnv of the same size and device, or a tiled cubie tensor as cubies()
        returns it.  Assemblies need not be legal; a byte that names no (piece, orientation) raises ValueError and the env keeps its
        cubes.  Starts new episodes like from_cubies(); returns the observation."""
        n, SL = self.num_envs, ops.N_SLOTS[self.cube_size]
        if isinstance(other, VecCubeEnv):
            if (other.num_envs, other.cube_size, other.device) != (n, self.cube_size, self.device):
                raise ValueError("compose: the other env must have the same num_envs, cube_size and device")
            y = other.cubies()
        elif isinstance(other, torch.Tensor) and other.dim() == 3 and other.shape[1] == SL and other.dtype == torch.uint8:
            y = other.to(self.device)
        else:
            raise ValueError(f"compose: other must be a VecCubeEnv or a tiled uint8 cubie tensor [tiles, {SL}, pitch]")
        bad = torch.zeros(1, dtype=torch.uint8, device=self.device)
        x = self.cubies()
        return self._set_cubies(ops.group_product(x, y, n, self.cube_size, out=x, bad=bad), bad, "compose")

    def invert(self):
        """Every cube becomes its inverse: the cube whose solutions are this cube's scrambles.  A sticker state whose slots are no
        permutation of the pieces raises ValueError and the env keeps its cubes.  Starts new episodes; returns the observation."""
        bad = torch.zeros(1, dtype=torch.uint8, device=self.device)
        x = self.cubies()
        return self._set_cubies(ops.group_inverse(x, self.num_envs, self.cube_size, out=x, bad=bad), bad, "invert")

    def reset_uniform(self, seed, stream_id=0, first=0):
        """Every cube drawn uniformly from the group (cg_random): cube i is a function of (seed, stream_id, first + i) alone.  Starts new
        episodes like reset(); returns the observation."""
        cub = ops.random_cubies(self.num_envs, self.cube_size, self.device, seed=seed, stream_id=stream_id, first=first,
                                out_pitch=self.stickers.shape[2])
        return self._set_cubies(cub, None, "reset_uniform")

    def expand(self, children=False, codes=True, pitch=None):
        """All A children of every cube (cube_env.py:212-236, mcts.py:96-101).
        Returns dict(child_solved [A, Wp], child_code [A, tiles, SLOTS, pitch], children [A, tiles, S, pitch]);
        ops.to_aos(buf[a], n) turns one child's tiled buffer into [n, rows]."""
        n, cs = self.num_envs, self.cube_size
        _, pitch = ops._tile_shape(n, pitch)
        out = ops.expand_buffers(n, cs, self.device, pitch, children=children, codes=codes)
        ops.expand_children(self.stickers, n, cs, out.get("children"), out["child_solved"], out.get("child_code"), pitch=pitch)
        return out

    def check_actions(self):
        """Raise IndexError if any kernel since the last check saw an out-of-range action, or apply_symmetry an out-of-range
        symmetry index (synchronises)."""
        if _lib.read_status(self.device) & _lib.STATUS_BAD_ACTION:
            raise IndexError("action out of range")  # cube_env.py:86,96
        if self._sym_bad is not None and int(self._sym_bad):
            self._sym_bad.zero_()
            raise IndexError("symmetry index out of range")

    def apply_symmetry(self, sym):
        """Every cube becomes its image under a whole-cube symmetry (tables.get_symmetries; include/rubiksym.h).  sym: an int (one
        symmetry for all cubes) or a uint8 tensor [N] on the env's device (one per cube).  The image is written into a scratch
        buffer the env keeps, which then becomes `stickers` (the old buffer is the next scratch: `stickers` is REBOUND, hold no
        reference to it across this call).  The observation is refreshed and returned; reward, done and the episode counters are
        untouched (a symmetry keeps solved cubes solved and every distance).  A following step(amap[s][a]) gives the image of
        step(a).  An int out of range raises IndexError at once; an index tensor is not checked on the host: an entry >= K leaves that
        cube as it is and raises IndexError at the next check_actions()."""
        if isinstance(sym, torch.Tensor):
            if sym.dtype != torch.uint8 or sym.device != self.device or sym.numel() != self.num_envs:
                raise ValueError(f"sym must be an int or a uint8 tensor [{self.num_envs}] on {self.device}")
            sym = sym.contiguous().reshape(-1)
            if sym.data_ptr() % 16:
                sym = sym.clone()
            if self._sym_bad is None:
                self._sym_bad = torch.zeros(1, dtype=torch.uint8, device=self.device)
        if self._sym_buf is None:
            self._sym_buf = torch.empty_like(self.stickers)
        ops.apply_symmetry(self.stickers, self.num_envs, None, self.cube_size, sym, out=self._sym_buf, bad=self._sym_bad)
        self.stickers, self._sym_buf = self._sym_buf, self.stickers
        return self._observe()

    def canonical(self):
        """uint8 [N]: per cube the lowest symmetry index whose image is the lexicographically smallest of the K images (the
        canonical form up to symmetry, rcs_sym_canonical).  The cubes stay as they are; apply_symmetry(env.canonical()) makes
        every cube its canonical image."""
        return ops.canonical_symmetry(self.stickers, self.num_envs, None, self.cube_size)

    def clone(self, lean=False):
        """Independent copy of the cubes.  lean: copy only the sticker buffer (the state); reward / done / observation
        are outputs of the next step and get fresh uninitialised buffers -- one copy kernel instead of four (the batch-1
        facade, which mcts.py:37 deep-copies once per simulation, keeps its observation on the host)."""
        other = object.__new__(VecCubeEnv)
        other.__dict__.update(self.__dict__)
        other.stickers = self.stickers.clone()
        other._sym_buf = other._sym_bad = None
        for k in ("reward", "done", "_obs_buf"):
            v = getattr(self, k)
            setattr(other, k, None if v is None else (torch.empty_like(v) if lean else v.clone()))
        if self.auto_reset:
            other.elapsed, other.episode = self.elapsed.clone(), self.episode.clone()         # state, like the stickers
            other.ended, other.episode_length = (torch.empty_like(v) if lean else v.clone() for v in (self.ended, self.episode_length))
        return other

    __copy__ = clone

    def __deepcopy__(self, memo):
        return self.clone()

    # ------------------------------------------------------------------------------- helpers
    def _actions(self, actions):
        a = actions
        if isinstance(a, torch.Tensor) and a.numel() != self.num_envs:
            raise ValueError(f"need {self.num_envs} actions")
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.uint8 and a.device == self.device):
            a = torch.as_tensor(np.asarray(actions) if not isinstance(actions, torch.Tensor) else actions)
            if a.numel() != self.num_envs:
                raise ValueError(f"need {self.num_envs} actions")
            if a.numel() and (int(a.max()) >= self.action_dim or int(a.min()) < 0):
                raise IndexError("action out of range")
            a = a.to(device=self.device, dtype=torch.uint8)
        return a.contiguous().reshape(-1)

    def _new_episodes(self):
        """reset() / init_state(): every cube starts an episode; the auto-reset count (the walk numbering) keeps running."""
        if self.auto_reset:
            self.elapsed.zero_()

    def _observe(self):
        if self._obs_buf is not None:
            ops.encode(self.stickers, self.num_envs, self.cube_size, self._obs_buf, self._fmt)
        return self._obs_buf
