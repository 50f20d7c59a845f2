/*
 * rubikhip.h -- C ABI of librubikhip.so: the MI355X (gfx950) cube-environment hot path.
 *
 * The reference (SUNGBEOMCHOI/Rubiks-Cube-Solver) has no FFI: its env path is Python
 * (SURVEY.md section 8b).  Each entry point below names the reference code it replaces,
 * paths relative to /root/reference.  A binding only needs plain pointers and sizes; see
 * INTEGRATION.md for the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - All buffers are DEVICE memory owned by the caller (e.g. PyTorch-ROCm tensors); the
 *     library allocates nothing but its constant tables and one status word per device (rc_apply_moves_ws takes a
 *     caller-owned workspace).
 *   - State layout.  Cube states are structure-of-arrays uint8, values 0..5, S = 54
 *     (cube_size 3) or 24 (cube_size 2) rows, in TILES of `pitch` cubes:
 *         sticker s of cube n lives at st[(n / pitch) * S * pitch + s * pitch + n % pitch].
 *     One tile (pitch >= n_cubes, pitch % 16 == 0) is plain SoA, st[s * pitch + n].  Several
 *     tiles need a power-of-two pitch >= 512 (the widest wave span); 16384-32768 measured best on MI355X at 4M cubes
 *     (+12..24 % HBM throughput over one 4M-wide tile: every wave's 54 row segments then sit
 *     within 54 * pitch bytes).  RC_FMT_CODE buffers are tiled the same way with SLOTS rows.
 *     Buffers described as "plain" below are one tile.
 *   - Alignment.  Every device pointer that a kernel reads or writes in packs must be 16-byte aligned, and 16 bytes is all it
 *     needs (a buffer carved 16 bytes into a larger allocation is fine): state / code / family buffers, children, child_code,
 *     child_solved, dense one-hots, workspaces, the uint8 per-cube arrays `actions`, `actions_in`, `actions_out` and `done` (one
 *     4- or 8-byte pack per lane) and `reward` (float4 stores).  A pointer that breaks the rule is RC_EINVAL before anything is
 *     launched; the message names the operand.  Arrays that are only indexed element by element need the NATURAL alignment of
 *     their element type and nothing more: rc_legacy_scramble_actions seeds / counts, rc_adi_targets* child_value / child_solved /
 *     parent_value / weight / target_value / target_policy / error, and every operand of rc_search_pack (bytes).  The facade's
 *     `st` is read one sticker per lane (natural); its host_out has its own 512-byte contract.
 *   - actions are uint8 in the env's action order U,U',F,F',R,R'[,D,D',B,B',L,L']
 *     (gym-cube/gym_cube/envs/cube_env.py:24-28); A = 12 | 6.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     stream-ordered, never synchronise (except rc_read_status, rc_facade_step(wait=1) and
 *     rc_get_tables), are re-entrant, and keep no mutable state besides the per-device status word
 *     (one word per DEVICE, shared by all streams).
 *   - Row offsets inside one tile are 32-bit scalar offsets of buffer instructions: rows * pitch
 *     must stay below 2^32 (a single tile of more than ~79 M 3x3x3 cubes has to be split into tiles).
 *   - Return value: RC_OK or a negative RC_E* code; rc_last_error() gives the message of
 *     the calling thread's last failure.  Nothing is thrown across the ABI.
 *   - The action value A itself (12 | 6) is a NO-OP: the cube is left unchanged (its done /
 *     reward / one-hot are still written).  Batched rollouts use it to park finished cubes and to
 *     pad scrambles of different lengths.  The reference has no such action.
 *   - Out-of-range actions (> A) are the reference's IndexError (cube_env.py:86,96).  On the
 *     device they cannot raise: the cube is left in an unspecified (in-bounds) state and
 *     bit RC_STATUS_BAD_ACTION of the status word is set; rc_read_status() reports it.
 *
 * One-hot formats (`fmt`)
 *   RC_FMT_NONE   nothing written
 *   RC_FMT_CODE   compact, lossless: uint8 code[slot * pitch + n] (tiled like states), slot = 0..19 | 0..6,
 *                 code = piece*3+ori (corner slots) or piece*2+ori (edge slots)
 *                 (getOP_3, assets/py333.py:224-227).  3x3x3: one-hot column of row `slot`
 *                 (pos_to_state_3, py333.py:235-246).  2x2x2: row = code/3,
 *                 column = slot*3 + code%3 (cube_env.py:142-147).
 *   RC_FMT_U8 / RC_FMT_F16 / RC_FMT_BF16 / RC_FMT_F32
 *                 dense [n][R][C] (R,C = 20,24 | 7,21), contiguous per cube, values {0,1}:
 *                 exactly what model.py:31-45 consumes after `.float()`.
 */
#ifndef RUBIKHIP_H
#define RUBIKHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RC_OK 0
#define RC_EINVAL (-1)    /* bad argument (null, alignment, cube_size, fmt, sizes) */
#define RC_EHIP (-2)      /* a HIP runtime call failed */
#define RC_ENODEV (-3)    /* rc_init not called / no gfx950 device */

#define RC_FMT_NONE 0
#define RC_FMT_CODE 1
#define RC_FMT_U8 2
#define RC_FMT_F16 3
#define RC_FMT_F32 4
#define RC_FMT_BF16 5

#define RC_STATUS_BAD_ACTION 1u

/* Library / ABI version (major*100 + minor). */
int rc_version(void);

/* Identity of the sources this binary was built from: the first 16 hex digits of a sha256 over rubikhip.hip, rc_device.h,
 * rc_tables.h and this header (rubiks-cube-solver_amd/_build.py), passed as -DRC_SRC_HASH at build time; "unhashed" for a build
 * that was not given one.  The Python binding compares it with the tree's sources and refuses a stale library.  Static storage.
 * (Tooling; no reference counterpart.) */
const char *rc_build_id(void);

/* Check that `device` is a gfx950 GPU, make the code object resident there and clear its status
 * word.  Idempotent; the caller's current device is not changed (kernels run on the device of the
 * stream / current device the caller set, one process per GPU).  Replaces: importing py333 (module-level table construction,
 * gym-cube/gym_cube/envs/assets/py333.py:41-198). */
int rc_init(int device);

/* Host copies of the tables the kernels use (any pointer may be NULL).
 *   perm        [A][S]   new[i] = old[perm[a][i]]            (py333.py:46-138 moveDefs)
 *   solved      [S]                                           (py333.py:211-218)
 *   corner_defs [NC][3], edge_defs [NE][2]                    (py333.py:140-164)
 *   corner_code [72], edge_code [72]  hash -> piece*3+ori / piece*2+ori, 0 where the
 *                reference table has no entry or ends        (py333.py:171-198)
 * dims, if non-NULL, receives {S, A, NC, NE, R, C}. */
int rc_get_tables(int cube_size, uint8_t *perm, uint8_t *solved, uint8_t *corner_defs,
                  uint8_t *edge_defs, uint8_t *corner_code, uint8_t *edge_code, int32_t dims[6]);

/* st[s][n] = s / face_size for n < n_cubes.  Replaces initState_3 (py333.py:211-218) /
 * CubeEnv.init_state (cube_env.py:33-42). */
int rc_fill_solved(uint8_t *st, int64_t n_cubes, int64_t pitch, int cube_size, void *stream);

/* One env step for n_cubes independent cubes: out = in moved by actions[n], then
 * done[n] = solved, reward[n] = done ? +1.0f : -1.0f, and the one-hot of the NEW state.
 * `out` may alias `in` (in-place); reward, done, onehot may be NULL (onehot NULL requires
 * fmt RC_FMT_NONE).  code_pitch is the row pitch of an RC_FMT_CODE buffer (ignored for
 * dense formats).  RC_EINVAL: a NULL or not 16-byte aligned in / out / actions, a reward, done or onehot that is not 16-byte
 * aligned, a bad pitch, fmt or cube_size, onehot and fmt that disagree.  Replaces CubeEnv.step (cube_env.py:71-111) = doMove_3 (py333.py:220-222)
 * + sim_state_to_state (cube_env.py:132-152) + isSolved_3 (py333.py:229-233). */
int rc_apply_moves(const uint8_t *in, uint8_t *out, const uint8_t *actions, int64_t n_cubes,
                   int64_t pitch_in, int64_t pitch_out, int cube_size, float *reward,
                   uint8_t *done, void *onehot, int fmt, int64_t code_pitch, void *stream);
/* rc_apply_moves with a caller-owned WORKSPACE (device memory, 16-byte aligned, rc_workspace_bytes(RC_OP_STEP, ...) bytes; its
 * contents are scratch; it must not overlap in, out, actions, reward, done or onehot: RC_EINVAL).  Results are identical to rc_apply_moves.  With a dense `fmt` on large 3x3x3 batches the workspace lets the
 * call run as two launches -- step + reward + done + compact code into the workspace, then the front writer
 * (k_code_to_dense_front) -- so that the dense stream leaves the chip as one sweeping window: 0.80-0.94 of the HBM peak on every
 * allocation instead of 0.67-0.87 depending on where the buffer lives (DESIGN.md "Dense one-hot").  A NULL or too small workspace,
 * or a call that has no use for one (rc_workspace_bytes() == 0), runs exactly rc_apply_moves.  The library still allocates nothing. */
int64_t rc_workspace_bytes(int op, int cube_size, int64_t n_cubes, int fmt);
int rc_apply_moves_ws(const uint8_t *in, uint8_t *out, const uint8_t *actions, int64_t n_cubes,
                      int64_t pitch_in, int64_t pitch_out, int cube_size, float *reward, uint8_t *done,
                      void *onehot, int fmt, int64_t code_pitch, void *workspace, int64_t workspace_bytes, void *stream);
/* rc_encode with a caller-owned workspace (the same rc_workspace_bytes(RC_OP_STEP, ...) bytes): a dense one-hot of a large 3x3x3
 * batch is then encoded into the workspace as compact codes and expanded by the front writer.  Results identical to rc_encode. */
int rc_encode_ws(const uint8_t *st, int64_t n_cubes, int64_t pitch, int cube_size, void *onehot, int fmt, int64_t code_pitch,
                 void *workspace, int64_t workspace_bytes, void *stream);
/* Same with a per-call tuning override (see "Tuning override" at the end; 0 = rc_apply_moves). */
int rc_apply_moves_ex(const uint8_t *in, uint8_t *out, const uint8_t *actions, int64_t n_cubes,
                      int64_t pitch_in, int64_t pitch_out, int cube_size, float *reward,
                      uint8_t *done, void *onehot, int fmt, int64_t code_pitch, void *stream, int variant);

/* CubeEnv.step for ONE cube with the lowest host latency (cube_env.py:71-111; the batch-1 facade):
 * st is a device state buffer whose cube 0 is stepped in place (sticker s at st[s * pitch]); the action
 * travels by value; the kernel writes into `host_out`, 512 bytes of HOST-MAPPED pinned memory
 * (hipHostMalloc / torch pin_memory): [0, R*C) the dense uint8 one-hot of the new state, [496] done,
 * [504..507] `seq` (non-zero, written last after a system-scope fence).  The kernel writes through the buffer's DEVICE alias
 * (hipPointerGetAttributes), the host polls the host address, so hipHostRegister'ed memory works too.  wait != 0: returns once `seq`
 * is visible in host_out (spin on the flag; no stream synchronisation, no copies); wait == 0: returns
 * after the launch and the caller polls host_out itself.  Out-of-range actions set RC_STATUS_BAD_ACTION. */
int rc_facade_step(uint8_t *st, int64_t pitch, int cube_size, int action, uint8_t *host_out,
                   uint32_t seq, int wait, void *stream);
/* Same for a SEQUENCE of moves (`actions`: n_actions bytes in HOST memory, copied into the launch arguments; n_actions
 * may be 0 = just report the current state): one launch per 60 moves instead of one per move; host_out describes the
 * final state.  This is a whole tree descent of MCTS.traverse (mcts.py:52-81, one env.step per level there). */
int rc_facade_steps(uint8_t *st, int64_t pitch, int cube_size, const uint8_t *actions, int n_actions,
                    uint8_t *host_out, uint32_t seq, int wait, void *stream);

/* Node expansion of a single-root tree search for ONE cube (cube 0 of st; MCTS.expand, mcts.py:83-113: the
 * reference does 12 env.step + 13 deepcopy(env) per leaf; also the child loop of get_target_value,
 * cube_env.py:212-236).  One launch, results in `host_out` (host-mapped pinned memory, as above; 512 bytes,
 * or 512 + A*R*C = 6272 with dense != 0): [0, SLOTS) the cube's own compact code (RC_FMT_CODE bytes: the node
 * key), [32 + a * SLOTS, ...) the code of child a, [288 + a] solved flag of child a, [504..507] `seq`,
 * and with dense != 0 [512 + a * R*C, ...) the dense uint8 one-hot of child a. */
int rc_facade_expand(const uint8_t *st, int64_t pitch, int cube_size, uint8_t *host_out, uint32_t seq,
                     int dense, int wait, void *stream);

/* The facade entry points cache the device alias of every host_out they validated, process-wide, keyed on (host address, current
 * device); a call with seq == 1 (a caller's first use of a buffer) always validates afresh.  Call this before freeing a host_out
 * buffer, from ANY thread (NULL drops everything cached); CubeEnv.close() / garbage collection does. */
int rc_facade_release(const uint8_t *host_out);

/* Device address of HOST-MAPPED pinned memory (hipHostMalloc / hipHostRegister / torch pin_memory), for callers that let a kernel
 * read a small input straight from host memory instead of uploading it first: e.g. the action paths of a lockstep tree search, written
 * by the host trees and replayed by rc_scramble(actions_in = the alias) -- one H2D copy less per simulation.  RC_EINVAL for other memory. */
int rc_host_alias(const void *host, void **device_alias);

/* `depth` moves applied in place to every cube: the scramble loop of CubeEnv.reset
 * (cube_env.py:65-67) for n_cubes cubes at once.  actions_in[d * act_pitch + n] replays given
 * moves (e.g. the host's legacy-numpy draws, for bit-exact reset(seed)); NULL draws them on
 * the device exactly like rc_adi_generate (walk = walk_offset + n).  actions_out (same layout,
 * NULL to skip) receives the moves used.  done/reward (NULL to skip) describe the final state.
 * RC_EINVAL: a NULL or not 16-byte aligned st (src), an actions_in, actions_out, done or reward that is not 16-byte aligned, a bad
 * pitch / act_pitch / cube_size, negative n_cubes or depth. */
int rc_scramble(uint8_t *st, int64_t n_cubes, int64_t pitch, int cube_size, int depth, uint64_t seed,
                uint64_t stream_id, int64_t walk_offset, const uint8_t *actions_in, uint8_t *actions_out,
                int64_t act_pitch, uint8_t *done, float *reward, void *stream);

/* rc_scramble that reads the start states from `src` (same layout and pitch as st) and leaves them untouched: st = src moved.  The
 * lockstep tree search replays every simulation's descents from its root states this way (mcts.py:37,80: one deepcopy + one env.step
 * per tree level there).  depth == 0 copies. */
int rc_scramble_from(const uint8_t *src, uint8_t *st, int64_t n_cubes, int64_t pitch, int cube_size, int depth,
                     uint64_t seed, uint64_t stream_id, int64_t walk_offset, const uint8_t *actions_in,
                     uint8_t *actions_out, int64_t act_pitch, uint8_t *done, float *reward, void *stream);

/* One record per root for the host trees of a lockstep search (include/rubiktree.h rc_tree_update; mcts.py:96-101 keeps the same three
 * things per expanded node): from the leaves' codes (RC_FMT_CODE layout, [tile][SLOTS][pitch]) and the outputs of rc_expand_children
 * with pitch_out = pitch (child_code [A][tiles][SLOTS][pitch], child_solved [A][tiles * pitch]) to
 * leaf_out [n][SLOTS], child_out [n][A][SLOTS], solved_out [n][A], contiguous. */
int rc_search_pack(const uint8_t *leaf_code, const uint8_t *child_code, const uint8_t *child_solved, int64_t n_cubes,
                   int64_t pitch, int cube_size, uint8_t *leaf_out, uint8_t *child_out, uint8_t *solved_out, void *stream);

/* The scramble draws of CubeEnv.reset(seed, k) (cube_env.py:62-68) for n envs at once, bit for bit:
 * np.random.seed(seeds[i]); np.random.randint(action_dim, size=k_i) of numpy's LEGACY generator
 * (MT19937 + masked rejection) runs on the device, one env per lane.  k_i = counts[i] (device memory;
 * values outside 0..kmax are clamped to that range) or count_uniform when counts is NULL.  actions_out[d * pitch + i] for d < k_i, the no-op value A
 * for k_i <= d < kmax: ready to be replayed by rc_scramble(actions_in).  pitch >= n, pitch % 16 == 0. */
int rc_legacy_scramble_actions(const uint32_t *seeds, const int32_t *counts, int count_uniform, int kmax,
                               int64_t n_envs, int cube_size, uint8_t *actions_out, int64_t pitch,
                               void *stream);
/* Same with the generator form chosen by the caller (RC_VARIANT_LEGACY_*; 0 = rc_legacy_scramble_actions).  Two forms produce the
 * same bytes: the LDS form keeps MT19937's 624-word state per env in LDS (any count; the twist is done lazily, 64 words at a time);
 * the STREAMING form computes outputs 0..622 of the first generation from a few init_genrand chain iterators in registers (no state at
 * all) and is followed by a fix-up launch of the LDS form for the waves in which a lane needed more -- the default up to kmax = 400. */
int rc_legacy_scramble_actions_ex(const uint32_t *seeds, const int32_t *counts, int count_uniform, int kmax,
                                  int64_t n_envs, int cube_size, uint8_t *actions_out, int64_t pitch,
                                  void *stream, int variant);

/* done / reward of the given states, no move (at least one of them; each 16-byte aligned, else RC_EINVAL).  Replaces isSolved_3
 * (py333.py:229-233). */
int rc_is_solved(const uint8_t *st, int64_t n_cubes, int64_t pitch, int cube_size,
                 uint8_t *done, float *reward, void *stream);

/* One-hot of the given states, no move.  Replaces sim_state_to_state (cube_env.py:132-152)
 * = pos_to_state_3(getOP_3(s)) (py333.py:224-246). */
int rc_encode(const uint8_t *st, int64_t n_cubes, int64_t pitch, int cube_size, void *onehot,
              int fmt, int64_t code_pitch, void *stream);

/* Dense one-hot [n][R][C] from a compact code buffer (RC_FMT_CODE layout). fmt = U8/F16/BF16/F32. */
int rc_onehot_from_code(const uint8_t *code, int64_t n_cubes, int64_t code_pitch, int cube_size,
                        void *onehot, int fmt, void *stream);
int rc_onehot_from_code_ex(const uint8_t *code, int64_t n_cubes, int64_t code_pitch, int cube_size,
                           void *onehot, int fmt, void *stream, int variant);
/* The same for n_blocks EQUALLY TILED code buffers in one launch: block b is read at code + b * src_block_stride bytes (n_cubes cubes,
 * tiling code_pitch) and written at onehot + b * dst_block_stride cubes (dst_block_stride >= n_cubes; every block 16-byte aligned).
 * What the 2x2x2 ADI pipeline needs: the A child-code buffers of each depth ([depth][A][tile][SLOTS][pitch] of rc_adi_generate) become
 * the packed [depth * A][dst_block_stride] input of ONE forward of the value net (cube_env.py:239-251 evaluates 12 + 1 rows at a time)
 * instead of blocks padded to whole tiles (the 3x3x3 pipeline uses rc_onehot_from_family_depths). */
int rc_onehot_from_code_blocks(const uint8_t *code, int64_t n_cubes, int64_t code_pitch, int cube_size, void *onehot, int fmt,
                               int n_blocks, int64_t src_block_stride, int64_t dst_block_stride, void *stream);

/* All A children of every cube.  Outputs use one tiling (pitch_out, tiles = ceil(n / pitch_out)
 * when n > pitch_out, else 1), child-major:
 *   children     [A][tiles][S][pitch_out]        child a = a tiled state buffer of its own
 *   child_code   [A][tiles][SLOTS][pitch_out]
 *   child_solved [A][tiles * pitch_out]          flag of child a of cube n at [a][n]
 * (any may be NULL).  With one tile this is children[(a*S + s) * pitch_out + n].  `in` may be tiled too.
 * Replaces the child loops of CubeEnv.get_target_value (cube_env.py:212-236) and MCTS.expand (mcts.py:96-101). */
int rc_expand_children(const uint8_t *in, int64_t n_cubes, int64_t pitch_in, int cube_size,
                       uint8_t *children, uint8_t *child_solved, uint8_t *child_code,
                       int64_t pitch_out, void *stream);
int rc_expand_children_ex(const uint8_t *in, int64_t n_cubes, int64_t pitch_in, int cube_size,
                          uint8_t *children, uint8_t *child_solved, uint8_t *child_code,
                          int64_t pitch_out, void *stream, int variant);

/* ADI scramble generator: n_walks random walks of `depth` moves from the solved cube, each
 * step expanded to all A children.  Replaces the env work of CubeEnv.get_random_samples
 * (cube_env.py:177-194) + get_target_value's child loop (cube_env.py:212-236).
 *   actions_in   NULL: moves are drawn on the device, walk w (global index walk_offset + w)
 *                uses xoroshiro128+ seeded by splitmix64 from (seed, stream_id, walk)
 *                (DESIGN.md "RNG"); non-NULL: replay actions_in[d * pitch + w].
 * Layouts, with tiles = ceil(n_walks / pitch) when n_walks > pitch (then pitch is a power of two
 * >= 512), else 1, and Wp = tiles * pitch (any pointer may be NULL to skip that output):
 *   actions_in / actions_out  [depth][Wp]
 *   parents      [depth][tiles][S][pitch]          one tiled state buffer per depth
 *   parent_code  [depth][tiles][SLOTS][pitch]
 *   children     [depth][A][tiles][S][pitch]       one tiled state buffer per (depth, child)
 *   child_code   [depth][A][tiles][SLOTS][pitch]
 *   child_solved [depth][A][Wp]
 * With one tile these are the plain [depth][A][S][pitch] arrays. */
int rc_adi_generate(uint64_t seed, uint64_t stream_id, int64_t walk_offset, int64_t n_walks,
                    int depth, int cube_size, int64_t pitch, const uint8_t *actions_in,
                    uint8_t *actions_out, uint8_t *parents, uint8_t *parent_code,
                    uint8_t *children, uint8_t *child_code, uint8_t *child_solved, void *stream);
int rc_adi_generate_ex(uint64_t seed, uint64_t stream_id, int64_t walk_offset, int64_t n_walks,
                       int depth, int cube_size, int64_t pitch, const uint8_t *actions_in,
                       uint8_t *actions_out, uint8_t *parents, uint8_t *parent_code,
                       uint8_t *children, uint8_t *child_code, uint8_t *child_solved, void *stream,
                       int variant);

/* ADI target assembly for `n` parents with A children each.
 * Replaces cube_env.py:229-232,239-251:
 *   if any child is solved: target_value = 1.0, target_policy = lowest solved index;
 *   else target_value = max_a(child_value[a] + (-1.0f)), target_policy = first arg max;
 *   error = |double(parent_value) - double(target_value)| * weight[n]   (weight = d**-T, host).
 * child_value[a * pitch + n] (float), child_solved[a * pitch + n], parent_value[n]. */
/* The same walks with the FAMILY record instead of parent / child codes (3x3x3 and 2x2x2): a face turn carries whole cubies, so every
 * slot code of a parent and of its A children is one of NF shared look-ups -- 51 for the 3x3x3 (31 corner + 20 edge (slot, reading
 * order) pairs), 15 for the 2x2x2.  family[((d * tiles + tile) * NF + row) * pitch + walk] holds them (tiled like the codes, NF rows):
 * 51 bytes per (walk, depth) instead of 13 x 20.  rc_family_layout gives NF and rows[(A + 1)][SLOTS]: the family row that IS slot p's
 * code of child a (a = A: the parent) -- the pick of cube_env.py:212-236 / py333.py:224-227 as a table.  rc_onehot_from_family
 * (3x3x3) expands one depth's rows ([tile][NF][pitch], n walks) to the dense one-hots of all A children and the parent in one
 * launch: child a at onehot + a * block_stride cubes, the parent as block A (block_stride >= n). */
int rc_adi_generate_family(uint64_t seed, uint64_t stream_id, int64_t walk_offset, int64_t n_walks,
                           int depth, int cube_size, int64_t pitch, const uint8_t *actions_in,
                           uint8_t *actions_out, uint8_t *parents, uint8_t *family, uint8_t *child_solved,
                           void *stream, int variant);
int rc_family_layout(int cube_size, uint8_t *rows, int32_t *n_rows);
int rc_onehot_from_family(const uint8_t *family, int64_t n_cubes, int64_t pitch, int cube_size, void *onehot,
                          int fmt, int64_t block_stride, void *stream);
/* The same for n_depths CONSECUTIVE depths of one rc_adi_generate_family call in one launch: `family` points at the first depth's
 * record ([n_depths][tile][NF][pitch]); depth g, block a (child a; a = A: the parent) goes to onehot + (g * (A + 1) + a) * block_stride
 * cubes -- the [depth][A + 1][block_stride] input of ONE forward of the value net (cube_env.py:239-251 evaluates it 2 x per sample). */
int rc_onehot_from_family_depths(const uint8_t *family, int64_t n_cubes, int64_t pitch, int cube_size, void *onehot,
                                 int fmt, int64_t block_stride, int n_depths, void *stream);

/* ADI targets of one depth (cube_env.py:229-232,239-251).  child_value / child_solved [A][pitch], walk w < n:
 *   a solved child exists  target_value = 1.0f, target_policy = the lowest solved index (whatever the values are, NaN included);
 *   otherwise              torch.max(child_value + (-1.0f)) over the A children, with torch.max's order: the FIRST maximal index
 *                          (-0 == +0, so a tie of zeros keeps the lower index; the first +inf wins), and NaN propagates -- if any
 *                          child value is NaN the target is NaN and target_policy is the index of the FIRST NaN;
 *   error (optional)       fabs((double)parent_value[w] - (double)target_value) * weight[w], NaN when either side is. */
int rc_adi_targets(const float *child_value, const uint8_t *child_solved, const float *parent_value,
                   const double *weight, int64_t n, int64_t pitch, int cube_size,
                   float *target_value, int32_t *target_policy, double *error, void *stream);
/* The same rule for n_depths depths at once, reading the value net's output in place and writing WALK-MAJOR results (the layout of
 * the replay sink, utils.py:253-260 one record per (cube, depth)):
 *   child_value[g * cv_depth_stride + a * cv_child_stride + w], parent_value[g * pv_depth_stride + w]  (floats; strides in elements),
 *   child_solved[(g * A + a) * solved_pitch + w]  (the [depth][A][Wp] flags of rc_adi_generate*),  weight[g] = (g0 + g + 1) ** -T,
 *   target_value / target_policy / error [w * out_stride + g]   for w < n, g < n_depths  (out_stride >= n_depths). */
int rc_adi_targets_depths(const float *child_value, int64_t cv_depth_stride, int64_t cv_child_stride,
                          const uint8_t *child_solved, int64_t solved_pitch, const float *parent_value,
                          int64_t pv_depth_stride, const double *weight, int64_t n, int n_depths, int cube_size,
                          float *target_value, int32_t *target_policy, double *error, int64_t out_stride, void *stream);

/* Read-and-clear the device status word: ONE atomic exchange on the device, ordered after the work queued
 * on `stream` (which it synchronises).  The word is per device, not per stream: a bit set by a kernel
 * that is still running on another stream is not lost -- it shows up in a later read. */
int rc_read_status(uint32_t *status, void *stream);

/* Which kernel instantiation and launch geometry a call WOULD use, as text (e.g. "k_step<Cube3,V=2,move,store,POL=1>
 * grid=8192 block=64"), decided by the same host functions the launchers call: benchmarks label their records with it.
 *   op       RC_OP_STEP (rc_apply_moves / rc_is_solved / rc_encode), RC_OP_EXPAND, RC_OP_ADI, RC_OP_CODE_TO_DENSE, RC_OP_FAMILY_TO_DENSE
 *   n        cubes / parents / walks;  depth: RC_OP_ADI only
 *   outputs  RC_OUT_* bits: STATES = the out buffer of a step (move + store) or the children stickers, CODE = compact codes,
 *            FLAGS = child_solved, REWARD / DONE = the step's reward / done arrays, INPLACE = out aliases in (step)
 *   fmt      the one-hot format of a step / code-to-dense call;  variant: the tuning override (0 = defaults)
 * Nothing is launched; no reference counterpart (tooling).  `variant` must only use the RC_VARIANT_* fields of `op`'s group. */
#define RC_OP_STEP 1
#define RC_OP_EXPAND 2
#define RC_OP_ADI 3
#define RC_OP_CODE_TO_DENSE 4
#define RC_OP_FAMILY_TO_DENSE 5 /* rc_onehot_from_family_depths: n = walks, depth = depths per launch, fmt = the dense format; variant must be 0 */
#define RC_OUT_STATES 1u
#define RC_OUT_CODE 2u
#define RC_OUT_FLAGS 4u
#define RC_OUT_REWARD 8u
#define RC_OUT_INPLACE 16u
#define RC_OUT_DONE 32u
#define RC_OUT_FAMILY 128u     /* RC_OP_ADI: the family record instead of codes (rc_adi_generate_family) */
#define RC_OUT_WORKSPACE 64u   /* RC_OP_STEP with a dense fmt: what rc_apply_moves_ws launches when given its workspace */
int rc_describe_dispatch(int op, int cube_size, int64_t n, int depth, unsigned outputs, int fmt, int variant,
                         char *buf, int buflen);

/* Message of the calling thread's last failed call ("" if none). */
const char *rc_last_error(void);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Tuning override (`variant`) of the *_ex entry points and of rc_describe_dispatch.  TOOLING: benchmarks and tests that must reach
 * every kernel instantiation; there is NO process-global knob and a binding of the reference needs none of this (INTEGRATION.md lists
 * the twelve entry points it does need).  Everything named *_ex, rc_describe_dispatch, rc_family_layout and rc_workspace_bytes is
 * tooling in that sense.  0 = the measured defaults.  A value is the SUM of macros of ONE group below; an entry point rejects
 * (RC_EINVAL) any decimal field its group does not define, so a value built for one entry point never means something else in another.
 *
 * rc_apply_moves_ex / RC_OP_STEP */
#define RC_VARIANT_STEP_PACK(v) (v)                   /* 1, 2: 4, 8 cubes per lane */
#define RC_VARIANT_STEP_POLICY(p) ((p) * 10)          /* row traffic: 1 stream in / stream out, 2 default-cached, 3 stream in / keep the
                                                         output in the Infinity Cache, 4 state default-cached / side outputs streamed */
#define RC_VARIANT_STEP_DENSE_TILE(t) ((t) * 100000)  /* fused dense writer: 1 -> 64-cube tiles, 2 -> 256-cube tiles; any non-zero value
                                                         also makes rc_apply_moves_ws ignore its workspace */
/* rc_expand_children_ex / RC_OP_EXPAND */
#define RC_VARIANT_EXPAND_PACK(v) (v)                 /* 1, 2 */
#define RC_VARIANT_EXPAND_STREAM(h) ((h) * 100)       /* streaming form (few persistent waves): 1..7 -> 128, 192, 256, 384, 512, 768, 1024
                                                         waves, 8 -> never */
#define RC_VARIANT_EXPAND_PARTS(p) ((p) * 1000)       /* 1..A parts per walk group (rounded up to a divisor of A) */
/* rc_adi_generate_ex, rc_adi_generate_family / RC_OP_ADI */
#define RC_VARIANT_ADI_PACK(v) (v)                    /* 1, 2 */
#define RC_VARIANT_ADI_PARTS(p) ((p) * 1000)          /* 1..A */
#define RC_VARIANT_ADI_SEGS(s) ((s) * 1000000)        /* 1..16 depth segments per walk group (clamped to the depth) */
/* rc_onehot_from_code_ex / RC_OP_CODE_TO_DENSE */
#define RC_VARIANT_DENSE_FORM(f) ((f) * 100000)       /* 1 -> 64-cube tiles, 2 -> 256-cube tiles, 3 -> the wide form (960-thread workgroups
                                                         sweeping contiguous tile ranges; superseded, kept for A/B), 4 -> the front form (one
                                                         3840-byte pass per workgroup; the default from 2^15 / 2^16 / 2^18 cubes, f32 / 16-bit / u8) */
#define RC_VARIANT_DENSE_WIDE_GROUPS16(g) ((g) * 1000) /* form 3: wanted workgroups / 16 (1..99) */
#define RC_VARIANT_DENSE_WIDE_SKEW(k) ((k) * 10)      /* form 3: sweep skew 1..9 */
#define RC_VARIANT_DENSE_FRONTS(f) (f)                /* form 4 / default front: 1, 2, 4 fronts per XCD per workgroup */
#define RC_VARIANT_DENSE_FRONT_FETCH(t) ((t) * 10)    /* form 4 / default front: 2 = one linear front, 3 = code bytes by a gather per lane,
                                                         4 = by one load of wave 0 + LDS */
/* rc_legacy_scramble_actions_ex (not decimal: mode + 16 * limit) */
#define RC_VARIANT_LEGACY_LDS 1                       /* the LDS form alone */
#define RC_VARIANT_LEGACY_STREAM(limit) (2 + 16 * (limit)) /* the streaming form with `limit` outputs per lane (1..623; 0 = 623) + fix-up */

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Cubie coordinates (prefix rcc_): the cube as pieces.  No reference counterpart: the reference's only piece-level view is getOP_3
 * (py333.py:224-227 = RC_FMT_CODE), whose corner table is incomplete and not injective; the bytes below are exact for ANY colouring.
 *
 * THE RULE.  Slots and pieces are numbered as rc_get_tables' corner_defs / edge_defs: piece q is the cubie that sits in slot q of the
 * solved cube.  One byte per slot, SLOTS = 20 | 7 rows, corner slots first, tiled like an RC_FMT_CODE buffer:
 *   edge     piece * 2 + ori   -- DEFINED as RC_FMT_CODE's edge byte: ori = 0 when the piece's first colour (edge_defs order of its home
 *                              slot) shows on the slot's first sticker;
 *   corner   piece * 3 + ori   -- ori = the number of clockwise steps, seen from outside the cube looking at that corner, from the slot's
 *                              U/D-face sticker to the sticker that shows the piece's U/D colour.  The handedness of every slot comes from
 *                              the cube's geometry (rcc_tables corner_cw), not from the listing order of corner_defs, which mixes
 *                              handedness.  This is deliberately NOT RC_FMT_CODE's corner byte;
 *   0xFF     the slot's colours are no cubie: two equal or opposite colours, a mirror-image corner, a value above 5.
 * status, one byte per cube, is 0 exactly when the state can be reached from the solved cube by the env's moves: */
#define RCC_BAD_COLOUR 1u  /* a sticker value is above 5 */
#define RCC_BAD_FIXED 2u   /* a sticker the moves never touch differs from solved: the 6 centres | the 3 stickers of the 2x2x2's DLB cubie */
#define RCC_BAD_PIECE 4u   /* some slot reads 0xFF */
#define RCC_DUP_PIECE 8u   /* a piece occurs twice (among the slots that name one) */
#define RCC_TWIST 16u      /* the sum of the corner ori is not 0 mod 3 */
#define RCC_FLIP 32u       /* the sum of the edge ori is odd (3x3x3 only) */
#define RCC_PARITY 64u     /* corner-permutation parity != edge-permutation parity, both relative to solved (3x3x3 only) */
/* Bits 16..64 are evaluated only when bits 1..8 are clear, and are 0 otherwise.
 * Indices, NC = 8 | 7:
 *   corner_index = lehmer(corner pieces) * 3^(NC-1) + sum_{q < NC-1} ori[q] * 3^q,  lehmer = sum_q #{r > q : piece[r] < piece[q]} * (NC-1-q)!
 *                  (below 88 179 840 | 3 674 160);
 *   edge_index   = lehmer(edge pieces) * 2^11 + sum_{q < 11} ori[q] * 2^q  (below 479 001 600 * 2048; 3x3x3 only);
 * both all-ones when status != 0.  On the 2x2x2, corner_index alone is a bijection from the group onto 0 .. 3 674 159.
 *
 * Conventions as above: caller-owned device memory, stream-ordered, nothing allocated; RC_EINVAL before any launch (rc_last_error names
 * the operand); pad columns and every byte outside the rows keep their bytes; n_cubes == 0 succeeds without a launch; every pointer
 * needs 16-byte alignment and no more.
 *
 * rcc_cubies: one launch, whichever outputs are asked for.  cubies [tiles][SLOTS][cubie_pitch], status [n_cubes], corner_index
 * [n_cubes], edge_index [n_cubes]: each may be NULL, not all four; edge_index must be NULL for cube_size 2. */
int rcc_cubies(const uint8_t *st, int64_t n_cubes, int64_t pitch, int cube_size, uint8_t *cubies, int64_t cubie_pitch,
               uint8_t *status, uint32_t *corner_index, uint64_t *edge_index, void *stream);
/* The inverse: all S stickers of cubes < n_cubes from their cubie rows; centres and the DLB stickers come out solved.  It does NOT
 * require a legal assembly: a twisted corner or a repeated piece is written as given.  A byte that names no (piece, ori) -- a corner
 * byte >= 3 * NC, an edge byte >= 24 -- cannot raise on the device: that cube is written as solved and *bad (one device byte the
 * caller zeroes and reads, required) is set to 1, the idea of RC_STATUS_BAD_ACTION. */
int rcc_from_cubies(const uint8_t *cubies, int64_t n_cubes, int64_t cubie_pitch, int cube_size, uint8_t *st, int64_t pitch,
                    uint8_t *bad, void *stream);
/* Host copies of the rule's tables, no device (any pointer may be NULL): corner_cw [NC][3] the stickers of each corner slot clockwise
 * seen from outside, the U/D sticker first; edge_facelets [NE][2] = edge_defs; corner_colours [NC][3] / edge_colours [NE][2] the colours
 * of piece p in the order of corner_cw[p] / edge_facelets[p]. */
int rcc_tables(int cube_size, uint8_t *corner_cw, uint8_t *edge_facelets, uint8_t *corner_colours, uint8_t *edge_colours);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Edge pattern databases (prefix rce_): exact distance tables over the places and flips of up to 7 of the 12 edge pieces, Korf's
 * companion of the corner table (include/rubiksearch.h rcp_*).  3x3x3 ONLY: the 2x2x2 has no edges, and no entry point takes a
 * cube_size.  No reference counterpart.
 *
 * THE RULE.
 *   tracked set   `mask`: bit t set = edge PIECE t (numbered as edge_defs) is tracked; k set bits, 1 <= k <= 7, t_0 < ... < t_{k-1}.
 *   pattern       for each t_i the slot p_i in 0..11 it sits in and its ori bit o_i = the low bit of that slot's edge byte
 *                 (piece * 2 + ori, the rcc_* / RC_FMT_CODE edge byte).
 *   index         d_i = p_i - #{j < i : p_j < p_i} (in [0, 12 - i));  perm = sum_i d_i * prod_{j = i+1}^{k-1} (12 - j);
 *                 index = perm * 2^k + sum_i o_i * 2^i, below N(k) = 12!/(12-k)! * 2^k = 24, 528, 10 560, 190 080, 3 041 280,
 *                 42 577 920, 510 935 040 (all below 2^32).
 *   home          p_i = t_i, o_i = 0: rce_home_index(mask), NOT 0 in general.
 *   move a        2 * esrc[a][q] + eflip[a][q] is the edge byte of slot q after move a on the solved cube (rce_tables): a piece in slot s
 *                 goes to the q with esrc[a][q] == s and its ori bit is XORed with eflip[a][q].
 *   table         table[i] = the least number of quarter turns that bring pattern i home; nothing stays 0xFF.  An admissible and
 *                 consistent bound on the cube's distance.  Unlike the corner table's, its parity is NOT the distance's.
 *   illegal       a row set with an edge byte >= 24, a tracked piece absent or a tracked piece twice: h = 0xFF (score -255) and NO table
 *                 read.  Untracked slots are not looked at beyond the range check.  Every table address passes one guard
 *                 (idx < N ? table[idx] : 0xFF); the host checks bytes >= N(k).
 *
 * Conventions as in the rcc_* section: caller-owned device memory, stream-ordered, nothing allocated; RC_EINVAL before any launch
 * (rc_last_error names the operand) for a mask that is 0, has a bit above 11 or more than 7 bits, a table smaller than N(k), a NULL
 * or misaligned pointer, a negative size; pad columns and every byte outside the rows keep their bytes; n == 0 succeeds without a
 * launch; every pointer needs 16-byte alignment and no more.
 *
 * Host only, no device: N(k) and the home index of `mask` (-1 for a bad mask); the library's move tables esrc, eflip [12][12]. */
int64_t rce_table_bytes(int mask);
int64_t rce_home_index(int mask);
int rce_tables(uint8_t *esrc, uint8_t *eflip);
/* Breadth-first build, one launch per level.  rce_build_begin: every entry 0xFF, home 0 (one fill kernel).  rce_build_level: an entry
 * still 0xFF becomes depth + 1 iff one of its 12 neighbours holds `depth`; *count (one device uint32, 16-byte aligned, zeroed by the
 * call) receives how many were set.  Each lane writes its own entry only: the table after a level does not depend on scheduling.  The
 * table is complete when a level sets nothing.  depth in 0..253. */
int rce_build_begin(uint8_t *table, int64_t bytes, int mask, void *stream);
int rce_build_level(uint8_t *table, int64_t bytes, int mask, int depth, uint32_t *count, void *stream);
/* indices [n] (uint32) -> the 20 cubie rows (rcc_* layout, [tiles][20][cubie_pitch]) of a REACHABLE cube with that pattern: corners
 * home; the tracked pieces as the index says; the untracked pieces fill the free slots, both in ascending order, with ori 0; if the
 * flip sum is odd the edge in the highest free slot is flipped; then, if the edge permutation is odd, the edges of the two highest
 * free slots trade places.  An index >= N(k) is written as the solved cube and sets *bad (one device byte the caller zeroes and
 * reads, required). */
int rce_unrank(const uint32_t *indices, int64_t n, int mask, uint8_t *cubies, int64_t cubie_pitch, uint8_t *bad, void *stream);
/* out[c] = table[index of cube c], 0xFF for an illegal row set.  rows: a tiled [tiles][20][pitch] buffer in RC_FMT_CODE or rcc_cubies
 * layout (their edge rows are the same bytes); only rows 8..19 are read. */
int rce_lookup(const uint8_t *rows, int64_t n, int64_t pitch, int mask, const uint8_t *table, int64_t bytes, uint8_t *out, void *stream);
/* The same over rc_search_expand's candidate code buffer (include/rubiksearch.h: child-major [A * tiles][20][pitch], tiles =
 * ceil(n_problems * width / pitch), pitch a power of two >= 512), EVERY slot j < A * tiles * pitch, also those past `live` whose bytes
 * are arbitrary: combine 0: scores[j] = -(float)h;  combine 1: scores[j] = -(float)h where that is LESS than what scores[j] holds
 * (a tie, -0 against +0 included, and a NaN keep what is there).  One launch per table forms the maximum of several tables; -255,
 * the illegal score, wins over everything. */
int rce_score_codes(const uint8_t *code, int64_t n_problems, int width, int64_t pitch, int mask, const uint8_t *table, int64_t bytes,
                    float *scores, int combine, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Subgroup chain (prefix rct_): Thistlethwaite's chain <all> > <U,D,R,L,F2,B2> > <U,D,F2,R2,B2,L2> > <half turns> > {solved} as four
 * exact coset-distance tables and a descent that goes downhill in each: a solution of ANY legal cube without a search and without a
 * net, at most 47 generators = 87 quarter turns long.  3x3x3 ONLY: no entry point takes a cube_size.  No reference counterpart.
 *
 * THE RULE.  Cubie bytes as in the rcc_* section: corner slots 0..7 hold piece cp[q] with ori co[q], edge slots 0..11 hold ep[q] with
 * eo[q]; lehmer as defined there; a subset's rank is the lexicographic rank of its sorted slot tuple.
 *   stage 0   domain: every cube.  index = sum_{q<11} eo[q] * 2^q, N = 2048, goal 0.  Generators, in this order: the 12 actions 0..11.
 *   stage 1   domain: all 12 eo = 0.  index = sum_{q<7} co[q] * 3^q + 2187 * C, C = the rank among the 495 4-subsets of {0..11} of the
 *             slots that hold pieces 8..11; N = 1 082 565; goal: twist 0, C = 494.  Generators: U, U', F2, R, R', D, D', B2, L, L'.
 *   stage 2   domain: stage 1's goal set (all eo and co 0, pieces 8..11 in slots 8..11).  index = lehmer(cp) + 40320 * E, E = the rank
 *             among the 70 4-subsets of {0..7} of the slots that hold pieces {0, 2, 4, 6}; N = 2 822 400; goals: the 96 entries
 *             (h, E_home), h in H = the corner permutations half turns reach (rct_corner_cosets), E_home = 20 = the rank of (0, 2, 4, 6).
 *             Generators: U, U', F2, R2, D, D', B2, L2.
 *   stage 3   domain: stage 2's goal set.  index = ((r * 24 + m) * 24 + s) * 24 + e: r = the rank of lehmer(cp) in sorted H, m = the
 *             lehmer of (ep[0], ep[2], ep[4], ep[6]) / 2, s = that of ((ep[1], ep[3], ep[5], ep[7]) - 1) / 2, e = that of ep[8..11] - 8;
 *             N = 1 327 104; goal: the solved cube, index 0.  Generators: U2, F2, R2, D2, B2, L2.  The 663 552 entries whose corner
 *             and edge permutations differ in parity belong to no cube and stay 0xFF.
 *   table     table[i] = the least number of the stage's generators (a half turn counts one) that bring coset i to a goal.
 *   descent   at distance d > 0 take the FIRST generator of the stage's order whose child reads d - 1, emit its one or two quarter-turn
 *             actions (a half turn is the clockwise action twice), repeat until 0.  At most 16 generators are taken per call.
 *   guard     every table address passes one guard (idx < N ? table[idx] : 0xFF); the host checks bytes >= N.
 * status, one byte per cube of rct_descend (0: fine; a cube with a nonzero status is not moved, but for RCT_STUCK): */
#define RCT_ILLEGAL 1u   /* a byte names no cubie (>= 24), or a piece occurs twice */
#define RCT_OUTSIDE 2u   /* the cube is not in the stage's domain, or its entry is 0xFF */
#define RCT_NO_ROOM 4u   /* length < 0 or length + 2 * d > max_length: the cube is not walked */
#define RCT_STUCK 8u     /* no child is one closer, or the walk is not home after 16 generators: the table is not this stage's.  The
                            walk stops where it is; what it took so far is written */
/* Conventions as in the rce_* section: caller-owned device memory, stream-ordered, nothing allocated, nothing synchronises; RC_EINVAL
 * before any launch (rc_last_error names the operand) for a stage outside 0..3, a table smaller than N, a NULL or misaligned pointer,
 * a negative size; pad columns and every byte outside the rows keep their bytes; n == 0 succeeds without a launch; every pointer
 * needs 16-byte alignment and no more.
 *
 * Host only, no device: N of a stage (-1 for a bad stage); its generators, gens [12][2] = the one or two actions of each (0xFF: none,
 * also in the rows from *count on); sorted H, h [96].  Any pointer may be NULL. */
int64_t rct_table_bytes(int stage);
int rct_generators(int stage, uint8_t *gens, int *count);
int rct_corner_cosets(uint16_t *h);
/* Breadth-first build, one launch per level, as rce_build_*.  rct_build_begin: every entry 0xFF, the goals 0 (one fill kernel).
 * rct_build_level: an entry still 0xFF becomes depth + 1 iff one of its neighbours under the stage's generators holds `depth` (the
 * generator sets are closed under inversion); *count (one device uint32, 16-byte aligned, zeroed by the call) receives how many were
 * set.  Each lane writes its own entry only.  The table is complete when a level sets nothing.  depth in 0..253. */
int rct_build_begin(uint8_t *table, int64_t bytes, int stage, void *stream);
int rct_build_level(uint8_t *table, int64_t bytes, int stage, int depth, uint32_t *count, void *stream);
/* index[c] (uint32) = the stage's index of the cubie rows ([tiles][20][cubie_pitch], rcc_* layout) of cube c; 0xFFFFFFFF for an
 * illegal row set (RCT_ILLEGAL's rule) and for a cube outside the stage's domain.  The twist, flip and parity sums are NOT looked at:
 * that is rcc_cubies' status. */
int rct_index(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, int stage, uint32_t *index, void *stream);
/* indices [n] (uint32) -> the 20 cubie rows of a REACHABLE cube of the stage's domain with that index.  What the index leaves free:
 *   stage 0   every piece home, co 0, eo[11] closes the flip sum;
 *   stage 1   corners home, co[7] closes the twist, eo 0; pieces 8..11 fill the subset's slots and pieces 0..7 the other slots, both
 *             ascending; then, if the edge permutation is odd, the edges of the two highest slots outside the subset trade places;
 *   stage 2   co, eo 0; pieces 0, 2, 4, 6 fill the subset's slots and 1, 3, 5, 7 the other slots of 0..7, both ascending, 8..11 home;
 *             then, if the corner and edge permutations differ in parity, the edges of slots 10 and 11 trade places;
 *   stage 3   nothing.
 * An index >= N, and a stage-3 index whose permutations differ in parity, is written as the solved cube and sets *bad (one device
 * byte the caller zeroes and reads, required). */
int rct_unrank(const uint32_t *indices, int64_t n, int stage, uint8_t *cubies, int64_t cubie_pitch, uint8_t *bad, void *stream);
/* The walk of one stage, in place, one launch: cube c's rows are moved to the stage's goal set, its quarter turns are appended to
 * column c of actions [max_length][act_pitch] (uint8; act_pitch % 16 == 0, act_pitch >= n) from row length[c] on, and length[c]
 * (int32) advances; rows past the new length keep their bytes (the caller prefills the no-op 12).  moves[c] = the table value at
 * entry, 0xFF for an illegal cube or one outside the domain; status[c] as above.  max_length >= 1. */
int rct_descend(uint8_t *cubies, int64_t n, int64_t cubie_pitch, int stage, const uint8_t *table, int64_t bytes, uint8_t *actions,
                int max_length, int64_t act_pitch, int32_t *length, uint8_t *moves, uint8_t *status, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Iterative-deepening A* (prefix ida_): Korf's cost-bounded depth-first search under the pattern databases above -- the OPTIMAL
 * solution of a cube with no node memory: a cube's whole search is a trail of moves, a depth and a bound.  3x3x3 ONLY.  No reference
 * counterpart.  The prefix does not start with "rc": every export of this library that does belongs to one of the sections above,
 * whose lists are closed; a section of further names is the only kind they admit.
 *
 * THE RULE.
 *   state       the 20 cubie bytes of the rcc_* section.  Move a acts by the corner and edge move tables (rcp_tables, rce_tables); a ^ 1
 *               undoes a.  A cube is the goal iff all 20 bytes are the solved cube's.
 *   heuristic   h(x) = the maximum over the tables given: at most one corner table (index = corner_index, as rcp_*) and 0..4 edge
 *               tables, each with its mask (index as rce_*); h = 0 with no table.  Every table address passes the one guard of its
 *               section (idx < N ? table[idx] : 0xFF); the host checks bytes >= N.
 *   canonical   after a path ending ..., p2, p1 move m is skipped iff m == p1 ^ 1, or m == p1 and m is odd (a half turn is the even
 *               action twice), or m == p1 == p2, or (m >> 1) + 3 == (p1 >> 1) (faces f and f + 3 commute: U/D, F/B, R/L; the lower
 *               face goes first).  ida_canonical gives the mask.  12, 114, 1068, 10 011, 93 840, ... sequences of length 1, 2, ...
 *   iteration   at `bound`, depth-first from the start node, moves in the order 0..11.  Every generated child y at depth g + 1 counts
 *               one in nodes; f = g + 1 + h(y).  f > bound: next = min(next, f), the child is dropped.  Otherwise, y the goal: SOLVED,
 *               length = g + 1, the trail is the solution.  Otherwise descend into y.  The iteration exhausted: next > limit gives
 *               EXHAUSTED (next stays readable, a proven lower bound), otherwise bound = next, next = +inf = 2^31 - 1, and the search
 *               starts again from the start node.  First bound = floor + h(start); a first bound above the limit is EXHAUSTED with
 *               next = that bound.  A start node that is the goal: SOLVED, length = floor, nodes = 0.  The answer of a SOLVED cube is
 *               therefore unique: the first optimal solution in this order, with this count of nodes.
 *   limit       limit[c] counts as min(limit[c], max_depth): a trail never outgrows the rows of path.
 *   frame       caller-owned, per cube c; nothing lives in the library.
 *                 path    uint8 [max_depth][path_pitch], max_depth <= 32, path_pitch % 16 == 0, path_pitch >= n.  path[0..floor) is a
 *                         prefix the caller wrote; the start node is the root moved by it, the search never goes above it, and the
 *                         canonical rule looks at its last two moves.  A SOLVED cube's rows floor..length-1 receive the solution; no
 *                         other row is ever written (the caller prefills 12, the no-op).
 *                 floor   int32, may be NULL (= 0);  limit  int32.
 *                 trail   uint64 [n][2]: nibble i (of 32) = move i of the path from the root to the current node, prefix included.
 *                         The trail, not path, carries a running search from call to call: rows of path written at one budget's
 *                         cuts and not at another's would break the invariance below.
 *                 cursor  uint8: the least move not yet tried at the current node (0..12).
 *                 depth, bound, next  int32;  nodes  uint64;  status  uint8, 0 = running, else the bits below.
 *               The root cubies are an input and are never written: a call rebuilds the current node by replaying trail[0..depth).  A
 *               cube with a nonzero status is not touched again.  After SOLVED length = depth.
 *   budget      ida_search advances every running cube by at most max_steps passes.  A pass generates one child (dropped, entered or
 *               the goal), or goes back one level (the inverse of the last move is applied; at the start node: the iteration ends as
 *               above).  The kernel's only loop is bounded by max_steps; no loop's trip count depends on what a table holds.
 *   invariance  the frame after k passes in all depends on the inputs alone, not on how the calls cut the k.
 *   written     ida_search takes any frame with status 0, not only one ida_init or an earlier call left: a caller may store a frame and
 *               put it back, or write one.  It reads floor, trail[0..depth), cursor, depth, bound, next and nodes, never path.  A frame
 *               is refused with IDA_BAD_FRAME for floor outside 0..max_depth, depth < floor, depth > max_depth, cursor > 12,
 *               bound > min(limit, max_depth), or a trail nibble >= 12 below depth.  The bit is OR-ed into status; every other field of
 *               the frame and every row of path keep the bytes the caller wrote, and the cube is not counted in *running.  Nibbles from
 *               depth on are stale and never looked at.  depth > bound is NOT refused (a caller may lower or raise bound between
 *               calls): every child is dropped into next until the search is back below the bound. */
#define IDA_SOLVED 1u
#define IDA_EXHAUSTED 2u
#define IDA_ILLEGAL 4u     /* a cubie byte >= 24, a piece twice, or a table read 0xFF */
#define IDA_BAD_FRAME 8u   /* floor, depth or cursor out of range, bound above the limit, a prefix or trail move >= 12 */
/* Conventions as in the rct_* section: caller-owned device memory, stream-ordered, nothing allocated, nothing synchronises; RC_EINVAL
 * before any launch with nothing written (rc_last_error names the operand) for a NULL or misaligned pointer, a negative size, a table
 * smaller than its N, a bad mask, n_edge outside 0..4, max_depth outside 1..32, max_steps outside 1..ida_max_steps(); pad columns keep
 * their bytes; n == 0 succeeds without a launch; every pointer needs 16-byte alignment and no more.  corner_table may be NULL (no
 * corner table); masks, edge_tables (device pointers) and edge_bytes are HOST arrays of n_edge entries and travel to the kernel by value.
 *
 * Host only, no device: the largest max_steps ida_search takes (one launch at it stays near a second); allowed [13][13][12], the
 * canonical rule as the kernel was compiled with it: allowed[p2][p1][m] = 1 iff m may follow ..., p2, p1 (12 = no move); a NULL
 * pointer is RC_EINVAL. */
int64_t ida_max_steps(void);
int ida_canonical(uint8_t *allowed);
/* The frame's first contents: legality of the cubie rows (IDA_ILLEGAL), the prefix replayed (IDA_BAD_FRAME for floor outside
 * 0..max_depth or a prefix byte >= 12), the first bound, zeroed counters.  A cube with one of these two bits gets depth = bound = 0. */
int ida_init(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *corner_table, int64_t corner_bytes, int n_edge,
             const int *masks, const uint8_t *const *edge_tables, const int64_t *edge_bytes, uint8_t *path, int max_depth, int64_t path_pitch,
             const int32_t *floor, const int32_t *limit, uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next,
             uint64_t *nodes, uint8_t *status, void *stream);
/* At most max_steps passes per running cube; the frames are stored, and the cubes still running are added to *running (one device
 * uint32, 16-byte aligned, zeroed by the call). */
int ida_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *corner_table, int64_t corner_bytes, int n_edge,
               const int *masks, const uint8_t *const *edge_tables, const int64_t *edge_bytes, uint8_t *path, int max_depth, int64_t path_pitch,
               const int32_t *floor, const int32_t *limit, uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next,
               uint64_t *nodes, uint8_t *status, int64_t max_steps, uint32_t *running, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Two-phase (prefix tp_): Kociemba's two-phase algorithm -- a SHORT solution of any cube.  Phase 1 searches for ways into
 * G1 = <U,D,F2,R2,B2,L2> (the goal set of the chain's stage 1), phase 2 solves each G1 cube found, optimally within G1, under four
 * coset-distance tables of about 1 MB each.  3x3x3 ONLY.  No reference counterpart.  The prefix does not start with "rc" for the
 * reason given in the ida_* section.
 *
 * THE RULE.  Cubie bytes, cp/co/ep/eo, lehmer and subset ranks as in the rcc_* / rct_* sections; the move tables are rcp_tables /
 * rce_tables; the actions are 0..11 = U, U', F, F', R, R', D, D', B, B', L, L'.  All lengths are in quarter turns.
 *   generators  phase 1: the 12 actions, cost 1 each.  Phase 2, in this order (the chain's stage 2): U, U', F2, R2, D, D', B2, L2 with
 *               costs 1, 1, 2, 2, 1, 1, 2, 2; a half turn is the clockwise action twice.
 *   tables      table[i] = the least cost to the goal under the phase's generators, 0xFF = not reached.
 *                 0 twist-slice   index = sum_{q<7} co[q] * 3^q + 2187 * C, C = the rank among the 495 4-subsets of {0..11} of the slots
 *                                 that hold pieces 8..11; N = 1 082 565; domain: every cube; goal: twist 0, C = 494.
 *                 1 flip-slice    index = sum_{q<11} eo[q] * 2^q + 2048 * C; N = 1 013 760; every cube; goal: flip 0, C = 494.
 *                 2 corner-slice  index = lehmer(cp) * 24 + s, s = lehmer(ep[8..11] - 8); N = 967 680; domain G1 (all co and eo 0, pieces
 *                                 8..11 in slots 8..11); goal 0.
 *                 3 edge-slice    index = lehmer(ep[0..7]) * 24 + s; N = 967 680; domain G1; goal 0.
 *               Tables 0, 1 are phase 1's, tables 2, 3 phase 2's.  h = the maximum of the phase's two tables; a node is the phase's goal
 *               iff both read 0.  Every table address passes the one guard (idx < N ? table[idx] : 0xFF); the host checks bytes >= N.
 *   level       tp_build_level on tables 0, 1 is rct_build_level's rule.  On tables 2, 3 it is WEIGHTED: an entry still 0xFF becomes
 *               depth + 1 iff a neighbour under a generator of cost w holds depth + 1 - w.  Each lane writes its own entry only; a
 *               weighted table is complete when TWO levels in a row set nothing.
 *   canonical   ida_canonical's rule on the trail of ACTIONS; a phase-2 generator is allowed iff its first action is.
 *   search      the ida_* state machine: a pass generates one child or goes back one level; children in generator order;
 *               f = g + cost + h(child); f > bound: next = min(next, f), the child is dropped; an exhausted iteration moves bound to
 *               next (next = 2^31 - 1), or ends EXHAUSTED when next > the limit; a child whose h reads 0xFF ends ILLEGAL.  Frames are
 *               caller-owned; the only loop is bounded by max_steps; the frame after k passes depends on the inputs alone, not on how
 *               the calls cut the k.  A cube or column with a nonzero status is not touched again.
 *   phase 1     one lane per cube c < n, floor 0, first bound h(root), limit[c] counts as min(limit[c], max_depth, 32).  It collects up
 *               to K = candidates per cube: a goal child with f <= bound is never entered; it is EMITTED iff g + 1 == bound and its
 *               last action is not a U or D turn (0, 1, 6, 7).  Emission writes, for slot j = found[c], column j * stride + c
 *               (candidate-major; stride % 16 == 0, stride >= max(n, 16)): the trail with the last action into rows 0..g of path, g + 1
 *               into cand_length, the 20 cubie rows of the G1 cube reached into cand_cubies ([tiles][20][cand_pitch] over
 *               K * stride columns); then found[c] advances, and found[c] == K ends the cube FULL.  A root that is in G1 is emitted at
 *               init with length 0 and searched all the same (bound 0).  Candidates come out by length and, within a length, in
 *               depth-first order, each once.  depth = the number of actions on the trail; trail nibble i = action i.
 *   phase 2     one lane per column c < n (n = K * stride after phase 1).  The root is the column's cubie rows: not in G1 gives
 *               OUTSIDE.  floor[c] in 0..max_depth is the length of the prefix in rows 0..floor-1 of path column c; only its last
 *               two actions are read (a byte >= 12 there: BAD_FRAME).  g starts at floor, and limit[c] counts the TOTAL length, as
 *               min(limit[c], max_depth, floor + 32).  First bound floor + h(root); a bound above the limit is EXHAUSTED at init with
 *               next = that bound -- tested BEFORE the goal, so a column with limit -1 is skipped whatever it holds; otherwise a root
 *               that is the goal is SOLVED with length floor.  The first goal entered ends the column SOLVED: depth = the total length,
 *               rows floor..depth-1 of path receive the actions (a half turn twice); no other row is written.  depth = g, the total
 *               length at the current node; trail nibble i = generator i (0..7) of the phase-2 part (at most 32); cursor 0..8.
 *   frame       path uint8 [max_depth][path_pitch], max_depth <= 48, path_pitch % 16 == 0 (phase 1: >= K * stride; phase 2: >= n), the
 *               caller prefills 12; trail uint64 [n][2]; cursor uint8; depth, bound, next int32; nodes uint64 (children generated);
 *               found int32 (phase 1); status uint8, 0 = running, else the bits below.  The root cubies are never written.
 *   written     the search calls take any frame with status 0, as ida_search does; a refused frame gets TP_BAD_FRAME OR-ed into status,
 *               keeps every other byte of the frame, of path and of the candidate slots, and is not counted in *running.  Phase 1
 *               refuses depth outside 0..31, depth > bound, cursor > 12, bound > min(limit, max_depth, 32), found outside 0..K-1, and a
 *               trail nibble >= 12 below depth.  Phase 2 refuses a floor outside 0..max_depth or a byte >= 12 in the prefix's last two
 *               rows, g < floor, g > max_depth, g > bound, cursor > 8, bound > min(limit, max_depth, floor + 32), and a trail that does
 *               not spell g: the number of generators is not stored, they are read from nibble 0 on until their costs reach
 *               g - floor; one >= 8 on the way, or costs that step over g, are refused.  A root outside G1 is OUTSIDE here too. */
#define TP_SOLVED 1u      /* phase 2: the column is solved */
#define TP_FULL 1u        /* phase 1: K candidates were emitted */
#define TP_EXHAUSTED 2u
#define TP_ILLEGAL 4u     /* a cubie byte >= 24, a piece twice, or a table read 0xFF */
#define TP_BAD_FRAME 8u   /* floor, depth, cursor or found out of range, bound above the limit, a prefix or trail entry out of range */
#define TP_OUTSIDE 16u    /* phase 2: the root is not in G1 */
/* Conventions as in the ida_* section: caller-owned device memory, stream-ordered, nothing allocated, nothing synchronises; RC_EINVAL
 * before any launch with nothing written (rc_last_error names the operand) for a NULL or misaligned pointer, a negative size, a table
 * smaller than its N, which outside 0..3, candidates outside 1..4096, a bad stride or pitch, max_depth outside 1..48, max_steps
 * outside 1..tp_max_steps(); pad columns keep their bytes; n == 0 succeeds without a launch; every pointer needs 16-byte alignment
 * and no more.  table_a, table_b: tables 0, 1 for phase 1 and 2, 3 for phase 2.
 *
 * Host only, no device: N of table `which` (-1 for a bad one); the generators of phase 1 | 2, gens [12][2] = the one or two actions of
 * each (0xFF: none, also in the rows from *count on) and cost [12] (0 from *count on), any pointer may be NULL; the largest max_steps
 * a search call takes (one launch at it at 2^20 lanes stays near a second). */
int64_t tp_table_bytes(int which);
int tp_generators(int phase, uint8_t *gens, uint8_t *cost, int *count);
int64_t tp_max_steps(void);
/* Breadth-first build, one launch per level, as rct_build_*: tp_build_begin: every entry 0xFF, the goal 0 (one fill kernel);
 * tp_build_level: the level rule above; *count (one device uint32, 16-byte aligned, zeroed by the call) receives how many entries
 * were set to depth + 1.  depth in 0..253. */
int tp_build_begin(uint8_t *table, int64_t bytes, int which, void *stream);
int tp_build_level(uint8_t *table, int64_t bytes, int which, int depth, uint32_t *count, void *stream);
/* index[c] (uint32) = table which's index of the cubie rows ([tiles][20][cubie_pitch]) of cube c; 0xFFFFFFFF for an illegal row set
 * (a byte >= 24, a piece twice) and for a cube outside the table's domain. */
int tp_index(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, int which, uint32_t *index, void *stream);
/* Phase 1: the frame's first contents (legality, first bound, a root in G1 emitted), and at most max_steps passes per running cube;
 * the cubes still running are added to *running (one device uint32, 16-byte aligned, zeroed by the call). */
int tp_phase1_init(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                   int64_t bytes_b, const int32_t *limit, int candidates, int64_t stride, uint8_t *path, int max_depth, int64_t path_pitch,
                   int32_t *cand_length, uint8_t *cand_cubies, int64_t cand_pitch, uint64_t *trail, uint8_t *cursor, int32_t *depth,
                   int32_t *bound, int32_t *next, uint64_t *nodes, int32_t *found, uint8_t *status, void *stream);
int tp_phase1_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                     int64_t bytes_b, const int32_t *limit, int candidates, int64_t stride, uint8_t *path, int max_depth, int64_t path_pitch,
                     int32_t *cand_length, uint8_t *cand_cubies, int64_t cand_pitch, uint64_t *trail, uint8_t *cursor, int32_t *depth,
                     int32_t *bound, int32_t *next, uint64_t *nodes, int32_t *found, uint8_t *status, int64_t max_steps, uint32_t *running,
                     void *stream);
/* Phase 2, likewise, over n columns; floor may be NULL (= 0). */
int tp_phase2_init(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                   int64_t bytes_b, uint8_t *path, int max_depth, int64_t path_pitch, const int32_t *floor, const int32_t *limit,
                   uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next, uint64_t *nodes, uint8_t *status,
                   void *stream);
int tp_phase2_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                     int64_t bytes_b, uint8_t *path, int max_depth, int64_t path_pitch, const int32_t *floor, const int32_t *limit,
                     uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next, uint64_t *nodes, uint8_t *status,
                     int64_t max_steps, uint32_t *running, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------------------
 * Cube group (prefix cg_): whole cubes as group elements -- product, inverse, uniformly random cubes, and the inverse of an action
 * list.  Both cube sizes.  No reference counterpart.
 *
 * THE RULE.  Cubie bytes, slots and pieces are those of the rcc_* section (rows [tiles][SLOTS][pitch], SLOTS = 20 | 7, NC = 8 | 7);
 * a legal cube x is the group element that takes solved to x.
 *   product    x o y ("x then y") is the cube reached from x by any move sequence that takes solved to y.  In bytes, for every slot q
 *              with p = piece(y[q]):  piece(out[q]) = piece(x[p]),  ori(out[q]) = (ori(x[p]) + ori(y[q])) mod 3 (corners) | mod 2
 *              (edges).  The move tables are this rule with y = one move: rc_apply_moves by action a = the product with the cube
 *              "solved then a".
 *   inverse    for every slot q with p = piece(x[q]):  out[p] = (q, -ori(x[q])), mod 3 | mod 2.  Defined only when the corner rows and
 *              the edge rows are each a permutation.
 *   identity   the solved cube's rows.
 *   2x2x2      only the 7 stored corner rows take part; the DLB cubie is fixed.
 *   bad input  a corner byte >= 3 * NC or an edge byte >= 24, in either operand of the product or in the operand of the inverse: that
 *              cube's output is the identity and *bad is set to 1 (one device byte the caller zeroes and reads, required, as in
 *              rcc_from_cubies; set by a plain vector store).  A repeated piece in the operand of the inverse: the same.  The
 *              product does not require permutations: it is the gather as written.  Twist, flip and parity are NOT checked: the
 *              operations are defined on all assemblies, and RCC_TWIST, RCC_FLIP and RCC_PARITY of a product follow from its
 *              factors (the twist sums add mod 3, the flip sums mod 2, the permutation parities mod 2), those of an inverse are its
 *              operand's.
 *   random     cube i of a call uses the walk generator (xoroshiro128+ seeded through splitmix64, as rc_adi_generate's) seeded with
 *              (seed, stream_id, first + i); `first` lets a caller cut one stream into chunks or shards.  next64() = s0 + s1,
 *              followed by the state step every action draw makes; draw(m) = the high 64 bits of next64() * m, which deviates from
 *              uniform by less than m / 2^64 per draw.  Order of draws, 3x3x3:
 *                1 corners  from the identity permutation, for i = 7 down to 1: j = draw(i + 1), swap entries i and j;
 *                2 twists   ori[q] = draw(3) for q = 0..6; ori[7] makes the sum 0 mod 3;
 *                3 edges    as 1, for i = 11 down to 1;
 *                4 flips    one r = next64(): ori[q] = bit (63 - q) of r for q = 0..10; ori[11] makes the sum even;
 *                5 parity   if the corner permutation's parity differs from the edge permutation's, the whole bytes of edge slots
 *                           10 and 11 change places.
 *              26 generator steps, uniform over the 43 252 003 274 489 856 000 legal cubes: step 5 maps the mismatched half of the
 *              (corner, edge) permutation pairs one-to-one onto the matched half.  2x2x2: steps 1 and 2 over 7 slots (i = 6..1,
 *              twists q = 0..5, the last one fixed): 12 steps, uniform over 3 674 160 cubes.
 *   inverted actions   of a column of actions [rows][act_pitch], A = 12 | 6 the no-op: the column's non-no-op entries in reverse order,
 *              each ^ 1, then no-ops up to row rows - 1.  An entry above A is treated like the no-op and sets *bad.
 *
 * Conventions as in the rcc_* section: caller-owned device memory, stream-ordered, nothing allocated; RC_EINVAL before any launch
 * (rc_last_error names the operand); n == 0 succeeds without a launch; every pointer needs 16-byte alignment and no more; pad columns
 * and every byte outside the rows keep their bytes.  out may be exactly x or exactly y -- the same pointer AND the same pitch --, then
 * every lane reads its own columns before it writes them; any other overlap of out with an input is RC_EINVAL.  For
 * cg_invert_actions, out == actions is allowed on the same terms; its pitches are one tile's (pitch % 16 == 0, pitch >= n). */
int cg_product(const uint8_t *x, int64_t x_pitch, const uint8_t *y, int64_t y_pitch, int64_t n, int cube_size,
               uint8_t *out, int64_t out_pitch, uint8_t *bad, void *stream);
int cg_inverse(const uint8_t *x, int64_t x_pitch, int64_t n, int cube_size, uint8_t *out, int64_t out_pitch, uint8_t *bad, void *stream);
int cg_random(uint64_t seed, uint64_t stream_id, int64_t first, int64_t n, int cube_size, uint8_t *out, int64_t out_pitch, void *stream);
int cg_invert_actions(const uint8_t *actions, int64_t rows, int64_t n, int64_t act_pitch, int cube_size,
                      uint8_t *out, int64_t out_pitch, uint8_t *bad, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RUBIKHIP_H */
