/*
 * rubikepisode.h -- episode bookkeeping of librubikhip.so: an EXTENSION of include/rubikhip.h (whose surface is frozen).
 *
 * A vectorised environment restarts the cubes whose episode ended and enforces a time limit.  rcx_episode_end is the launch that
 * follows a step (rc_apply_moves): it advances the per-cube step counters, marks the cubes whose episode ended (solved = terminated,
 * or the time limit = truncated) and re-scrambles those cubes -- and only those -- from the solved cube with the per-walk generator
 * of rc_scramble.  The reference (gym-cube/gym_cube/envs/cube_env.py) has no counterpart: its reset() restarts one cube on request.
 *
 * Conventions: those of include/rubikhip.h -- caller-owned DEVICE memory, stream-ordered, no synchronisation, no allocation;
 * RC_OK / RC_EINVAL / RC_EHIP / RC_ENODEV (rc_init first), the message through rc_last_error(); `st` is a tiled state buffer
 * [tiles][S][pitch] ("State layout").  The functions here carry the prefix rcx_ and live in the same library.
 */
#ifndef RUBIKEPISODE_H
#define RUBIKEPISODE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCX_ENDED_NO 0           /* values of ended[i] */
#define RCX_ENDED_TERMINATED 1   /* done[i] != 0 */
#define RCX_ENDED_TRUNCATED 2    /* the time limit: not done and elapsed reached max_steps */

/* The end of one env step for n_cubes cubes.  done, ended [n_cubes] uint8 and elapsed, episode, length [n_cubes] int32 are 16-byte
 * aligned and accessed in packs of 4 cubes; `done` is read only.  For every cube i < n_cubes:
 *     e          = elapsed[i] + 1
 *     terminated = done[i] != 0
 *     truncated  = !terminated && max_steps > 0 && e >= max_steps          (max_steps 0: no time limit)
 *   neither:  elapsed[i] = e, ended[i] = 0, length[i] = 0; the cube's stickers and episode[i] keep their bytes;
 *   else:     ended[i] = terminated ? 1 : 2, length[i] = e, elapsed[i] = 0, ep = ++episode[i],
 *             walk = walk_offset + ep * walk_stride + i (64-bit, wrapping), a generator seeded with (seed, stream_id, walk) as in
 *             rc_scramble, k = depth_lo (+ the generator's FIRST draw below depth_hi - depth_lo + 1, when depth_hi > depth_lo),
 *             and the cube becomes the solved cube moved by the next k action draws.  With depth_lo == depth_hi that is cube i of
 *             rc_fill_solved + rc_scramble(depth = k, seed, stream_id, walk_offset + ep * walk_stride).  A fresh cube that happens
 *             to be solved stays as drawn.
 * Columns of `st` at or beyond n_cubes keep their bytes.  A wave (256 cubes) in which no episode ended does not touch `st`.
 * n_cubes == 0 succeeds without a launch.  RC_EINVAL, before anything is launched and with the operand named in the message: a NULL
 * or not 16-byte aligned st / done / elapsed / episode / ended / length, a bad pitch or cube_size, n_cubes < 0, max_steps < 0,
 * depth_lo < 0, depth_hi < depth_lo, walk_stride < 0. */
int rcx_episode_end(uint8_t *st, int64_t n_cubes, int64_t pitch, int cube_size,
                    const uint8_t *done, int32_t *elapsed, int32_t max_steps, int32_t *episode,
                    int depth_lo, int depth_hi, uint64_t seed, uint64_t stream_id,
                    int64_t walk_offset, int64_t walk_stride,
                    uint8_t *ended, int32_t *length, void *stream);

/* rc_build_id()'s string: the extension is part of the same binary and of the same source hash (this header and
 * csrc/rc_episode.h are hashed with the library's other sources).  Static storage. */
const char *rcx_episode_build_tag(void);

#ifdef __cplusplus
}
#endif
#endif /* RUBIKEPISODE_H */
