/*
 * rubiksym.h -- the cube's symmetries on the device: an EXTENSION of librubiksearch.so (whose rc_search_* surface,
 * include/rubiksearch.h, is unchanged).
 *
 * The 3x3x3 has K = 48 symmetries: the rotations and reflections of the whole cube, each followed by the recolouring that turns
 * the moved solved cube back into the solved cube.  The 2x2x2 env never moves the DLB cubie and keeps the K = 6 of them that fix it.
 * A symmetry maps a state at distance d from solved to a state at distance d, and a solution to a solution through a fixed
 * relabelling of the moves.  Index 0 is the identity, the first K / 2 are the rotations (det +1), the rest the reflections.
 *
 * THE RULE.  With the tables of rcs_sym_tables (generated from tables.py get_symmetries into csrc/rc_sym_tables.h):
 *
 *     image[i] = relabel[s][ state[ perm[s][i] ] ]                       for every sticker i
 *
 * and T_s(move_a(x)) == move_{amap[s][a]}(T_s(x)) for every action a.  The reference (gym-cube/gym_cube/envs) has no counterpart.
 *
 * Conventions: those of include/rubiksearch.h -- caller-owned DEVICE memory, stream-ordered, no synchronisation, no allocation;
 * 0 on success, -1 for a bad argument (before anything is launched, the message names the operand), -2 for a HIP failure, the
 * message through rc_search_last_error().  State buffers are tiled [tiles][S][pitch] under the layout rules of include/rubikhip.h
 * ("State layout": one tile with pitch >= n_cubes and pitch % 16 == 0, or power-of-two tiles >= 512; S * pitch < 2^32), every
 * operand with a pitch of its own, and every pointer 16-byte aligned (16 bytes is all it needs).  The functions here carry the
 * prefix rcs_ and live in the same library; rcs_sym_count and rcs_sym_tables never touch a device.
 */
#ifndef RUBIKSYM_H
#define RUBIKSYM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* K: 48 (cube_size 3), 6 (cube_size 2); -1 for any other cube size. */
int rcs_sym_count(int cube_size);

/* Host copies of the library's tables (any pointer may be NULL), uint8, row-major:
 *   perm [K][S], relabel [K][6]   the rule above
 *   amap [K][A + 1]               the action that does to the image what a does to the state; amap[s][A] = A, the no-op
 *   inverse [K]                   applying s and then inverse[s] gives the input back
 *   compose [K][K]                compose[s][u] = the symmetry equal to applying s and then u
 * det[s] is +1 for s < K / 2 and -1 from there on.  No device is needed. */
int rcs_sym_tables(int cube_size, uint8_t *perm, uint8_t *relabel, uint8_t *amap, uint8_t *inverse, uint8_t *compose);

/* Cube n of `out` = the image of cube n of `in` under symmetry sym[n] (sym: uint8 [n_cubes], 16-byte aligned) or, when sym is
 * NULL, under sym_uniform for every cube.  `in` and `out` must not overlap.  Columns of `out` at or beyond n_cubes keep their
 * bytes, and so does every byte outside the rows.  n_cubes == 0 succeeds without a launch.
 * A sym[n] >= K cannot raise on the device: that cube gets the identity image and *bad (a uint8 in device memory that the caller
 * zeroes; may be NULL) is set to 1 -- the idea of RC_STATUS_BAD_ACTION.  sym_uniform is checked on the host.
 * Two kernels.  Uniform: the image is a row permutation of the tile, output row i = the recoloured input row perm[s][i]; it
 * moves 2 * S bytes per cube like an out-of-place rc_apply_moves.  Per cube: the workgroup's sticker block is staged in LDS and
 * every lane gathers its four cubes from it (DESIGN.md "Symmetries").
 * -1: a NULL or not 16-byte aligned in / out, a sym that is not 16-byte aligned, a bad pitch_in / pitch_out or cube_size,
 * n_cubes < 0, sym_uniform outside 0..K-1 (when sym is NULL), in == out or overlapping buffers. */
int rcs_sym_apply(const uint8_t *in, uint8_t *out, int64_t n_cubes, int64_t pitch_in, int64_t pitch_out, int cube_size,
                  const uint8_t *sym, int sym_uniform, uint8_t *bad, void *stream);

/* The canonical form up to symmetry: sym_out[n] (uint8 [n_cubes], 16-byte aligned) = the LOWEST s whose image of cube n is the
 * lexicographically smallest of the K images, compared as S-byte strings with sticker 0 first.  When `out` is not NULL that image
 * is written there at pitch_out, under the rules of rcs_sym_apply (no overlap with `in`, pad columns keep their bytes); pitch_out
 * is ignored otherwise.  Two states are images of each other exactly when their canonical images are equal.
 * -1: a NULL or misaligned in / sym_out, a misaligned out, a bad pitch_in / pitch_out or cube_size, n_cubes < 0, overlap. */
int rcs_sym_canonical(const uint8_t *in, int64_t n_cubes, int64_t pitch_in, int cube_size, uint8_t *sym_out, uint8_t *out,
                      int64_t pitch_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RUBIKSYM_H */
