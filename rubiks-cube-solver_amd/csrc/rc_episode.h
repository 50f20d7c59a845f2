// rc_episode.h -- episode bookkeeping and the masked re-scramble (include/rubikepisode.h), the last part of rubikhip.hip's
// translation unit: it uses that file's helpers (need_init, kWave, ...), rc_host.h and rc_device.h, and adds the rcx_*
// entry points to librubikhip.so.
//
//   k_episode_end     the launch after a step: counters of every cube, then solved + scramble for the cubes whose episode ended.
//                     One lane = one pack of 4 cubes (k_scramble's shape), one wave = 256 cubes.  Every lane moves 14 bytes per
//                     cube (done 1 + elapsed 4 + 4, ended 1, length 4); a wave without an ended cube stops there.  A lane with an
//                     ended cube adds 2 x S bytes per cube of its pack (the rows in and out) and 8 bytes per ended cube (episode).
#pragma once

#include "../../include/rubikepisode.h"

namespace {

struct EpisodeArgs {
    uint8_t *st;
    int64_t n, pitch;
    int shift;
    const uint8_t *done;
    int32_t *elapsed, *episode, *length;
    uint8_t *ended;
    int32_t max_steps;
    int depth_lo, depth_hi;
    uint64_t seed, stream_id, walk_offset, walk_stride;
};

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

template <class T>
__global__ void __launch_bounds__(kWave) k_episode_end(EpisodeArgs a) {
    constexpr int V = 1;
    const int64_t g0 = (int64_t)blockIdx.x * (kWave * 4 * V);
    const uint32_t lo = threadIdx.x * (4 * V);
    const int64_t n0 = g0 + lo;
    if (n0 >= a.n) return;
    const bool full = n0 + 4 <= a.n;                          // the whole pack lies inside the batch: 16-byte counter accesses
    // ---- counters: every index below is static (a run-time index would put the pack into scratch)
    const uint32_t dn = ld_tail<V>(a.done, n0, a.n, 0).d[0];
    int32_t el[4] = {0, 0, 0, 0}, len[4];
    if (full) {
        const i32x4 v = *reinterpret_cast<const i32x4 *>(a.elapsed + n0);
        el[0] = v[0]; el[1] = v[1]; el[2] = v[2]; el[3] = v[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n0 + j < a.n) el[j] = a.elapsed[n0 + j];
    }
    uint32_t end_b = 0;                                       // byte j: RCX_ENDED_* of cube n0 + j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t e = (int32_t)((uint32_t)el[j] + 1u);
        const bool term = ((dn >> (8 * j)) & 0xffu) != 0;
        const bool trunc = !term && a.max_steps > 0 && e >= a.max_steps;
        const bool end = (term || trunc) && n0 + j < a.n;     // columns past the batch never end: their stickers stay
        end_b |= (end ? (term ? (uint32_t)RCX_ENDED_TERMINATED : (uint32_t)RCX_ENDED_TRUNCATED) : 0u) << (8 * j);
        len[j] = end ? e : 0;
        el[j] = end ? 0 : e;
    }
    if (full) {
        const i32x4 ve = {el[0], el[1], el[2], el[3]}, vl = {len[0], len[1], len[2], len[3]};
        *reinterpret_cast<i32x4 *>(a.elapsed + n0) = ve;
        *reinterpret_cast<i32x4 *>(a.length + n0) = vl;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n0 + j < a.n) { a.elapsed[n0 + j] = el[j]; a.length[n0 + j] = len[j]; }
    }
    Pk<V> eb;
    eb.d[0] = end_b;
    st_tail<V>(a.ended, n0, a.n, eb);
    if (__ballot(end_b != 0) == 0) return;                    // the common case: no episode of this wave ended, st is not touched
    if (end_b == 0) return;
    // ---- the ended cubes: next episode's walk, its depth (the stream's FIRST draw), solved pattern
    WalkRng rng[4];
    int kd[4], kmax = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        rng[j].s0 = rng[j].s1 = 0;
        kd[j] = 0;
        if ((end_b >> (8 * j)) & 0xffu) {
            const int32_t ep = (int32_t)((uint32_t)a.episode[n0 + j] + 1u);
            a.episode[n0 + j] = ep;
            rng[j].seed(a.seed, a.stream_id, a.walk_offset + (uint64_t)(int64_t)ep * a.walk_stride + (uint64_t)(n0 + j));
            kd[j] = a.depth_lo;
            if (a.depth_hi > a.depth_lo) kd[j] += (int)rng[j].action((uint32_t)(a.depth_hi - a.depth_lo + 1));
        }
        kmax = kd[j] > kmax ? kd[j] : kmax;
    }
    const __amdgpu_buffer_rsrc_t rows = make_srd(a.st + tile_off(g0, a.pitch, a.shift, T::S));
    const uint32_t rs = (uint32_t)a.pitch;
    Pk<V> s[T::S];
#pragma unroll
    for (int i = 0; i < T::S; ++i) s[i] = bld<V, kAuxCached>(rows, lo, i * rs);
    Pk<V> em;                                                 // 0xff in the bytes of the ended cubes
    em.d[0] = ((end_b | (end_b >> 1)) & 0x01010101u) * 0xffu;
#pragma unroll
    for (int i = 0; i < T::S; ++i) s[i] = sel(em, solved_row<T, V>(i), s[i]);
    for (int d = 0; d < kmax; ++d) {
        Pk<V> act;                                            // the no-op A for cubes that did not end or are past their own depth
        act.d[0] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) act.d[0] |= (d < kd[j] ? rng[j].action(T::A) : (uint32_t)T::A) << (8 * j);
        (void)move_rows<T, V>(s, act);                        // actions are 0..A by construction
    }
    store_rows<kAuxCached>(rows, lo, rs, s);
}

}  // namespace

extern "C" {

int rcx_episode_end(uint8_t *stp, int64_t n, int64_t pitch, int cube_size, const uint8_t *done, int32_t *elapsed, int32_t max_steps,
                    int32_t *episode, int depth_lo, int depth_hi, uint64_t seed, uint64_t stream_id, int64_t walk_offset,
                    int64_t walk_stride, uint8_t *ended, int32_t *length, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rcx_episode_end: %s", what); };
    if (cube_size != 2 && cube_size != 3) return bad("cube_size must be 2 or 3");
    if (n < 0) return bad("n_cubes is negative");
    const int sh = tile_shift(pitch, n);
    if (!stp || !aligned16(stp)) return bad("st is NULL or not 16-byte aligned");
    if (sh < 0) return bad("bad pitch");
    if (!done || !aligned16(done)) return bad("done is NULL or not 16-byte aligned");
    if (!elapsed || !aligned16(elapsed)) return bad("elapsed is NULL or not 16-byte aligned");
    if (!episode || !aligned16(episode)) return bad("episode is NULL or not 16-byte aligned");
    if (!ended || !aligned16(ended)) return bad("ended is NULL or not 16-byte aligned");
    if (!length || !aligned16(length)) return bad("length is NULL or not 16-byte aligned");
    if (max_steps < 0) return bad("max_steps is negative");
    if (depth_lo < 0) return bad("depth_lo is negative");
    if (depth_hi < depth_lo) return bad("depth_hi is below depth_lo");
    if (walk_stride < 0) return bad("walk_stride is negative");
    if (n == 0) return RC_OK;
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        EpisodeArgs a{stp, n, pitch, sh, done, elapsed, episode, length, ended, max_steps, depth_lo, depth_hi, seed, stream_id,
                      (uint64_t)walk_offset, (uint64_t)walk_stride};
        const int64_t blocks = (n + kWave * 4 - 1) / (kWave * 4);
        RC_GRID(blocks);
        hipLaunchKernelGGL((k_episode_end<T>), dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

const char *rcx_episode_build_tag(void) { return rc_build_id(); }

}  // extern "C"
