// rc_cubies.h -- cubie coordinates and the legality test (include/rubikhip.h "Cubie coordinates"), a part of rubikhip.hip's
// translation unit: it uses that file's helpers (need_init, pick_v, kWave, ...), rc_host.h and rc_device.h, and adds the rcc_*
// entry points to librubikhip.so.
//
//   k_cubies        S sticker rows in, per cube: SLOTS cubie bytes, the status byte, and (INDEX) the two permutation / orientation
//                   indices.  One lane = one pack of 4 * V cubes, everything in packed bytes (rc_device.h cubies_of); the indices
//                   leave the packed domain, 4 * V scalar results per lane, and exist only in the INDEX instantiations.
//   k_from_cubies   the inverse: SLOTS cubie rows in, S sticker rows out (rc_device.h stickers_of).
// Both: raw buffer row access, whole packs; the ragged last pack of a batch merges with what the output rows hold, so pad columns
// keep their bytes (rc_device.h pack_valid, store_row).
#pragma once

namespace {

struct CubieArgs {
    const uint8_t *st;
    int64_t n, pitch;
    int sh;
    uint8_t *cubies;
    int64_t cubie_pitch;
    int sh_c;
    uint8_t *status;
    uint32_t *corner_index;
    uint64_t *edge_index;
};

template <class T, int V, bool INDEX, bool STREAM>
__global__ void __launch_bounds__(kWave) k_cubies(CubieArgs a) {
    constexpr int LD = STREAM ? kAuxStreamLoad : kAuxCached, ST = STREAM ? kAuxStreamStore : kAuxCached;
    const int64_t g0 = (int64_t)blockIdx.x * (kWave * 4 * V);
    const uint32_t lo = threadIdx.x * (4 * V);
    const int64_t n0 = g0 + lo;
    if (n0 >= a.n) return;
    const bool full = n0 + 4 * V <= a.n;
    Pk<V> s[T::S];
    {
        const __amdgpu_buffer_rsrc_t r = make_srd(a.st + tile_off(g0, a.pitch, a.sh, T::S));
        const uint32_t rs = (uint32_t)a.pitch;
#pragma unroll
        for (int i = 0; i < T::S; ++i) s[i] = bld<V, LD>(r, lo, i * rs);
    }
    Cubies<T, V> c;
    cubies_of<T, V, INDEX>(s, c);
    if (a.cubies) {
        const __amdgpu_buffer_rsrc_t r = make_srd(a.cubies + tile_off(g0, a.cubie_pitch, a.sh_c, T::SLOTS));
        const uint32_t rs = (uint32_t)a.cubie_pitch;
        Pk<V> keep;
        RC_V keep.d[k] = pack_valid(a.n - n0, k);
#pragma unroll
        for (int p = 0; p < T::SLOTS; ++p) store_row<V, ST>(r, lo, p * rs, c.code[p], full, keep);
    }
    if (a.status) st_tail<V>(a.status, n0, a.n, c.status);
    if constexpr (INDEX) {
        uint32_t ci[4 * V], el[4 * V], eo[4 * V];
        sfor<4 * V>([&](auto jc) {
            constexpr int j = decltype(jc)::value, w = j >> 2, sft = 8 * (j & 3);
            const auto byte = [&](const Pk<V> &p) { return (p.d[w] >> sft) & 0xffu; };
            const bool legal = byte(c.status) == 0;
            uint32_t lehmer = 0, oris = 0;
            sfor<T::NC>([&](auto qc) {                                           // sum_q lt[q] * (NC - 1 - q)!
                constexpr int q = decltype(qc)::value;
                lehmer = lehmer * (uint32_t)(T::NC - q) + byte(c.lt[q]);
            });
            sfor<T::NC - 1>([&](auto qc) {                                       // sum_{q < NC - 1} ori[q] * 3^q
                constexpr int q = T::NC - 2 - decltype(qc)::value;
                oris = oris * 3u + byte(c.ori[q]);
            });
            constexpr uint32_t pow3 = T::NC == 8 ? 2187u : 729u;                // 3^(NC - 1)
            ci[j] = legal ? lehmer * pow3 + oris : 0xffffffffu;
            lehmer = 0, oris = 0;
            sfor<T::NE>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                lehmer = lehmer * (uint32_t)(T::NE - q) + byte(c.lt[T::NC + q]);
            });
            sfor<(T::NE > 0 ? T::NE - 1 : 0)>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                oris |= byte(c.ori[T::NC + q]) << q;
            });
            el[j] = legal ? (lehmer << 11) | oris : 0xffffffffu;                 // edge_index = lehmer * 2^11 + oris: low, high word
            eo[j] = legal ? lehmer >> 21 : 0xffffffffu;
        });
        if (a.corner_index) {
            if (full) {
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const u32x4 u = {ci[4 * k], ci[4 * k + 1], ci[4 * k + 2], ci[4 * k + 3]};
                    *reinterpret_cast<u32x4 *>(a.corner_index + n0 + 4 * k) = u;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4 * V; ++j)
                    if (n0 + j < a.n) a.corner_index[n0 + j] = ci[j];
            }
        }
        if constexpr (T::NE > 0) {
            if (a.edge_index) {
                if (full) {
#pragma unroll
                    for (int k = 0; k < 2 * V; ++k) {
                        const u32x4 u = {el[2 * k], eo[2 * k], el[2 * k + 1], eo[2 * k + 1]};
                        *reinterpret_cast<u32x4 *>(a.edge_index + n0 + 2 * k) = u;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4 * V; ++j)
                        if (n0 + j < a.n) a.edge_index[n0 + j] = ((uint64_t)eo[j] << 32) | el[j];
                }
            }
        }
    }
}

struct FromCubieArgs {
    const uint8_t *cubies;
    int64_t n, cubie_pitch;
    int sh_c;
    uint8_t *st;
    int64_t pitch;
    int sh;
    uint8_t *bad;
};

template <class T, int V>
__global__ void __launch_bounds__(kWave) k_from_cubies(FromCubieArgs a) {
    const int64_t g0 = (int64_t)blockIdx.x * (kWave * 4 * V);
    const uint32_t lo = threadIdx.x * (4 * V);
    const int64_t n0 = g0 + lo;
    if (n0 >= a.n) return;
    const bool full = n0 + 4 * V <= a.n;
    Pk<V> code[T::SLOTS], s[T::S];
    {
        const __amdgpu_buffer_rsrc_t r = make_srd(a.cubies + tile_off(g0, a.cubie_pitch, a.sh_c, T::SLOTS));
        const uint32_t rs = (uint32_t)a.cubie_pitch;
#pragma unroll
        for (int p = 0; p < T::SLOTS; ++p) code[p] = bld<V, kAuxCached>(r, lo, p * rs);
    }
    const Pk<V> bad = stickers_of<T, V>(code, s);
    if (a.bad && any_bad<V>(bad, n0, a.n)) *a.bad = 1;                            // the idea of RC_STATUS_BAD_ACTION: a flag, no trap
    const __amdgpu_buffer_rsrc_t r = make_srd(a.st + tile_off(g0, a.pitch, a.sh, T::S));
    const uint32_t rs = (uint32_t)a.pitch;
    Pk<V> keep;
    RC_V keep.d[k] = pack_valid(a.n - n0, k);
#pragma unroll
    for (int i = 0; i < T::S; ++i) store_row<V, kAuxCached>(r, lo, i * rs, s[i], full, keep);
}

// Pack width: 8 cubes per lane from 2^18 cubes on the 2x2x2, as the step kernel; 4 always on the 3x3x3, where 8 cubes' 54 sticker rows,
// 20 cubie bytes, pieces and orientations do not fit 256 VGPRs (the V = 2 build of the index form spilled 48..136 bytes per lane).
template <class T>
int cubies_v(int64_t n) { return T::SIZE == 2 ? pick_v(n, Variant{}) : 1; }

template <class T, int V, bool INDEX>
int launch_cubies(const CubieArgs &a, hipStream_t st, bool stream_rows) {
    const int64_t blocks = (a.n + kWave * 4 * V - 1) / (kWave * 4 * V);
    RC_GRID(blocks);
    const dim3 g((unsigned)blocks), b(kWave);
    if (stream_rows) hipLaunchKernelGGL((k_cubies<T, V, INDEX, true>), g, b, 0, st, a);
    else hipLaunchKernelGGL((k_cubies<T, V, INDEX, false>), g, b, 0, st, a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

}  // namespace

extern "C" {

int rcc_cubies(const uint8_t *stp, int64_t n, int64_t pitch, int cube_size, uint8_t *cubies, int64_t cubie_pitch, uint8_t *status,
               uint32_t *corner_index, uint64_t *edge_index, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rcc_cubies: %s", what); };
    if (cube_size != 2 && cube_size != 3) return bad("cube_size must be 2 or 3");
    if (n < 0) return bad("n_cubes is negative");
    if (!stp || !aligned16(stp)) return bad("st is NULL or not 16-byte aligned");
    const int sh = tile_shift(pitch, n), sh_c = cubies ? tile_shift(cubie_pitch, n, 20) : 63;
    if (sh < 0) return bad("pitch: need pitch % 16 == 0 and pitch >= n_cubes, or a power-of-two tile >= 512");
    if (!cubies && !status && !corner_index && !edge_index) return bad("nothing to write: cubies, status, corner_index and edge_index are all NULL");
    if (cubies && !aligned16(cubies)) return bad("cubies is not 16-byte aligned");
    if (sh_c < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n_cubes, or a power-of-two tile >= 512");
    if (status && !aligned16(status)) return bad("status is not 16-byte aligned");
    if (corner_index && !aligned16(corner_index)) return bad("corner_index is not 16-byte aligned");
    if (edge_index && cube_size == 2) return bad("edge_index must be NULL for cube_size 2 (the 2x2x2 has no edges)");
    if (edge_index && !aligned16(edge_index)) return bad("edge_index is not 16-byte aligned");
    if (n == 0) return RC_OK;
    const CubieArgs a{stp, n, pitch, sh, cubies, cubie_pitch, sh_c, status, corner_index, edge_index};
    const bool index = corner_index || edge_index;
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        const bool stream_rows = n * (T::S + (cubies ? T::SLOTS : 0) + (status ? 1 : 0) + (corner_index ? 4 : 0) + (edge_index ? 8 : 0)) > kMallBytes;
        if constexpr (T::SIZE == 2)
            if (cubies_v<T>(n) == 2) return index ? launch_cubies<T, 2, true>(a, S(stream), stream_rows) : launch_cubies<T, 2, false>(a, S(stream), stream_rows);
        return index ? launch_cubies<T, 1, true>(a, S(stream), stream_rows) : launch_cubies<T, 1, false>(a, S(stream), stream_rows);
    });
}

int rcc_from_cubies(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, int cube_size, uint8_t *stp, int64_t pitch, uint8_t *badp,
                    void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rcc_from_cubies: %s", what); };
    if (cube_size != 2 && cube_size != 3) return bad("cube_size must be 2 or 3");
    if (n < 0) return bad("n_cubes is negative");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh_c = tile_shift(cubie_pitch, n, 20), sh = tile_shift(pitch, n);
    if (sh_c < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n_cubes, or a power-of-two tile >= 512");
    if (!stp || !aligned16(stp)) return bad("st is NULL or not 16-byte aligned");
    if (sh < 0) return bad("pitch: need pitch % 16 == 0 and pitch >= n_cubes, or a power-of-two tile >= 512");
    if (!badp) return bad("bad is NULL");
    if (n == 0) return RC_OK;
    const FromCubieArgs a{cubies, n, cubie_pitch, sh_c, stp, pitch, sh, badp};
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        const int v = pick_v(n, Variant{});
        const int64_t blocks = (n + kWave * 4 * v - 1) / (kWave * 4 * v);
        RC_GRID(blocks);
        if (v == 2) hipLaunchKernelGGL((k_from_cubies<T, 2>), dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
        else hipLaunchKernelGGL((k_from_cubies<T, 1>), dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

int rcc_tables(int cube_size, uint8_t *corner_cw, uint8_t *edge_facelets, uint8_t *corner_colours, uint8_t *edge_colours) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        if (corner_cw) memcpy(corner_cw, T::ccw, (size_t)T::NC * 3);
        if (corner_colours) memcpy(corner_colours, T::ccol, (size_t)T::NC * 3);
        if (edge_facelets && T::NE) memcpy(edge_facelets, T::edef, (size_t)T::NE * 2);
        if (edge_colours && T::NE) memcpy(edge_colours, T::ecol, (size_t)T::NE * 2);
        return RC_OK;
    });
}

}  // extern "C"
