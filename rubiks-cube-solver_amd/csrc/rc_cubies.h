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

// ================================================================================================== edge pattern databases
// The rce_* entry points (include/rubikhip.h "Edge pattern databases", DESIGN.md "Edge pattern databases"), on rc_device.h's edge
// coordinates.  3x3x3 only; the tracked set (mask, k, N = N(k)) is a kernel argument, so one kernel of each kind serves every mask.
//   k_edge_fill     every entry 0xFF, the home entry 0 (a kernel, not a memset: include/rubikhip.h "stream order")
//   k_edge_level    one lane per entry, PULL, the form of rc_search.hip k_pdb_level: an entry still 0xFF unranks itself, ranks its 12
//                   neighbours and becomes depth + 1 iff one of them holds `depth`; a lane writes its own entry only
//   k_edge_unrank   index -> the 20 cubie rows of a reachable cube, 4 cubes per lane
//   k_edge_lookup   edge rows 8..19 of a code / cubie buffer -> distance bytes (OUT 0) or scores (OUT 1 write, OUT 2 min in place)
// Every table address is formed in edge_table_at (rc_device.h) and nowhere else.
namespace {

struct EdgeSet {
    uint32_t mask, k, n, home;    // the tracked pieces, how many, N(k), the home index
};

// false: the mask names no 1..7 of the 12 pieces
inline bool edge_set(int64_t mask, EdgeSet &e) {
    if (mask <= 0 || mask > 0xFFF) return false;
    const uint32_t k = (uint32_t)__builtin_popcountll((unsigned long long)mask);
    if (k > (uint32_t)kEdgeMaxK) return false;
    uint32_t perm = 0, used = 0, i = 0;
    for (uint32_t t = 0; t < (uint32_t)kEdgeSlots; ++t)
        if (mask >> t & 1) {                                              // p_i = t_i, o_i = 0
            perm = perm * ((uint32_t)kEdgeSlots - i) + t - (uint32_t)__builtin_popcount(used & ((1u << t) - 1u));
            used |= 1u << t;
            ++i;
        }
    e = EdgeSet{(uint32_t)mask, k, edge_space((int)k), perm << k};
    return true;
}

__global__ void __launch_bounds__(256) k_edge_fill(uint8_t *table, EdgeSet e) {
    const uint32_t b0 = (blockIdx.x * 256u + threadIdx.x) * 16u;          // N(k) % 8 == 0; only N(1) = 24 is no multiple of 16
    if (b0 >= e.n) return;
    if (b0 + 16u <= e.n) {
        const uint32_t z = e.home - b0 < 16u ? ~(0xFFu << (8u * (e.home & 3u))) : ~0u, w = (e.home >> 2) & 3u;
        const u32x4 u = {w == 0 ? z : ~0u, w == 1 ? z : ~0u, w == 2 ? z : ~0u, w == 3 ? z : ~0u};
        *reinterpret_cast<u32x4 *>(table + b0) = u;
    } else {
        for (uint32_t b = b0; b < e.n; ++b) table[b] = b == e.home ? 0u : 0xFFu;
    }
}

__global__ void k_edge_zero(uint32_t *p) { *p = 0u; }

__global__ void __launch_bounds__(256) k_edge_level(uint8_t *table, EdgeSet e, uint32_t depth, uint32_t *count) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool set = false;
    if (edge_table_at(table, i, e.n) == 0xFFu && i < e.n) {               // past N edge_table_at reads nothing and says 0xFF
        const EdgeCoord c = edge_unrank(i, e.k);
        sfor<Cube3::A>([&](auto ac) {
            constexpr int A_ = decltype(ac)::value;
            if (!set) set = edge_table_at(table, edge_rank(edge_move<A_>(c, e.k), e.k), e.n) == depth;
        });
        if (set) table[i] = (uint8_t)(depth + 1u);                        // the lane's own entry
    }
    const unsigned long long bal = __ballot(set);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (uint32_t)__popcll(bal));
}

struct EdgeUnrankArgs {
    const uint32_t *index;
    int64_t n;
    uint8_t *cubies;
    int64_t pitch;
    int sh;
    uint8_t *bad;
    EdgeSet e;
};

__global__ void __launch_bounds__(256) k_edge_unrank(EdgeUnrankArgs a) {
    using T = Cube3;
    const int64_t n0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= a.n) return;
    const bool full = n0 + 4 <= a.n;
    uint32_t idx[4] = {a.e.home, a.e.home, a.e.home, a.e.home};
    if (full) {
        const u32x4 u = *reinterpret_cast<const u32x4 *>(a.index + n0);
        idx[0] = u[0]; idx[1] = u[1]; idx[2] = u[2]; idx[3] = u[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n0 + j < a.n) idx[j] = a.index[n0 + j];
    }
    uint32_t row[T::SLOTS] = {};
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = idx[j] < a.e.n;
        bad = bad || !ok;
        const EdgeCoord c = edge_unrank(ok ? idx[j] : a.e.home, a.e.k);   // out of range: home, which comes out as the solved cube
        uint64_t piece_at = 0;                                            // nibble q: the piece in slot q
        uint32_t ori_at = 0, used = 0, m = a.e.mask;
        sfor<kEdgeMaxK>([&](auto ic) {
            constexpr uint32_t i = decltype(ic)::value;
            if (i < a.e.k) {
                const uint32_t t = (uint32_t)__ffs((int)m) - 1u, p = (c.pos >> (4 * i)) & 15u;
                m &= m - 1u;
                piece_at |= (uint64_t)t << (4u * p);
                ori_at |= ((c.ori >> i) & 1u) << p;
                used |= 1u << p;
            }
        });
        // the untracked pieces fill the free slots, both ascending, ori 0; k <= 7 leaves five at the least
        uint32_t um = ~a.e.mask & 0xFFFu, fm = ~used & 0xFFFu, last = 0, last2 = 0;
        sfor<kEdgeSlots - 1>([&](auto) {
            if (um) {
                const uint32_t t = (uint32_t)__ffs((int)um) - 1u, s = (uint32_t)__ffs((int)fm) - 1u;
                um &= um - 1u;
                fm &= fm - 1u;
                piece_at |= (uint64_t)t << (4u * s);
                last2 = last;
                last = s;
            }
        });
        if (__popc(c.ori) & 1) ori_at ^= 1u << last;                      // an odd flip sum: the highest free slot's edge is flipped
        uint32_t seen = 0, odd = 0;                                       // parity of the inversion count of slot -> piece
        sfor<kEdgeSlots>([&](auto qc) {
            constexpr uint32_t q = decltype(qc)::value;
            const uint32_t p = (uint32_t)(piece_at >> (4 * q)) & 15u;
            odd ^= (uint32_t)__popc(seen >> (p + 1u));
            seen |= 1u << p;
        });
        if (odd & 1u) {                                                   // corners are home (even): the last two untracked edges trade places
            const uint64_t x = ((piece_at >> (4u * last)) ^ (piece_at >> (4u * last2))) & 15ull;
            piece_at ^= (x << (4u * last)) | (x << (4u * last2));
        }
        sfor<T::NC>([&](auto qc) { row[decltype(qc)::value] |= (3u * decltype(qc)::value) << (8 * j); });
        sfor<kEdgeSlots>([&](auto qc) {
            constexpr uint32_t q = decltype(qc)::value;
            row[T::NC + q] |= (2u * ((uint32_t)(piece_at >> (4 * q)) & 15u) + ((ori_at >> q) & 1u)) << (8 * j);
        });
    }
    if (bad) *a.bad = 1;                                                  // every writer stores the same byte
    uint8_t *dst = a.cubies + (a.sh >= 63 ? n0 : tiled(n0, a.pitch, a.sh, T::SLOTS));   // n0 % 4 == 0, pitch % 16 == 0: one tile, dword aligned
    if (full) {
#pragma unroll
        for (int q = 0; q < T::SLOTS; ++q) *reinterpret_cast<uint32_t *>(dst + (int64_t)q * a.pitch) = row[q];
    } else {
#pragma unroll
        for (int q = 0; q < T::SLOTS; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n0 + j < a.n) dst[(int64_t)q * a.pitch + j] = (uint8_t)(row[q] >> (8 * j));   // pad columns keep their bytes
    }
}

struct EdgeLookupArgs {
    const uint8_t *rows;
    int64_t n, pitch;
    int sh;
    const uint8_t *table;
    EdgeSet e;
    uint8_t *dist;
    float *scores;
};

template <int OUT>
__global__ void __launch_bounds__(kWave) k_edge_lookup(EdgeLookupArgs a) {
    using T = Cube3;
    constexpr int kEdgeSpan = kWave * 4;
    const int64_t g0 = (int64_t)blockIdx.x * kEdgeSpan;
    const uint32_t lo = threadIdx.x * 4;
    const int64_t n0 = g0 + lo;
    if (n0 >= a.n) return;
    const __amdgpu_buffer_rsrc_t r = make_srd(a.rows + tile_off(g0, a.pitch, a.sh, T::SLOTS));
    const uint32_t rs = (uint32_t)a.pitch;
    uint32_t w[kEdgeSlots];                                               // the 12 edge rows, 4 cubes per dword (pad columns are read, never used)
    sfor<kEdgeSlots>([&](auto qc) {
        constexpr uint32_t q = decltype(qc)::value;
        w[q] = bld<1, kAuxCached>(r, lo, (uint32_t)(T::NC + q) * rs).d[0];
    });
    uint32_t d[4];
    sfor<4>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        uint32_t e[kEdgeSlots];
        sfor<kEdgeSlots>([&](auto qc) { e[decltype(qc)::value] = (w[decltype(qc)::value] >> (8 * j)) & 0xFFu; });
        d[j] = edge_table_at(a.table, edge_index_of(e, a.e.mask, a.e.k), a.e.n);
    });
    if constexpr (OUT == 0) {
        Pk<1> out;
        out.d[0] = d[0] | (d[1] << 8) | (d[2] << 16) | (d[3] << 24);
        st_tail<1>(a.dist, n0, a.n, out);
    } else {                                                              // n % 4 == 0: a pack is whole or absent
        typedef float f32x4 __attribute__((ext_vector_type(4)));
        f32x4 s = {-(float)d[0], -(float)d[1], -(float)d[2], -(float)d[3]};
        f32x4 *dst = reinterpret_cast<f32x4 *>(a.scores + n0);
        if constexpr (OUT == 2) {
            const f32x4 old = *dst;
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = s[j] < old[j] ? s[j] : old[j];   // a tie (-0 against +0 too) and a NaN keep what was there
        }
        *dst = s;
    }
}

int edge_table_arg(const char *fn, int64_t mask, const void *table, int64_t bytes, EdgeSet &e) {
    if (!edge_set(mask, e)) return fail(RC_EINVAL, "%s: mask must name 1..7 of the edge pieces 0..11", fn);
    if (!table || !aligned16(table)) return fail(RC_EINVAL, "%s: table is NULL or not 16-byte aligned", fn);
    if (bytes < (int64_t)e.n) return fail(RC_EINVAL, "%s: bytes is smaller than rce_table_bytes(mask)", fn);
    return RC_OK;
}

}  // namespace

extern "C" {

int64_t rce_table_bytes(int mask) {
    EdgeSet e;
    return edge_set(mask, e) ? (int64_t)e.n : -1;
}

int64_t rce_home_index(int mask) {
    EdgeSet e;
    return edge_set(mask, e) ? (int64_t)e.home : -1;
}

int rce_tables(uint8_t *esrc, uint8_t *eflip) {
    if (esrc) memcpy(esrc, Cube3::emove_src, sizeof Cube3::emove_src);
    if (eflip) memcpy(eflip, Cube3::emove_flip, sizeof Cube3::emove_flip);
    return RC_OK;
}

int rce_build_begin(uint8_t *table, int64_t bytes, int mask, void *stream) {
    RC_NEED_INIT();
    EdgeSet e;
    if (int rc = edge_table_arg("rce_build_begin", mask, table, bytes, e)) return rc;
    hipLaunchKernelGGL(k_edge_fill, dim3((e.n + 4095u) / 4096u), dim3(256), 0, S(stream), table, e);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

int rce_build_level(uint8_t *table, int64_t bytes, int mask, int depth, uint32_t *count, void *stream) {
    RC_NEED_INIT();
    EdgeSet e;
    if (int rc = edge_table_arg("rce_build_level", mask, table, bytes, e)) return rc;
    if (depth < 0 || depth >= 254) return fail(RC_EINVAL, "rce_build_level: depth must be in 0..253");
    if (!count || !aligned16(count)) return fail(RC_EINVAL, "rce_build_level: count is NULL or not 16-byte aligned");
    hipLaunchKernelGGL(k_edge_zero, dim3(1), dim3(1), 0, S(stream), count);
    RC_HIP(RC_EHIP, hipGetLastError());
    hipLaunchKernelGGL(k_edge_level, dim3((e.n + 255u) / 256u), dim3(256), 0, S(stream), table, e, (uint32_t)depth, count);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

int rce_unrank(const uint32_t *index, int64_t n, int mask, uint8_t *cubies, int64_t cubie_pitch, uint8_t *badp, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rce_unrank: %s", what); };
    EdgeSet e;
    if (!edge_set(mask, e)) return bad("mask must name 1..7 of the edge pieces 0..11");
    if (n < 0) return bad("n is negative");
    if (!index || !aligned16(index)) return bad("indices is NULL or not 16-byte aligned");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    if (!badp) return bad("bad is NULL");
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, 1024);
    RC_GRID(blocks);
    const EdgeUnrankArgs a{index, n, cubies, cubie_pitch, sh, badp, e};
    hipLaunchKernelGGL(k_edge_unrank, dim3((unsigned)blocks), dim3(256), 0, S(stream), a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

int rce_lookup(const uint8_t *rows, int64_t n, int64_t pitch, int mask, const uint8_t *table, int64_t bytes, uint8_t *out, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rce_lookup: %s", what); };
    EdgeSet e;
    if (n < 0) return bad("n is negative");
    if (!rows || !aligned16(rows)) return bad("rows is NULL or not 16-byte aligned");
    const int sh = tile_shift(pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    if (int rc = edge_table_arg("rce_lookup", mask, table, bytes, e)) return rc;
    if (!out || !aligned16(out)) return bad("out is NULL or not 16-byte aligned");
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, kWave * 4);
    RC_GRID(blocks);
    const EdgeLookupArgs a{rows, n, pitch, sh, table, e, out, nullptr};
    hipLaunchKernelGGL(k_edge_lookup<0>, dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

int rce_score_codes(const uint8_t *code, int64_t n_problems, int width, int64_t pitch, int mask, const uint8_t *table, int64_t bytes,
                    float *scores, int combine, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rce_score_codes: %s", what); };
    EdgeSet e;
    if (n_problems < 1 || width < 1 || width > 65536) return bad("need n_problems >= 1 and 1 <= width <= 65536");
    if (tile_shift(pitch, INT64_MAX, Cube3::S) < 0) return bad("pitch must be a power of two >= 512 with S * pitch < 2^32");
    if (!code || !aligned16(code)) return bad("code is NULL or not 16-byte aligned");
    if (int rc = edge_table_arg("rce_score_codes", mask, table, bytes, e)) return rc;
    if (!scores || !aligned16(scores)) return bad("scores is NULL or not 16-byte aligned");
    if (combine != 0 && combine != 1) return bad("combine must be 0 (write) or 1 (min in place)");
    const int64_t total = (int64_t)Cube3::A * ceil_div(n_problems * width, pitch) * pitch;   // every slot, a multiple of 512
    const int64_t blocks = total / (kWave * 4);
    RC_GRID(blocks);
    const EdgeLookupArgs a{code, total, pitch, log2_exact(pitch), table, e, nullptr, scores};
    if (combine) hipLaunchKernelGGL(k_edge_lookup<2>, dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
    else hipLaunchKernelGGL(k_edge_lookup<1>, dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

}  // extern "C"

// ================================================================================================== subgroup chain
// The rct_* entry points (include/rubikhip.h "Subgroup chain", DESIGN.md "Subgroup chain"): Thistlethwaite's four coset-distance
// tables and the descent that walks any cube home through them.  3x3x3 only; the stage is a template argument, so a stage's kernels
// hold its generators and its coordinate alone.
//   k_chain_fill      every entry 0xFF, the goals 0 (a kernel, not a memset: include/rubikhip.h "stream order")
//   k_chain_level     one lane per entry, PULL, the form of k_edge_level: an entry still 0xFF unranks itself, ranks its neighbours and
//                     becomes depth + 1 iff one of them holds `depth`; a lane writes its own entry only
//   k_chain_index     20 cubie rows -> the stage's index, one lane per cube
//   k_chain_unrank    index -> the 20 cubie rows of a reachable cube of the stage's domain, one lane per cube
//   k_chain_descend   the walk: one lane per cube, at most kChainWalk generators, every table read through chain_table_at
// The cube lives in four registers of nibbles and bits (ChainCube), never in an indexed array (no scratch); a generator is a
// compile-time gather on them, and what a stage's coordinate does not read the compiler drops.
namespace {

constexpr int kChainWalk = 16;                                            // the deepest table has 15 levels
constexpr uint32_t kChainN[4] = {2048u, 2187u * 495u, 40320u * 70u, 96u * 24u * 24u * 24u};
constexpr uint32_t kChainSliceHome = 494u, kChainEHome = 20u, kChainNH = 96u;

struct ChainCube {
    uint32_t cp, co;   // nibble q: the piece in corner slot q, its ori
    uint64_t ep;       // nibble q: the piece in edge slot q
    uint32_t eo;       // bit q: its ori
};
constexpr uint32_t kChainCornersHome = 0x76543210u;
constexpr uint64_t kChainEdgesHome = 0xBA9876543210ull;

struct ChainHDev {
    uint16_t v[kChainNH];
    constexpr ChainHDev() : v{} {
        for (uint32_t i = 0; i < kChainNH; ++i) v[i] = Cube3::chain_h[i];
    }
};
__constant__ ChainHDev c_chain_h{};

// generator G of a stage as gathers: the action once, or twice for a half turn
struct ChainGen {
    uint8_t csrc[8], ctw[8], esrc[12], eflip[12], action, half;
};
constexpr ChainGen chain_gen(int stage, int g) {
    ChainGen r{};
    const int code = Cube3::chain_gen[stage][g], a = code & 15;
    r.action = (uint8_t)a;
    r.half = (uint8_t)(code >> 4);
    for (int q = 0; q < 8; ++q) {
        int s = Cube3::cmove_src[a][q], t = Cube3::cmove_twist[a][q];
        if (r.half) {
            t = (t + Cube3::cmove_twist[a][s]) % 3;
            s = Cube3::cmove_src[a][s];
        }
        r.csrc[q] = (uint8_t)s;
        r.ctw[q] = (uint8_t)t;
    }
    for (int q = 0; q < 12; ++q) {
        int s = Cube3::emove_src[a][q], f = Cube3::emove_flip[a][q];
        if (r.half) {
            f ^= Cube3::emove_flip[a][s];
            s = Cube3::emove_src[a][s];
        }
        r.esrc[q] = (uint8_t)s;
        r.eflip[q] = (uint8_t)f;
    }
    return r;
}
template <int STAGE, int G>
struct ChainGenOf {
    static constexpr ChainGen v = chain_gen(STAGE, G);
};

template <int STAGE, int G>
__device__ __forceinline__ ChainCube chain_move(const ChainCube &c) {
    using M = ChainGenOf<STAGE, G>;
    ChainCube r{0u, 0u, 0ull, 0u};
    sfor<8>([&](auto qc) {
        constexpr int q = decltype(qc)::value, s = M::v.csrc[q], t = M::v.ctw[q];
        r.cp |= ((c.cp >> (4 * s)) & 15u) << (4 * q);
        if constexpr (t == 0) {
            r.co |= ((c.co >> (4 * s)) & 15u) << (4 * q);
        } else {
            const uint32_t o = ((c.co >> (4 * s)) & 3u) + (uint32_t)t;
            r.co |= (o >= 3u ? o - 3u : o) << (4 * q);
        }
    });
    sfor<12>([&](auto qc) {
        constexpr int q = decltype(qc)::value, s = M::v.esrc[q], f = M::v.eflip[q];
        r.ep |= ((c.ep >> (4 * s)) & 15ull) << (4 * q);
        r.eo |= (((c.eo >> s) & 1u) ^ (uint32_t)f) << q;
    });
    return r;
}

// THE GUARD of the chain tables: the only place a table address is formed.  n = N(stage); the host has checked bytes >= n.
__device__ __forceinline__ uint32_t chain_table_at(const uint8_t *table, uint32_t idx, uint32_t n) {
    return idx < n ? (uint32_t)table[idx] : 0xFFu;
}

constexpr uint32_t chain_binom(int m, int j) {
    if (j < 0 || j > m) return 0u;
    uint32_t r = 1;
    for (int i = 0; i < j; ++i) r = r * (uint32_t)(m - i) / (uint32_t)(i + 1);
    return r;
}
// C(m, 4 - i) for i = 0..3 (RANK) | C(m, 3 - i) (UNRANK), 16 bits each
constexpr uint64_t chain_binom_row(int m, int top) {
    uint64_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint64_t)chain_binom(m, top - i) << (16 * i);
    return r;
}

// the lexicographic rank of the sorted tuple of the 4 set bits of `mask` among the 4-subsets of {0..NS-1}
template <int NS>
__device__ __forceinline__ uint32_t chain_subset_rank(uint32_t mask) {
    uint32_t i = 0, sum = 0;
    sfor<NS>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        constexpr uint64_t row = chain_binom_row(NS - 1 - q, 4);
        const uint32_t bit = (mask >> q) & 1u;
        sum += bit ? (uint32_t)(row >> (16u * (i & 3u))) & 0xFFFFu : 0u;
        i += bit;
    });
    return chain_binom(NS, 4) - 1u - sum;
}
template <int NS>
__device__ __forceinline__ uint32_t chain_subset_unrank(uint32_t rank) {
    uint32_t i = 0, mask = 0;
    sfor<NS>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        constexpr uint64_t row = chain_binom_row(NS - 1 - q, 3);
        const uint32_t with = (uint32_t)(row >> (16u * (i & 3u))) & 0xFFFFu;   // the subsets whose next member is q
        const bool take = i < 4u && rank < with;
        if (i < 4u && !take) rank -= with;
        mask |= (uint32_t)take << q;
        i += (uint32_t)take;
    });
    return mask;
}

// lehmer of the N nibbles of v, a permutation of 0..N-1: sum_q #{r > q : v[r] < v[q]} * (N - 1 - q)!; *odd: the permutation's parity
template <int N>
__device__ __forceinline__ uint32_t chain_lehmer(uint64_t v, uint32_t *odd = nullptr) {
    uint32_t lehmer = 0, unused = 0xFFFFu, sum = 0;
    sfor<N>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t p = (uint32_t)(v >> (4 * q)) & 15u, d = (uint32_t)__popc(unused & ((1u << p) - 1u));
        lehmer = lehmer * (uint32_t)(N - q) + d;
        sum += d;
        unused &= ~(1u << p);
    });
    if (odd) *odd = sum & 1u;
    return lehmer;
}
// the inverse on the ascending values of `list` (nibble 0 first)
template <int N>
__device__ __forceinline__ uint64_t chain_unlehmer(uint32_t lehmer, uint64_t list, uint32_t *odd = nullptr) {
    uint32_t dig = 0, sum = 0;
    sfor<N>([&](auto xc) {
        constexpr int q = N - 1 - decltype(xc)::value;
        const uint32_t d = lehmer % (uint32_t)(N - q);
        lehmer /= (uint32_t)(N - q);
        dig |= d << (4 * q);
        sum += d;
    });
    uint64_t out = 0;
    sfor<N>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t sh = 4u * ((dig >> (4 * q)) & 15u);
        const uint64_t low = (1ull << sh) - 1ull;
        out |= ((list >> sh) & 15ull) << (4 * q);
        list = (list & low) | ((list >> 4) & ~low);
    });
    if (odd) *odd = sum & 1u;
    return out;
}

// the rank of `key` in sorted H (h: its copy in LDS), all-ones when it is no member
__device__ __forceinline__ uint32_t chain_h_rank(const uint16_t *h, uint32_t key) {
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = 64; step; step >>= 1) {
        const uint32_t at = lo + step < kChainNH ? lo + step : kChainNH - 1u;
        if (lo + step < kChainNH && h[at] <= key) lo += step;
    }
    return h[lo] == key ? lo : 0xffffffffu;
}
__device__ __forceinline__ void chain_h_load(uint16_t *h) {
    for (uint32_t i = threadIdx.x; i < kChainNH; i += blockDim.x) h[i] = c_chain_h.v[i];
    __syncthreads();
}

// nibbles 0, 2, 4, 6 | 1, 3, 5, 7 of the low dword of ep, packed into 4 nibbles
__device__ __forceinline__ uint32_t chain_alternate(uint32_t e, int odd) {
    e >>= 4 * odd;
    return (e & 15u) | ((e >> 4) & 0xF0u) | ((e >> 8) & 0xF00u) | ((e >> 12) & 0xF000u);
}

// the stage's domain, for a cube of 20 distinct pieces (stage 3: but for the corner permutation's membership of H, which
// chain_index reports)
template <int STAGE>
__device__ __forceinline__ bool chain_domain(const ChainCube &c) {
    bool ok = true;
    if constexpr (STAGE >= 1) ok = c.eo == 0u;
    if constexpr (STAGE >= 2) ok = ok && c.co == 0u && ((uint32_t)(c.ep >> 32) & 0x8888u) == 0x8888u;
    if constexpr (STAGE >= 3) ok = ok && ((uint32_t)c.ep & 0x01010101u) == 0u;
    return ok;
}

// the stage's index of a cube of its domain (include/rubikhip.h "Subgroup chain"); stage 3: all-ones when lehmer(cp) is not in H
template <int STAGE>
__device__ __forceinline__ uint32_t chain_index(const ChainCube &c, const uint16_t *h) {
    if constexpr (STAGE == 0) {
        return c.eo & 0x7FFu;
    } else if constexpr (STAGE == 1) {
        uint32_t twist = 0, slice = 0;
        sfor<7>([&](auto qc) {
            constexpr int q = 6 - decltype(qc)::value;
            twist = twist * 3u + ((c.co >> (4 * q)) & 3u);
        });
        sfor<12>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            slice |= ((uint32_t)(c.ep >> (4 * q + 3)) & 1u) << q;
        });
        return twist + 2187u * chain_subset_rank<12>(slice);
    } else if constexpr (STAGE == 2) {
        uint32_t even = 0;
        sfor<8>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            even |= (~(uint32_t)(c.ep >> (4 * q)) & 1u) << q;
        });
        return chain_lehmer<8>(c.cp) + 40320u * chain_subset_rank<8>(even);
    } else {
        const uint32_t r = chain_h_rank(h, chain_lehmer<8>(c.cp));
        // pieces 0, 2, 4, 6 | 1, 3, 5, 7 | 8..11 as 0..3: chain_lehmer counts among ALL smaller values
        const uint32_t m = chain_lehmer<4>((chain_alternate((uint32_t)c.ep, 0) >> 1) & 0x3333u),
                       s = chain_lehmer<4>((chain_alternate((uint32_t)c.ep, 1) >> 1) & 0x3333u), e = chain_lehmer<4>((uint32_t)(c.ep >> 32) & 0x3333u);
        return r == 0xffffffffu ? r : ((r * 24u + m) * 24u + s) * 24u + e;
    }
}

// spread the nibbles of `pieces` (ascending from nibble 0) over the set bits of `slots`, lowest slot first
__device__ __forceinline__ uint64_t chain_place(uint32_t slots, uint64_t pieces) {
    uint64_t out = 0;
    sfor<12>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        if ((slots >> q) & 1u) {
            out |= (pieces & 15ull) << (4 * q);
            pieces >>= 4;
        }
    });
    return out;
}
__device__ __forceinline__ uint64_t chain_swap(uint64_t ep, uint32_t a, uint32_t b) {
    const uint64_t x = ((ep >> (4u * a)) ^ (ep >> (4u * b))) & 15ull;
    return ep ^ (x << (4u * a)) ^ (x << (4u * b));
}

// A reachable cube of the stage's domain with index idx < N (include/rubikhip.h rct_unrank states what the index leaves free);
// false: a stage-3 index whose corner and edge permutations differ in parity, which no cube has (the coordinates come out all the same:
// the build walks them, and they never meet a legal entry)
template <int STAGE>
__device__ __forceinline__ bool chain_unrank(uint32_t idx, const uint16_t *h, ChainCube &c) {
    c = ChainCube{kChainCornersHome, 0u, kChainEdgesHome, 0u};
    if constexpr (STAGE == 0) {
        c.eo = idx | (((uint32_t)__popc(idx) & 1u) << 11);
        return true;
    } else if constexpr (STAGE == 1) {
        uint32_t tw = idx % 2187u, sum = 0;
        const uint32_t slice = chain_subset_unrank<12>(idx / 2187u), rest = ~slice & 0xFFFu;
        sfor<7>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const uint32_t d = tw % 3u;
            tw /= 3u;
            c.co |= d << (4 * q);
            sum += d;
        });
        c.co |= ((3u - sum % 3u) % 3u) << 28;                                 // the last corner closes the twist
        c.ep = chain_place(slice, 0xBA98ull) | chain_place(rest, 0x76543210ull);
        uint32_t odd;
        chain_lehmer<12>(c.ep, &odd);
        const uint32_t last = 31u - (uint32_t)__clz((int)rest), last2 = 31u - (uint32_t)__clz((int)(rest & ~(1u << last)));
        if (odd) c.ep = chain_swap(c.ep, last, last2);                        // corners are home (even)
        return true;
    } else if constexpr (STAGE == 2) {
        uint32_t codd, eodd;
        const uint32_t even = chain_subset_unrank<8>(idx / 40320u), rest = ~even & 0xFFu;
        c.cp = (uint32_t)chain_unlehmer<8>(idx % 40320u, kChainCornersHome, &codd);
        c.ep = chain_place(even, 0x6420ull) | chain_place(rest, 0x7531ull) | (kChainEdgesHome & 0xFFFF00000000ull);
        chain_lehmer<12>(c.ep, &eodd);
        if (codd != eodd) c.ep = chain_swap(c.ep, 10u, 11u);
        return true;
    } else {
        const uint32_t e = idx % 24u, s = idx / 24u % 24u, m = idx / 576u % 24u, r = idx / 13824u;
        uint32_t codd, modd, sodd, eodd;
        c.cp = (uint32_t)chain_unlehmer<8>(h[r < kChainNH ? r : 0u], kChainCornersHome, &codd);
        const uint64_t mv = chain_unlehmer<4>(m, 0x6420ull, &modd), sv = chain_unlehmer<4>(s, 0x7531ull, &sodd),
                       ev = chain_unlehmer<4>(e, 0xBA98ull, &eodd);
        c.ep = chain_place(0x55u, mv) | chain_place(0xAAu, sv) | (ev << 32);
        return codd == (modd ^ sodd ^ eodd);
    }
}

// the 20 cubie bytes of cube `at` -> c; false: a byte names no cubie, or a piece occurs twice
__device__ __forceinline__ bool chain_load(const uint8_t *at, int64_t pitch, ChainCube &c) {
    c = ChainCube{0u, 0u, 0ull, 0u};
    uint32_t cseen = 0, eseen = 0, bad = 0;
    sfor<8>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t b = at[(int64_t)q * pitch], p = (b * 171u) >> 9, o = b - 3u * p;
        bad |= (uint32_t)(b >= 24u) | ((cseen >> (p & 7u)) & 1u);
        cseen |= 1u << (p & 7u);
        c.cp |= (p & 7u) << (4 * q);
        c.co |= o << (4 * q);
    });
    sfor<12>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t b = at[(int64_t)(8 + q) * pitch], p = (b >> 1) & 15u;
        bad |= (uint32_t)(b >= 24u) | ((eseen >> p) & 1u);
        eseen |= 1u << p;
        c.ep |= (uint64_t)p << (4 * q);
        c.eo |= (b & 1u) << q;
    });
    return bad == 0u;
}
__device__ __forceinline__ void chain_store(uint8_t *at, int64_t pitch, const ChainCube &c) {
    sfor<8>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        at[(int64_t)q * pitch] = (uint8_t)(3u * ((c.cp >> (4 * q)) & 15u) + ((c.co >> (4 * q)) & 3u));
    });
    sfor<12>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        at[(int64_t)(8 + q) * pitch] = (uint8_t)(2u * ((uint32_t)(c.ep >> (4 * q)) & 15u) + ((c.eo >> q) & 1u));
    });
}
__device__ __forceinline__ int64_t chain_cube_off(int64_t b, int64_t pitch, int sh) {
    return sh >= 63 ? b : tiled(b, pitch, sh, Cube3::SLOTS);
}

__global__ void __launch_bounds__(256) k_chain_fill(uint8_t *table, uint32_t n, int stage) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    bool goal = i == (stage == 1 ? kChainSliceHome * 2187u : 0u);
    if (stage == 2) {
        goal = false;
        if (i / 40320u == kChainEHome) goal = chain_h_rank(c_chain_h.v, i % 40320u) != 0xffffffffu;
    }
    table[i] = goal ? 0u : 0xFFu;
}

template <int STAGE>
__global__ void __launch_bounds__(256) k_chain_level(uint8_t *table, uint32_t depth, uint32_t *count) {
    constexpr uint32_t N = kChainN[STAGE];
    __shared__ uint16_t h[kChainNH];
    if constexpr (STAGE == 3) chain_h_load(h);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool set = false;
    if (chain_table_at(table, i, N) == 0xFFu && i < N) {                  // past N chain_table_at reads nothing and says 0xFF
        ChainCube c;
        chain_unrank<STAGE>(i, h, c);
        sfor<Cube3::chain_ngen[STAGE]>([&](auto gc) {
            constexpr int G = decltype(gc)::value;
            if (!set) set = chain_table_at(table, chain_index<STAGE>(chain_move<STAGE, G>(c), h), N) == depth;
        });
        if (set) table[i] = (uint8_t)(depth + 1u);                        // the lane's own entry
    }
    const unsigned long long bal = __ballot(set);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (uint32_t)__popcll(bal));
}

template <int STAGE>
__global__ void __launch_bounds__(256) k_chain_index(const uint8_t *cubies, int64_t n, int64_t pitch, int sh, uint32_t *index) {
    __shared__ uint16_t h[kChainNH];
    if constexpr (STAGE == 3) chain_h_load(h);
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    ChainCube c;
    const bool ok = chain_load(cubies + chain_cube_off(b, pitch, sh), pitch, c) && chain_domain<STAGE>(c);
    const uint32_t idx = chain_index<STAGE>(c, h);
    index[b] = ok && idx < kChainN[STAGE] ? idx : 0xffffffffu;
}

template <int STAGE>
__global__ void __launch_bounds__(256) k_chain_unrank(const uint32_t *index, int64_t n, uint8_t *cubies, int64_t pitch, int sh, uint8_t *bad) {
    __shared__ uint16_t h[kChainNH];
    if constexpr (STAGE == 3) chain_h_load(h);
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const uint32_t idx = index[b];
    ChainCube c;
    if (!(idx < kChainN[STAGE] && chain_unrank<STAGE>(idx, h, c))) {
        c = ChainCube{kChainCornersHome, 0u, kChainEdgesHome, 0u};        // the solved cube
        *bad = 1;                                                         // every writer stores the same byte
    }
    chain_store(cubies + chain_cube_off(b, pitch, sh), pitch, c);
}

struct ChainDescendArgs {
    uint8_t *cubies;
    int64_t n, pitch;
    int sh;
    const uint8_t *table;
    uint8_t *actions;
    int32_t max_length;
    int64_t act_pitch;
    int32_t *length;
    uint8_t *moves, *status;
};

template <int STAGE>
__global__ void __launch_bounds__(256) k_chain_descend(ChainDescendArgs a) {
    constexpr uint32_t N = kChainN[STAGE];
    __shared__ uint16_t h[kChainNH];
    if constexpr (STAGE == 3) chain_h_load(h);
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= a.n) return;
    uint8_t *at = a.cubies + chain_cube_off(b, a.pitch, a.sh);
    ChainCube c;
    uint32_t status = 0, d = 0xFFu;
    if (!chain_load(at, a.pitch, c)) {
        status = RCT_ILLEGAL;
    } else {
        d = chain_table_at(a.table, chain_domain<STAGE>(c) ? chain_index<STAGE>(c, h) : 0xffffffffu, N);
        if (d == 0xFFu) status = RCT_OUTSIDE;
    }
    a.moves[b] = (uint8_t)d;
    int32_t len = a.length[b];
    if (!status && (len < 0 || (int64_t)len + 2 * (int64_t)d > (int64_t)a.max_length)) status = RCT_NO_ROOM;
    if (!status && d) {
        for (int step = 0; step < kChainWalk; ++step) {                   // a constant bound: the walk ends whatever the table holds
            if (d && !status) {
                ChainCube next = c;
                uint32_t act = 0xFFu, twice = 0;
                sfor<Cube3::chain_ngen[STAGE]>([&](auto gc) {             // every child is read; the first that is one closer is taken
                    constexpr int G = decltype(gc)::value;
                    const ChainCube child = chain_move<STAGE, G>(c);
                    const bool take = act == 0xFFu && chain_table_at(a.table, chain_index<STAGE>(child, h), N) == d - 1u;
                    constexpr uint32_t kAction = ChainGenOf<STAGE, G>::v.action, kHalf = ChainGenOf<STAGE, G>::v.half;
                    if (take) {
                        next = child;
                        act = kAction;
                        twice = kHalf;
                    }
                });
                if (act == 0xFFu) {
                    status = RCT_STUCK;
                } else {
                    for (uint32_t k = 0; k <= twice; ++k)
                        if (len < a.max_length) a.actions[(int64_t)len++ * a.act_pitch + b] = (uint8_t)act;   // room was checked; the guard stays
                    c = next;
                    --d;
                }
            }
        }
        if (d && !status) status = RCT_STUCK;                             // a foreign table deeper than the walk's bound
        chain_store(at, a.pitch, c);
        a.length[b] = len;
    }
    a.status[b] = (uint8_t)status;
}

template <class F>
int by_stage(int stage, F &&f) {
    switch (stage) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 3>{});
    }
}

int chain_table_arg(const char *fn, int stage, const void *table, int64_t bytes) {
    if (stage < 0 || stage > 3) return fail(RC_EINVAL, "%s: stage must be in 0..3", fn);
    if (!table || !aligned16(table)) return fail(RC_EINVAL, "%s: table is NULL or not 16-byte aligned", fn);
    if (bytes < (int64_t)kChainN[stage]) return fail(RC_EINVAL, "%s: bytes is smaller than rct_table_bytes(stage)", fn);
    return RC_OK;
}

}  // namespace

extern "C" {

int64_t rct_table_bytes(int stage) { return stage < 0 || stage > 3 ? -1 : (int64_t)kChainN[stage]; }

int rct_generators(int stage, uint8_t *gens, int *count) {
    if (stage < 0 || stage > 3) return fail(RC_EINVAL, "rct_generators: stage must be in 0..3");
    if (gens)
        for (int g = 0; g < 12; ++g) {
            const int code = Cube3::chain_gen[stage][g];
            gens[2 * g] = g < Cube3::chain_ngen[stage] ? (uint8_t)(code & 15) : 0xFFu;
            gens[2 * g + 1] = g < Cube3::chain_ngen[stage] && (code >> 4) ? (uint8_t)(code & 15) : 0xFFu;
        }
    if (count) *count = Cube3::chain_ngen[stage];
    return RC_OK;
}

int rct_corner_cosets(uint16_t *h) {
    if (h) memcpy(h, Cube3::chain_h, sizeof Cube3::chain_h);
    return RC_OK;
}

int rct_build_begin(uint8_t *table, int64_t bytes, int stage, void *stream) {
    RC_NEED_INIT();
    if (int rc = chain_table_arg("rct_build_begin", stage, table, bytes)) return rc;
    hipLaunchKernelGGL(k_chain_fill, dim3((kChainN[stage] + 255u) / 256u), dim3(256), 0, S(stream), table, kChainN[stage], stage);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

int rct_build_level(uint8_t *table, int64_t bytes, int stage, int depth, uint32_t *count, void *stream) {
    RC_NEED_INIT();
    if (int rc = chain_table_arg("rct_build_level", stage, table, bytes)) return rc;
    if (depth < 0 || depth >= 254) return fail(RC_EINVAL, "rct_build_level: depth must be in 0..253");
    if (!count || !aligned16(count)) return fail(RC_EINVAL, "rct_build_level: count is NULL or not 16-byte aligned");
    hipLaunchKernelGGL(k_edge_zero, dim3(1), dim3(1), 0, S(stream), count);
    RC_HIP(RC_EHIP, hipGetLastError());
    return by_stage(stage, [&](auto sc) {
        constexpr int STAGE = decltype(sc)::value;
        hipLaunchKernelGGL(k_chain_level<STAGE>, dim3((kChainN[STAGE] + 255u) / 256u), dim3(256), 0, S(stream), table, (uint32_t)depth, count);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

int rct_index(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, int stage, uint32_t *index, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rct_index: %s", what); };
    if (stage < 0 || stage > 3) return bad("stage must be in 0..3");
    if (n < 0) return bad("n is negative");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    if (!index || !aligned16(index)) return bad("index is NULL or not 16-byte aligned");
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, 256);
    RC_GRID(blocks);
    return by_stage(stage, [&](auto sc) {
        hipLaunchKernelGGL(k_chain_index<decltype(sc)::value>, dim3((unsigned)blocks), dim3(256), 0, S(stream), cubies, n, cubie_pitch, sh, index);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

int rct_unrank(const uint32_t *index, int64_t n, int stage, uint8_t *cubies, int64_t cubie_pitch, uint8_t *badp, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rct_unrank: %s", what); };
    if (stage < 0 || stage > 3) return bad("stage must be in 0..3");
    if (n < 0) return bad("n is negative");
    if (!index || !aligned16(index)) return bad("indices is NULL or not 16-byte aligned");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    if (!badp) return bad("bad is NULL");
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, 256);
    RC_GRID(blocks);
    return by_stage(stage, [&](auto sc) {
        hipLaunchKernelGGL(k_chain_unrank<decltype(sc)::value>, dim3((unsigned)blocks), dim3(256), 0, S(stream), index, n, cubies, cubie_pitch, sh, badp);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

int rct_descend(uint8_t *cubies, int64_t n, int64_t cubie_pitch, int stage, const uint8_t *table, int64_t bytes, uint8_t *actions,
                int max_length, int64_t act_pitch, int32_t *length, uint8_t *moves, uint8_t *status, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "rct_descend: %s", what); };
    if (n < 0) return bad("n is negative");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    if (int rc = chain_table_arg("rct_descend", stage, table, bytes)) return rc;
    if (!actions || !aligned16(actions)) return bad("actions is NULL or not 16-byte aligned");
    if (max_length < 1) return bad("max_length must be positive");
    if (act_pitch < n || (act_pitch & 15) != 0) return bad("act_pitch: need act_pitch % 16 == 0 and act_pitch >= n");
    if (!length || !aligned16(length)) return bad("length is NULL or not 16-byte aligned");
    if (!moves || !aligned16(moves)) return bad("moves is NULL or not 16-byte aligned");
    if (!status || !aligned16(status)) return bad("status is NULL or not 16-byte aligned");
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, 256);
    RC_GRID(blocks);
    const ChainDescendArgs a{cubies, n, cubie_pitch, sh, table, actions, max_length, act_pitch, length, moves, status};
    return by_stage(stage, [&](auto sc) {
        hipLaunchKernelGGL(k_chain_descend<decltype(sc)::value>, dim3((unsigned)blocks), dim3(256), 0, S(stream), a);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

}  // extern "C"

// ================================================================================================== iterative-deepening A*
// The ida_* entry points (include/rubikhip.h "Iterative-deepening A*", DESIGN.md "IDA*"): Korf's cost-bounded depth-first search under
// the maximum of the corner table and up to four edge tables, one lane per cube, no node memory.  3x3x3 only.
//   k_ida_init      legality, the prefix replayed, the first bound, the frame's first contents
//   k_ida_search    at most max_steps passes of the state machine per cube; a pass applies ONE move to the cube in registers -- the next
//                   canonical child, or the inverse of the last move to go back a level -- then ranks, reads the tables and compares
// The cube lives in five registers of cubie bytes (IdaCube); a move is a byte gather (v_perm_b32) whose selectors come from a row of
// s_moves, the 13 rows (12 actions and the identity) in LDS: the move index varies by lane, so nothing here is a compile-time gather
// and nothing is a switch.  The trail lives in two 64-bit registers of nibbles.  No indexed array, no scratch.
namespace {

constexpr int kIdaMaxDepth = 32, kIdaMaxEdge = 4;
constexpr uint32_t kIdaNoMove = 12u;
constexpr int32_t kIdaInf = 0x7FFFFFFF;
constexpr int64_t kIdaMaxSteps = (int64_t)1 << 14;                          // DESIGN.md "IDA*": 0.83 s a launch at 2^20 cubes, three tables

// THE RULE's canonical moves: bit m set = move m may follow a path that ends ..., p2, p1 (12: no move)
__host__ __device__ constexpr uint32_t ida_allowed(uint32_t p2, uint32_t p1) {
    uint32_t m = 0xFFFu;
    if (p1 < kIdaNoMove) {
        m &= ~(1u << (p1 ^ 1u));                                          // the inverse
        if ((p1 & 1u) || p1 == p2) m &= ~(1u << p1);                      // a half turn is the even action twice; never three times
        if (p1 >= 6u) m &= ~(3u << ((p1 & ~1u) - 6u));                    // of the commuting faces f, f + 3 the lower one goes first
    }
    return m;
}

// Row a of the move table: 0, 1 the corner selectors; 2, 3 the twists in the high nibbles; 4 + 2j, 5 + 2j the selectors of edge dword j
// from (e1, e0) and from e2 (0x0c: a zero byte); 10..12 the flips.  Row 12 is the identity.
struct IdaMoves {
    uint32_t w[13][16];
    constexpr IdaMoves() : w{} {
        for (int a = 0; a < 13; ++a) {
            for (int q = 0; q < 8; ++q) {
                const uint32_t s = a < 12 ? Cube3::cmove_src[a][q] : (uint32_t)q, t = a < 12 ? Cube3::cmove_twist[a][q] : 0u;
                w[a][q >> 2] |= s << (8 * (q & 3));
                w[a][2 + (q >> 2)] |= (t << 4) << (8 * (q & 3));
            }
            for (int q = 0; q < 12; ++q) {
                const uint32_t s = a < 12 ? Cube3::emove_src[a][q] : (uint32_t)q, f = a < 12 ? Cube3::emove_flip[a][q] : 0u;
                w[a][4 + 2 * (q >> 2)] |= (s < 8u ? s : 0x0cu) << (8 * (q & 3));
                w[a][5 + 2 * (q >> 2)] |= (s < 8u ? 0x0cu : s - 8u) << (8 * (q & 3));
                w[a][10 + (q >> 2)] |= f << (8 * (q & 3));
            }
        }
    }
};
__constant__ IdaMoves c_ida_moves{};

struct IdaCube {
    uint32_t c0, c1;       // byte q: corner slot q, piece | ori << 4
    uint32_t e0, e1, e2;   // byte q: edge slot q, the cubie byte piece * 2 + ori
};

__device__ __forceinline__ void ida_moves_load(uint32_t (*s_moves)[16]) {
    for (uint32_t i = threadIdx.x; i < 13u * 16u; i += blockDim.x) s_moves[i >> 4][i & 15u] = c_ida_moves.w[i >> 4][i & 15u];
    __syncthreads();
}

__device__ __forceinline__ IdaCube ida_move(const IdaCube &x, const uint32_t *row) {
    const u32x4 a = *reinterpret_cast<const u32x4 *>(row), b = *reinterpret_cast<const u32x4 *>(row + 4),
                c = *reinterpret_cast<const u32x4 *>(row + 8);
    const uint32_t f2 = row[12];
    IdaCube y;
    const auto twist = [](uint32_t v) { return v - (((v + 0x10101010u) >> 6) & 0x01010101u) * 0x30u; };   // ori 3, 4 -> 0, 1
    y.c0 = twist(__builtin_amdgcn_perm(x.c1, x.c0, a[0]) + a[2]);
    y.c1 = twist(__builtin_amdgcn_perm(x.c1, x.c0, a[1]) + a[3]);
    y.e0 = (__builtin_amdgcn_perm(x.e1, x.e0, b[0]) | __builtin_amdgcn_perm(0u, x.e2, b[1])) ^ c[2];
    y.e1 = (__builtin_amdgcn_perm(x.e1, x.e0, b[2]) | __builtin_amdgcn_perm(0u, x.e2, b[3])) ^ c[3];
    y.e2 = (__builtin_amdgcn_perm(x.e1, x.e0, c[0]) | __builtin_amdgcn_perm(0u, x.e2, c[1])) ^ f2;
    return y;
}

__device__ __forceinline__ bool ida_goal(const IdaCube &x) {
    return ((x.c0 ^ 0x03020100u) | (x.c1 ^ 0x07060504u) | (x.e0 ^ 0x06040200u) | (x.e1 ^ 0x0E0C0A08u) | (x.e2 ^ 0x16141210u)) == 0u;
}

// the 20 cubie bytes of cube `at` -> x; false: a byte names no cubie, or a piece occurs twice
__device__ __forceinline__ bool ida_load(const uint8_t *at, int64_t pitch, IdaCube &x) {
    uint32_t c[2] = {0u, 0u}, e[3] = {0u, 0u, 0u}, cseen = 0, eseen = 0, bad = 0;
    sfor<8>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t b = at[(int64_t)q * pitch], p = ((b * 171u) >> 9) & 7u, o = (b - 3u * ((b * 171u) >> 9)) & 3u;
        bad |= (uint32_t)(b >= 24u) | ((cseen >> p) & 1u);
        cseen |= 1u << p;
        c[q >> 2] |= (p | (o << 4)) << (8 * (q & 3));
    });
    sfor<12>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t b = at[(int64_t)(8 + q) * pitch], p = (b >> 1) & 15u;
        bad |= (uint32_t)(b >= 24u) | ((eseen >> p) & 1u);
        eseen |= 1u << p;
        e[q >> 2] |= (b & 31u) << (8 * (q & 3));
    });
    x = IdaCube{c[0], c[1], e[0], e[1], e[2]};
    return bad == 0u;
}

struct IdaTables {
    const uint8_t *corner;                 // NULL: no corner table
    const uint8_t *edge[kIdaMaxEdge];
    EdgeSet set[kIdaMaxEdge];
    int n_edge;
};

// THE GUARD of the corner table in this section: the only place its address is formed (the host has checked bytes >= N)
__device__ __forceinline__ uint32_t ida_corner_at(const uint8_t *table, uint32_t idx) {
    return idx < CornerSpace<Cube3>::N ? (uint32_t)table[idx] : 0xFFu;
}

// h = the maximum over the tables, 0 with none, 0xFF as soon as one reads 0xFF; !live: no table is read (every index is all-ones)
__device__ __forceinline__ uint32_t ida_h(const IdaCube &x, const IdaTables &t, bool live) {
    uint32_t h = live ? 0u : 0xFFu;
    if (t.corner) {
        uint32_t unused = 0xFFu, lehmer = 0, oris = 0;
        sfor<8>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const uint32_t p = ((q < 4 ? x.c0 : x.c1) >> (8 * (q & 3))) & 15u;
            lehmer = lehmer * (uint32_t)(8 - q) + (uint32_t)__popc(unused & ((1u << p) - 1u));
            unused &= ~(1u << p);
        });
        sfor<7>([&](auto qc) {
            constexpr int q = 6 - decltype(qc)::value;
            oris = oris * 3u + (((q < 4 ? x.c0 : x.c1) >> (8 * (q & 3) + 4)) & 3u);
        });
        const uint32_t d = ida_corner_at(t.corner, live ? lehmer * CornerSpace<Cube3>::POW3 + oris : 0xffffffffu);
        h = d > h ? d : h;
    }
    uint32_t e[kEdgeSlots];
    sfor<kEdgeSlots>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        e[q] = ((q < 4 ? x.e0 : q < 8 ? x.e1 : x.e2) >> (8 * (q & 3))) & 0xFFu;
    });
    sfor<kIdaMaxEdge>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if (i < t.n_edge) {
            const uint32_t d = edge_table_at(t.edge[i], live ? edge_index_of(e, t.set[i].mask, t.set[i].k) : 0xffffffffu, t.set[i].n);
            h = d > h ? d : h;
        }
    });
    return h;
}

__device__ __forceinline__ uint32_t ida_nib(uint64_t lo, uint64_t hi, int i) {   // i in 0..31
    return (uint32_t)((i & 16 ? hi : lo) >> (4 * (i & 15))) & 15u;
}
__device__ __forceinline__ void ida_nib_set(uint64_t &lo, uint64_t &hi, int i, uint32_t v) {
    const uint64_t keep = ~(15ull << (4 * (i & 15))), put = (uint64_t)v << (4 * (i & 15));
    if (i & 16) hi = (hi & keep) | put;
    else lo = (lo & keep) | put;
}

struct IdaArgs {
    const uint8_t *cubies;
    int64_t n, pitch;
    int sh;
    IdaTables t;
    uint8_t *path;
    int32_t max_depth;
    int64_t path_pitch;
    const int32_t *floor, *limit;
    uint64_t *trail;
    uint8_t *cursor;
    int32_t *depth, *bound, *next;
    uint64_t *nodes;
    uint8_t *status;
    int64_t max_steps;
    uint32_t *running;
};

__global__ void __launch_bounds__(kWave) k_ida_init(IdaArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_moves[13][16];
    ida_moves_load(s_moves);
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (c >= a.n) return;
    IdaCube x;
    uint32_t status = ida_load(a.cubies + chain_cube_off(c, a.pitch, a.sh), a.pitch, x) ? 0u : IDA_ILLEGAL;
    const int32_t f = a.floor ? a.floor[c] : 0;
    if (f < 0 || f > a.max_depth) status |= IDA_BAD_FRAME;
    uint64_t lo = 0, hi = 0;
    for (int r = 0; r < kIdaMaxDepth; ++r) {                              // the prefix: rows below floor <= max_depth are the caller's
        uint32_t m = kIdaNoMove;
        if (!status && r < f) {
            m = a.path[(int64_t)r * a.path_pitch + c];
            if (m >= kIdaNoMove) {
                status |= IDA_BAD_FRAME;
                m = kIdaNoMove;
            }
        }
        x = ida_move(x, s_moves[m]);
        if (r < f) ida_nib_set(lo, hi, r, m);
    }
    const uint32_t h = ida_h(x, a.t, status == 0u);
    if (!status && h == 0xFFu) status = IDA_ILLEGAL;
    int32_t depth = 0, bound = 0, next = kIdaInf;
    if (!status) {
        const int32_t lim = a.limit[c] < a.max_depth ? a.limit[c] : a.max_depth;
        depth = f;
        bound = f + (int32_t)h;
        if (ida_goal(x)) {
            status = IDA_SOLVED;
        } else if (bound > lim) {
            status = IDA_EXHAUSTED;
            next = bound;
        }
    } else {
        lo = hi = 0;
    }
    a.trail[2 * c] = lo;
    a.trail[2 * c + 1] = hi;
    a.cursor[c] = 0;
    a.depth[c] = depth;
    a.bound[c] = bound;
    a.next[c] = next;
    a.nodes[c] = 0;
    a.status[c] = (uint8_t)status;
}

__global__ void __launch_bounds__(kWave) k_ida_search(IdaArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_moves[13][16];
    ida_moves_load(s_moves);
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const bool mine = c < a.n && a.status[c] == 0u;                       // a cube with a nonzero status is not touched
    IdaCube x{};
    uint64_t lo = 0, hi = 0, nodes = 0;
    uint32_t status = 0, cursor = 0;
    int32_t f = 0, depth = 0, bound = 0, next = kIdaInf, lim = 0;
    if (mine) {
        if (!ida_load(a.cubies + chain_cube_off(c, a.pitch, a.sh), a.pitch, x)) status = IDA_ILLEGAL;
        f = a.floor ? a.floor[c] : 0;
        lo = a.trail[2 * c];
        hi = a.trail[2 * c + 1];
        cursor = a.cursor[c];
        depth = a.depth[c];
        bound = a.bound[c];
        next = a.next[c];
        nodes = a.nodes[c];
        lim = a.limit[c] < a.max_depth ? a.limit[c] : a.max_depth;
        if (f < 0 || f > a.max_depth || depth < f || depth > a.max_depth || cursor > kIdaNoMove || bound > lim) status |= IDA_BAD_FRAME;
    }
    for (int r = 0; r < kIdaMaxDepth; ++r) {                              // the current node: the root moved along the trail
        uint32_t m = kIdaNoMove;
        if (mine && !status && r < depth) {
            m = ida_nib(lo, hi, r);
            if (m >= kIdaNoMove) {
                status |= IDA_BAD_FRAME;
                m = kIdaNoMove;
            }
        }
        x = ida_move(x, s_moves[m]);
    }
    bool run = mine && !status;
    for (int64_t step = 0; step < a.max_steps; ++step) {                  // the only loop: whatever the tables hold, it ends
        if (__ballot(run) == 0ull) break;
        if (run) {
            const int g = depth;
            const uint32_t p1 = g >= 1 ? ida_nib(lo, hi, g - 1) : kIdaNoMove, p2 = g >= 2 ? ida_nib(lo, hi, g - 2) : kIdaNoMove;
            const uint32_t open = ida_allowed(p2, p1) & (0xFFFu << cursor) & 0xFFFu;
            const bool gen = open != 0u, back = !gen && g > f;
            const uint32_t m = gen ? (uint32_t)__ffs((int)open) - 1u : kIdaNoMove;
            const IdaCube y = ida_move(x, s_moves[gen ? m : back ? (p1 ^ 1u) : kIdaNoMove]);
            const uint32_t h = ida_h(y, a.t, gen);
            if (gen) {
                ++nodes;
                const int32_t fv = g + 1 + (int32_t)h;
                if (h == 0xFFu) {
                    status = IDA_ILLEGAL;
                    run = false;
                } else if (fv > bound) {
                    next = fv < next ? fv : next;
                    cursor = m + 1u;
                } else {                                                  // fv <= bound <= max_depth: row g exists
                    x = y;
                    ida_nib_set(lo, hi, g, m);
                    depth = g + 1;
                    cursor = 0;
                    if (ida_goal(y)) {
                        status = IDA_SOLVED;
                        run = false;
                    }
                }
            } else if (back) {
                x = y;
                cursor = p1 + 1u;
                depth = g - 1;
            } else if (next > lim) {                                      // the iteration is exhausted
                status = IDA_EXHAUSTED;
                run = false;
            } else {
                bound = next;
                next = kIdaInf;
                cursor = 0;
            }
        }
    }
    if (mine) {
        a.trail[2 * c] = lo;
        a.trail[2 * c + 1] = hi;
        a.cursor[c] = (uint8_t)cursor;
        a.depth[c] = depth;
        a.bound[c] = bound;
        a.next[c] = next;
        a.nodes[c] = nodes;
        a.status[c] = (uint8_t)status;
        if (status == IDA_SOLVED)
            for (int r = 0; r < kIdaMaxDepth; ++r)
                if (r >= f && r < depth) a.path[(int64_t)r * a.path_pitch + c] = (uint8_t)ida_nib(lo, hi, r);   // depth <= max_depth
    }
    const unsigned long long bal = __ballot(run);
    if (threadIdx.x == 0 && bal) atomicAdd(a.running, (uint32_t)__popcll(bal));
}

int ida_args(const char *fn, const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *corner, int64_t corner_bytes, int n_edge,
             const int *masks, const uint8_t *const *edge_tables, const int64_t *edge_bytes, uint8_t *path, int max_depth, int64_t path_pitch,
             const int32_t *floor, const int32_t *limit, uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next,
             uint64_t *nodes, uint8_t *status, IdaArgs &a) {
    const auto bad = [fn](const char *what) { return fail(RC_EINVAL, "%s: %s", fn, what); };
    if (n < 0) return bad("n is negative");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    IdaTables t{};
    if (corner) {
        if (!aligned16(corner)) return bad("corner_table is not 16-byte aligned");
        if (corner_bytes < (int64_t)CornerSpace<Cube3>::N) return bad("corner_bytes is smaller than the corner table of the 3x3x3 (88 179 840)");
        t.corner = corner;
    }
    if (n_edge < 0 || n_edge > kIdaMaxEdge) return bad("n_edge must be in 0..4");
    if (n_edge && (!masks || !edge_tables || !edge_bytes)) return bad("masks, edge_tables or edge_bytes is NULL with n_edge > 0");
    t.n_edge = n_edge;
    for (int i = 0; i < n_edge; ++i) {
        if (int rc = edge_table_arg(fn, masks[i], edge_tables[i], edge_bytes[i], t.set[i])) return rc;
        t.edge[i] = edge_tables[i];
    }
    if (!path || !aligned16(path)) return bad("path is NULL or not 16-byte aligned");
    if (max_depth < 1 || max_depth > kIdaMaxDepth) return bad("max_depth must be in 1..32");
    if (path_pitch < n || (path_pitch & 15) != 0) return bad("path_pitch: need path_pitch % 16 == 0 and path_pitch >= n");
    if (floor && !aligned16(floor)) return bad("floor is not 16-byte aligned");
    if (!limit || !aligned16(limit)) return bad("limit is NULL or not 16-byte aligned");
    if (!trail || !aligned16(trail)) return bad("trail is NULL or not 16-byte aligned");
    if (!cursor || !aligned16(cursor)) return bad("cursor is NULL or not 16-byte aligned");
    if (!depth || !aligned16(depth)) return bad("depth is NULL or not 16-byte aligned");
    if (!bound || !aligned16(bound)) return bad("bound is NULL or not 16-byte aligned");
    if (!next || !aligned16(next)) return bad("next is NULL or not 16-byte aligned");
    if (!nodes || !aligned16(nodes)) return bad("nodes is NULL or not 16-byte aligned");
    if (!status || !aligned16(status)) return bad("status is NULL or not 16-byte aligned");
    a = IdaArgs{cubies, n, cubie_pitch, sh, t, path, max_depth, path_pitch, floor, limit, trail, cursor, depth, bound, next, nodes, status, 0, nullptr};
    return RC_OK;
}

}  // namespace

extern "C" {

int64_t ida_max_steps(void) { return kIdaMaxSteps; }

int ida_canonical(uint8_t *allowed) {
    if (!allowed) return fail(RC_EINVAL, "ida_canonical: allowed is NULL");
    for (uint32_t p2 = 0; p2 < 13u; ++p2)
        for (uint32_t p1 = 0; p1 < 13u; ++p1)
            for (uint32_t m = 0; m < 12u; ++m) allowed[(p2 * 13u + p1) * 12u + m] = (uint8_t)((ida_allowed(p2, p1) >> m) & 1u);
    return RC_OK;
}

int ida_init(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *corner_table, int64_t corner_bytes, int n_edge,
             const int *masks, const uint8_t *const *edge_tables, const int64_t *edge_bytes, uint8_t *path, int max_depth, int64_t path_pitch,
             const int32_t *floor, const int32_t *limit, uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next,
             uint64_t *nodes, uint8_t *status, void *stream) {
    RC_NEED_INIT();
    IdaArgs a;
    if (int rc = ida_args("ida_init", cubies, n, cubie_pitch, corner_table, corner_bytes, n_edge, masks, edge_tables, edge_bytes, path, max_depth,
                          path_pitch, floor, limit, trail, cursor, depth, bound, next, nodes, status, a))
        return rc;
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, kWave);
    RC_GRID(blocks);
    hipLaunchKernelGGL(k_ida_init, dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

int ida_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *corner_table, int64_t corner_bytes, int n_edge,
               const int *masks, const uint8_t *const *edge_tables, const int64_t *edge_bytes, uint8_t *path, int max_depth, int64_t path_pitch,
               const int32_t *floor, const int32_t *limit, uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next,
               uint64_t *nodes, uint8_t *status, int64_t max_steps, uint32_t *running, void *stream) {
    RC_NEED_INIT();
    IdaArgs a;
    if (int rc = ida_args("ida_search", cubies, n, cubie_pitch, corner_table, corner_bytes, n_edge, masks, edge_tables, edge_bytes, path,
                          max_depth, path_pitch, floor, limit, trail, cursor, depth, bound, next, nodes, status, a))
        return rc;
    if (max_steps < 1 || max_steps > kIdaMaxSteps) return fail(RC_EINVAL, "ida_search: max_steps must be in 1..ida_max_steps()");
    if (!running || !aligned16(running)) return fail(RC_EINVAL, "ida_search: running is NULL or not 16-byte aligned");
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, kWave);
    RC_GRID(blocks);
    a.max_steps = max_steps;
    a.running = running;
    hipLaunchKernelGGL(k_edge_zero, dim3(1), dim3(1), 0, S(stream), running);
    RC_HIP(RC_EHIP, hipGetLastError());
    hipLaunchKernelGGL(k_ida_search, dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

}  // extern "C"
