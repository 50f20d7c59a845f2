// rc_edge.h -- edge pattern databases: the rce_* entry points (include/rubikhip.h "Edge pattern databases", DESIGN.md "Edge pattern
// databases"), on rc_device.h's edge coordinates and rc_table.h's table core; a part of rubikhip.hip's translation unit, after
// rc_cubies.h.  3x3x3 only; the tracked set (mask, k, N = N(k)) is a kernel argument, so one kernel of each kind serves every mask.
//   k_edge_fill     every entry 0xFF, the home entry 0
//   EdgeLevels      the index space of a tracked set under k_table_level: 12 neighbours per entry
//   k_edge_unrank   index -> the 20 cubie rows of a reachable cube, 4 cubes per lane
//   k_edge_lookup   edge rows 8..19 of a code / cubie buffer -> distance bytes (OUT 0) or scores (OUT 1 write, OUT 2 min in place)
#pragma once

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

struct EdgeLevels {
    static constexpr int kNeighbours = Cube3::A;
    EdgeSet e;
    __host__ __device__ uint32_t n() const { return e.n; }
    __device__ void block_begin() const {}
    __device__ EdgeCoord unrank(uint32_t i) const { return edge_unrank(i, e.k); }
    template <int A_>
    __device__ uint32_t neighbour(EdgeCoord c) const { return edge_rank(edge_move<A_>(c, e.k), e.k); }
};

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
    uint32_t idx[4];
    load_index4(a.index, n0, a.n, full, a.e.home, idx);
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
    store_cubie_rows4(a.cubies, n0, a.n, full, a.pitch, a.sh, row);
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
        d[j] = table_at(a.table, edge_index_of(e, a.e.mask, a.e.k), a.e.n);
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
    return table_arg(fn, table, bytes, e.n, "rce_table_bytes(mask)");
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
    return table_build_level("rce_build_level", table, EdgeLevels{e}, depth, count, S(stream), RC_EHIP);
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
