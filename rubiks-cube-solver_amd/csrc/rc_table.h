// rc_table.h -- what every exact distance table of csrc/ is built and read with (DESIGN.md "Distance tables"): the corner pattern
// database (rc_search.hip, rcp_*), the edge pattern databases (rc_edge.h, rce_*), the subgroup-chain tables (rc_chain.h, rct_*) and
// the IDA* search that reads the first two (rc_ida.h).  Included after rc_device.h and rc_host.h by rc_search.hip and rubikhip.hip,
// each into its own translation unit.
//
// A table is N bytes, entry i = the distance of index i, 0xFF = not reached (yet, or never: an entry no cube has).
//   the fill        *_build_begin: every entry 0xFF, the goals 0 -- by a kernel of the table's own (the goals differ), never by
//                   hipMemsetAsync: a captured memset node replays with other bytes (rc_search.hip "fills", include/rubikhip.h
//                   "stream order"), a kernel node replays as launched
//   k_table_level   *_build_level, level-synchronous and PULL: one lane per entry; an entry that is still 0xFF unranks itself, ranks
//                   its neighbours and becomes depth + 1 iff one of them holds `depth`.  A lane writes its own entry only; a neighbour
//                   another lane is writing meanwhile reads 0xFF or depth + 1, neither of which is `depth`: the table after a level
//                   does not depend on timing.  One ballot and one atomicAdd per wave count what the level set
// THE GUARD.  Every table address of every kernel is formed in table_at() below and nowhere else: it compares the index with the
// table size n (the host has checked bytes >= n: table_arg) before the load.  The rank functions give all-ones for a state that has
// no index, which fails that test like any other index >= n; the build's neighbour indices pass through it too.
#pragma once

namespace {

__device__ __forceinline__ uint32_t table_at(const uint8_t *table, uint32_t idx, uint32_t n) {
    return idx < n ? (uint32_t)table[idx] : 0xFFu;                        // THE GUARD: no load for an index outside the table
}

// a counter a launch adds to starts at 0 by a kernel in front of it, for the reason the fill is one
__global__ void k_zero32(uint32_t *p) { *p = 0u; }

// Space, one index space: n() its size, unrank(i) the coordinate of i < n(), neighbour<M>(c) the index of c's neighbour under move
// or generator M < kNeighbours, block_begin() what a block does before any of them (the chain's stage 3 copies a table to LDS).
template <class Space>
__global__ void __launch_bounds__(256) k_table_level(uint8_t *table, Space s, uint32_t depth, uint32_t *count) {
    s.block_begin();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, n = s.n();
    bool set = false;
    if (table_at(table, i, n) == 0xFFu && i < n) {                        // past n table_at reads nothing and says 0xFF
        const auto c = s.unrank(i);
        rc::sfor<Space::kNeighbours>([&](auto mc) {
            if (!set) set = table_at(table, s.template neighbour<decltype(mc)::value>(c), n) == depth;
        });
        if (set) table[i] = (uint8_t)(depth + 1u);                        // the lane's own entry
    }
    const unsigned long long bal = __ballot(set);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (uint32_t)__popcll(bal));
}

// The WEIGHTED level (rc_chain.h TpLevels, the two-phase tables whose half turns cost 2): Space::cost<M>() is what neighbour M costs,
// and an entry that is still 0xFF becomes depth + 1 iff a neighbour of cost w holds depth + 1 - w.  depth + 1 - w wraps above 0xFF
// when w > depth + 1, which no entry holds.  Pull and level-synchronous as above: a neighbour being written meanwhile reads 0xFF or
// depth + 1, and depth + 1 - w is neither.
template <class Space>
__global__ void __launch_bounds__(256) k_table_level_weighted(uint8_t *table, Space s, uint32_t depth, uint32_t *count) {
    s.block_begin();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, n = s.n();
    bool set = false;
    if (table_at(table, i, n) == 0xFFu && i < n) {
        const auto c = s.unrank(i);
        rc::sfor<Space::kNeighbours>([&](auto mc) {
            constexpr int M = decltype(mc)::value;
            if (!set) set = table_at(table, s.template neighbour<M>(c), n) == depth + 1u - Space::template cost<M>();
        });
        if (set) table[i] = (uint8_t)(depth + 1u);                        // the lane's own entry
    }
    const unsigned long long bal = __ballot(set);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(count, (uint32_t)__popcll(bal));
}

// a table operand: present, 16-byte aligned, and large enough for every index below n; `sizer`: the call that says how large
int table_arg(const char *fn, const void *table, int64_t bytes, uint32_t n, const char *sizer) {
    if (!table || !aligned16(table)) return fail(kEinval, "%s: table is NULL or not 16-byte aligned", fn);
    if (bytes < (int64_t)n) return fail(kEinval, "%s: bytes is smaller than %s", fn, sizer);
    return 0;
}

// *_build_level after the caller's table_arg: *count = 0, then one level over s; `ehip`: the library's code for a failed HIP call;
// WEIGHTED: the level kernel that asks the space for each neighbour's cost
template <bool WEIGHTED = false, class Space>
int table_build_level(const char *fn, uint8_t *table, Space s, int depth, uint32_t *count, hipStream_t st, int ehip) {
    if (depth < 0 || depth >= 254) return fail(kEinval, "%s: depth must be in 0..253", fn);
    if (!count || !aligned16(count)) return fail(kEinval, "%s: count is NULL or not 16-byte aligned", fn);
    hipLaunchKernelGGL(k_zero32, dim3(1), dim3(1), 0, st, count);
    RC_HIP(ehip, hipGetLastError());
    if constexpr (WEIGHTED)
        hipLaunchKernelGGL(k_table_level_weighted<Space>, dim3((s.n() + 255u) / 256u), dim3(256), 0, st, table, s, (uint32_t)depth, count);
    else
        hipLaunchKernelGGL(k_table_level<Space>, dim3((s.n() + 255u) / 256u), dim3(256), 0, st, table, s, (uint32_t)depth, count);
    RC_HIP(ehip, hipGetLastError());
    return 0;
}

// ---- index -> cubie rows, 4 cubes per lane (rcp_unrank, rce_unrank): the lane of cubes n0 .. n0 + 3, n0 % 4 == 0
// where cube b's column starts in a cubie buffer of `slots` rows (rc_host.h tile_shift gave sh)
__device__ __forceinline__ int64_t cubie_off(int64_t b, int64_t pitch, int sh, int slots) {
    return sh >= 63 ? b : rc::tiled(b, pitch, sh, slots);
}

// the pack's 4 indices, one 16-byte load; the ragged last pack byte by byte, `fill` for the cubes past n
__device__ __forceinline__ void load_index4(const uint32_t *index, int64_t n0, int64_t n, bool full, uint32_t fill, uint32_t (&idx)[4]) {
    idx[0] = idx[1] = idx[2] = idx[3] = fill;
    if (full) {
        const rc::u32x4 u = *reinterpret_cast<const rc::u32x4 *>(index + n0);
        idx[0] = u[0]; idx[1] = u[1]; idx[2] = u[2]; idx[3] = u[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (n0 + j < n) idx[j] = index[n0 + j];
    }
}

// row[q] = slot q of the pack's 4 cubes, one dword store per row; the ragged last pack byte by byte
template <int SLOTS>
__device__ __forceinline__ void store_cubie_rows4(uint8_t *cubies, int64_t n0, int64_t n, bool full, int64_t pitch, int sh, const uint32_t (&row)[SLOTS]) {
    uint8_t *dst = cubies + cubie_off(n0, pitch, sh, SLOTS);              // n0 % 4 == 0, pitch % 16 == 0: one tile, dword aligned
    if (full) {
#pragma unroll
        for (int q = 0; q < SLOTS; ++q) *reinterpret_cast<uint32_t *>(dst + (int64_t)q * pitch) = row[q];
    } else {
#pragma unroll
        for (int q = 0; q < SLOTS; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (n0 + j < n) dst[(int64_t)q * pitch + j] = (uint8_t)(row[q] >> (8 * j));   // pad columns keep their bytes
    }
}

}  // namespace
