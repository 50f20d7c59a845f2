// rc_ida.h -- iterative-deepening A*: the ida_* entry points (include/rubikhip.h "Iterative-deepening A*", DESIGN.md "IDA*"): Korf's
// cost-bounded depth-first search under the maximum of the corner table and up to four edge tables (read through rc_table.h
// table_at), one lane per cube, no node memory.  A part of rubikhip.hip's translation unit, after rc_edge.h (EdgeSet, edge_table_arg)
// and rc_chain.h (load_cubie_bytes).  3x3x3 only.
//   k_ida_init      legality, the prefix replayed, the first bound, the frame's first contents
//   k_ida_search    at most max_steps passes of the state machine per cube; a pass applies ONE move to the cube in registers -- the next
//                   canonical child, or the inverse of the last move to go back a level -- then ranks, reads the tables and compares
// The cube lives in five registers of cubie bytes (IdaCube); a move is a byte gather (v_perm_b32) whose selectors come from a row of
// s_moves, the 13 rows (12 actions and the identity) in LDS: the move index varies by lane, so nothing here is a compile-time gather
// and nothing is a switch.  The trail lives in two 64-bit registers of nibbles.  No indexed array, no scratch.
#pragma once

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

// load_cubie_bytes (rc_chain.h) into the bytes of x
__device__ __forceinline__ bool ida_load(const uint8_t *at, int64_t pitch, IdaCube &x) {
    uint32_t w[5] = {0u, 0u, 0u, 0u, 0u};                                 // c0, c1, e0, e1, e2: slot s is byte s & 3 of w[s >> 2]
    const bool ok = load_cubie_bytes(at, pitch, [&](auto sc, uint32_t piece, uint32_t ori, uint32_t b) {
        constexpr int s = decltype(sc)::value;
        w[s >> 2] |= (s < 8 ? piece | (ori << 4) : b & 31u) << (8 * (s & 3));
    });
    x = IdaCube{w[0], w[1], w[2], w[3], w[4]};
    return ok;
}

struct IdaTables {
    const uint8_t *corner;                 // NULL: no corner table
    const uint8_t *edge[kIdaMaxEdge];
    EdgeSet set[kIdaMaxEdge];
    int n_edge;
};

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
        const uint32_t d = table_at(t.corner, live ? lehmer * CornerSpace<Cube3>::POW3 + oris : 0xffffffffu, CornerSpace<Cube3>::N);
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
            const uint32_t d = table_at(t.edge[i], live ? edge_index_of(e, t.set[i].mask, t.set[i].k) : 0xffffffffu, t.set[i].n);
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
    uint32_t status = ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x) ? 0u : IDA_ILLEGAL;
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
        if (!ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x)) status = IDA_ILLEGAL;
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
    hipLaunchKernelGGL(k_zero32, dim3(1), dim3(1), 0, S(stream), running);
    RC_HIP(RC_EHIP, hipGetLastError());
    hipLaunchKernelGGL(k_ida_search, dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

}  // extern "C"

// ================================================================================================================== two-phase
// The tp_* entry points (include/rubikhip.h "Two-phase", DESIGN.md "Two-phase"): Kociemba's two phases on the state machine above.
//   k_tp1_init / k_tp1_search   phase 1: one lane per cube under max(twist-slice, flip-slice); up to K G1 candidates per cube are
//                               emitted (path column, length, cubie rows), the search never enters G1
//   k_tp2_init / k_tp2_search   phase 2: one lane per candidate column under max(corner-slice, edge-slice), stage 2's generators with
//                               a half turn costing 2; the first goal ends the lane
// The tables and tp_index are rc_chain.h's TpLevels / k_tp_index.  The cube is an IdaCube; the 13 move rows are extended by the four
// half turns F2, R2, B2, L2, so a phase-2 generator is one gather.  Both tables are ranked before either is read.
namespace {

constexpr int kTpMaxDepth = 48, kTpMaxTrail = 32, kTpRows = 17, kTpMaxK = 4096;
constexpr int64_t kTpMaxSteps = (int64_t)1 << 17;                           // DESIGN.md "Two-phase": 0.73 | 0.89 s a launch at 2^20 lanes

struct TpMoves {
    uint32_t w[kTpRows][16];
    constexpr TpMoves() : w{} {
        const IdaMoves base{};
        for (int a = 0; a < 13; ++a)
            for (int i = 0; i < 16; ++i) w[a][i] = base.w[a][i];
        const int half[4] = {1, 2, 4, 5};                                  // F2, R2, B2, L2 among stage 3's U2 F2 R2 D2 B2 L2
        for (int k = 0; k < 4; ++k) {
            const ChainGen g = chain_gen(3, half[k]);
            const int a = 13 + k;
            for (int q = 0; q < 8; ++q) {
                w[a][q >> 2] |= (uint32_t)g.csrc[q] << (8 * (q & 3));
                w[a][2 + (q >> 2)] |= ((uint32_t)g.ctw[q] << 4) << (8 * (q & 3));
            }
            for (int q = 0; q < 12; ++q) {
                const uint32_t s = g.esrc[q];
                w[a][4 + 2 * (q >> 2)] |= (s < 8u ? s : 0x0cu) << (8 * (q & 3));
                w[a][5 + 2 * (q >> 2)] |= (s < 8u ? 0x0cu : s - 8u) << (8 * (q & 3));
                w[a][10 + (q >> 2)] |= (uint32_t)g.eflip[q] << (8 * (q & 3));
            }
        }
    }
};
__constant__ TpMoves c_tp_moves{};

__device__ __forceinline__ void tp_moves_load(uint32_t (*s_moves)[16]) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)kTpRows * 16u; i += blockDim.x) s_moves[i >> 4][i & 15u] = c_tp_moves.w[i >> 4][i & 15u];
    __syncthreads();
}

// phase 2's generator j in 0..7 = U, U', F2, R2, D, D', B2, L2: its first action, its cost, its row of s_moves and its inverse's
__device__ __forceinline__ uint32_t tp_gen_action(uint32_t j) { return (0xA8764210u >> (4u * j)) & 15u; }
__device__ __forceinline__ uint32_t tp_gen_half(uint32_t j) { return (0xCCu >> j) & 1u; }
__device__ __forceinline__ uint32_t tp_gen_row(uint32_t j) { return (uint32_t)(0x100F07060E0D0100ull >> (8u * j)) & 0xFFu; }
__device__ __forceinline__ uint32_t tp_gen_back(uint32_t j) { return (uint32_t)(0x100F06070E0D0001ull >> (8u * j)) & 0xFFu; }
// ida_allowed's 12 bits -> the 8 generators, each by its first action
__device__ __forceinline__ uint32_t tp_gen_allowed(uint32_t m) {
    return (m & 3u) | (((m >> 2) & 1u) << 2) | (((m >> 4) & 1u) << 3) | (((m >> 6) & 3u) << 4) | (((m >> 8) & 1u) << 6) | (((m >> 10) & 1u) << 7);
}

// bit j = bit 0 of byte j
__device__ __forceinline__ uint32_t tp_bits4(uint32_t v) { return ((v & 0x01010101u) * 0x01020408u) >> 24; }

template <int N, class P>
__device__ __forceinline__ uint32_t tp_lehmer(P &&piece) {
    uint32_t unused = 0xFFFFu, lehmer = 0;
    sfor<N>([&](auto qc) {
        const uint32_t p = piece(qc);
        lehmer = lehmer * (uint32_t)(N - decltype(qc)::value) + (uint32_t)__popc(unused & ((1u << p) - 1u));
        unused &= ~(1u << p);
    });
    return lehmer;
}

struct TpTables {
    const uint8_t *a, *b;                  // phase 1: twist-slice, flip-slice; phase 2: corner-slice, edge-slice
};

// h of phase 1 = max(table 0, table 1), 0xFF as soon as one reads 0xFF; !live: no table is read
__device__ __forceinline__ uint32_t tp_h1(const IdaCube &x, const TpTables &t, bool live) {
    uint32_t twist = 0;
    sfor<7>([&](auto qc) {
        constexpr int q = 6 - decltype(qc)::value;
        twist = twist * 3u + (((q < 4 ? x.c0 : x.c1) >> (8 * (q & 3) + 4)) & 3u);
    });
    const uint32_t slice = tp_bits4(x.e0 >> 4) | (tp_bits4(x.e1 >> 4) << 4) | (tp_bits4(x.e2 >> 4) << 8),   // byte >= 16: piece >= 8
                   flip = (tp_bits4(x.e0) | (tp_bits4(x.e1) << 4) | (tp_bits4(x.e2) << 8)) & 0x7FFu, C = chain_subset_rank<12>(slice);
    const uint32_t i0 = live ? twist + 2187u * C : 0xffffffffu, i1 = live ? flip + 2048u * C : 0xffffffffu;
    const uint32_t d0 = table_at(t.a, i0, kTpN[0]), d1 = table_at(t.b, i1, kTpN[1]);
    return d0 > d1 ? d0 : d1;
}

__device__ __forceinline__ bool tp_in_g1(const IdaCube &x) {
    return ((x.c0 | x.c1) & 0x30303030u) == 0u && ((x.e0 | x.e1 | x.e2) & 0x01010101u) == 0u && (x.e2 & 0x10101010u) == 0x10101010u &&
           ((x.e0 | x.e1) & 0x10101010u) == 0u;
}

// h of phase 2 on a cube of G1
__device__ __forceinline__ uint32_t tp_h2(const IdaCube &x, const TpTables &t, bool live) {
    const uint32_t cl = tp_lehmer<8>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        return ((q < 4 ? x.c0 : x.c1) >> (8 * (q & 3))) & 7u;
    });
    const uint32_t el = tp_lehmer<8>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        return ((q < 4 ? x.e0 : x.e1) >> (8 * (q & 3) + 1)) & 7u;
    });
    const uint32_t s = tp_lehmer<4>([&](auto qc) { return (x.e2 >> (8 * decltype(qc)::value + 1)) & 3u; });
    const uint32_t i2 = live ? cl * 24u + s : 0xffffffffu, i3 = live ? el * 24u + s : 0xffffffffu;
    const uint32_t d2 = table_at(t.a, i2, kTpN[2]), d3 = table_at(t.b, i3, kTpN[3]);
    return d2 > d3 ? d2 : d3;
}

__device__ __forceinline__ void tp_store(uint8_t *at, int64_t pitch, const IdaCube &x) {
    sfor<8>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t v = ((q < 4 ? x.c0 : x.c1) >> (8 * (q & 3))) & 0xFFu;
        at[(int64_t)q * pitch] = (uint8_t)((v & 15u) * 3u + (v >> 4));
    });
    sfor<12>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        at[(int64_t)(8 + q) * pitch] = (uint8_t)(((q < 4 ? x.e0 : q < 8 ? x.e1 : x.e2) >> (8 * (q & 3))) & 0xFFu);
    });
}

struct Tp1Args {
    const uint8_t *cubies;
    int64_t n, pitch;
    int sh;
    TpTables t;
    const int32_t *limit;
    int32_t K;
    int64_t stride;
    uint8_t *path;
    int32_t max_depth;
    int64_t path_pitch;
    int32_t *cand_length;
    uint8_t *cand;
    int64_t cand_pitch;
    int cand_sh;
    uint64_t *trail;
    uint8_t *cursor;
    int32_t *depth, *bound, *next;
    uint64_t *nodes;
    int32_t *found;
    uint8_t *status;
    int64_t max_steps;
    uint32_t *running;
};

__device__ __forceinline__ int32_t tp1_lim(const Tp1Args &a, int64_t c) {
    const int32_t cap = a.max_depth < kTpMaxTrail ? a.max_depth : kTpMaxTrail;
    return a.limit[c] < cap ? a.limit[c] : cap;
}

// candidate `found` of cube c: its column of path, its length and the G1 cube reached; len <= min(max_depth, 32)
__device__ __forceinline__ void tp1_emit(const Tp1Args &a, int64_t c, int32_t found, const IdaCube &y, uint64_t lo, uint64_t hi, int32_t len) {
    const int64_t col = (int64_t)found * a.stride + c;
    for (int r = 0; r < kTpMaxTrail; ++r)
        if (r < len) a.path[(int64_t)r * a.path_pitch + col] = (uint8_t)ida_nib(lo, hi, r);
    a.cand_length[col] = len;
    tp_store(a.cand + cubie_off(col, a.cand_pitch, a.cand_sh, Cube3::SLOTS), a.cand_pitch, y);
}

__global__ void __launch_bounds__(kWave) k_tp1_init(Tp1Args a) {
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (c >= a.n) return;
    IdaCube x;
    uint32_t status = ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x) ? 0u : TP_ILLEGAL;
    const uint32_t h = tp_h1(x, a.t, status == 0u);
    if (!status && h == 0xFFu) status = TP_ILLEGAL;
    int32_t bound = 0, next = kIdaInf, found = 0;
    if (!status) {
        bound = (int32_t)h;
        if (h == 0u) {                                                     // the root is in G1: candidate 0, of length 0
            tp1_emit(a, c, 0, x, 0, 0, 0);
            found = 1;
            if (found == a.K) status = TP_FULL;
        }
        if (!status && bound > tp1_lim(a, c)) {
            status = TP_EXHAUSTED;
            next = bound;
        }
    }
    a.trail[2 * c] = 0;
    a.trail[2 * c + 1] = 0;
    a.cursor[c] = 0;
    a.depth[c] = 0;
    a.bound[c] = bound;
    a.next[c] = next;
    a.nodes[c] = 0;
    a.found[c] = found;
    a.status[c] = (uint8_t)status;
}

__global__ void __launch_bounds__(kWave) k_tp1_search(Tp1Args a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_moves[kTpRows][16];
    tp_moves_load(s_moves);
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const bool mine = c < a.n && a.status[c] == 0u;
    IdaCube x{};
    uint64_t lo = 0, hi = 0, nodes = 0;
    uint32_t status = 0, cursor = 0;
    int32_t depth = 0, bound = 0, next = kIdaInf, lim = 0, found = 0;
    if (mine) {
        if (!ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x)) status = TP_ILLEGAL;
        lo = a.trail[2 * c];
        hi = a.trail[2 * c + 1];
        cursor = a.cursor[c];
        depth = a.depth[c];
        bound = a.bound[c];
        next = a.next[c];
        nodes = a.nodes[c];
        found = a.found[c];
        lim = tp1_lim(a, c);
        if (depth < 0 || depth >= kTpMaxTrail || cursor > kIdaNoMove || bound > lim || depth > bound || found < 0 || found >= a.K)
            status |= TP_BAD_FRAME;
    }
    for (int r = 0; r < kTpMaxTrail; ++r) {
        uint32_t m = kIdaNoMove;
        if (mine && !status && r < depth) {
            m = ida_nib(lo, hi, r);
            if (m >= kIdaNoMove) {
                status |= TP_BAD_FRAME;
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
            const bool gen = open != 0u, back = !gen && g > 0;
            const uint32_t m = gen ? (uint32_t)__ffs((int)open) - 1u : kIdaNoMove;
            const IdaCube y = ida_move(x, s_moves[gen ? m : back ? (p1 ^ 1u) : kIdaNoMove]);
            const uint32_t h = tp_h1(y, a.t, gen);
            if (gen) {
                ++nodes;
                const int32_t fv = g + 1 + (int32_t)h;
                if (h == 0xFFu) {
                    status = TP_ILLEGAL;
                    run = false;
                } else if (fv > bound) {
                    next = fv < next ? fv : next;
                    cursor = m + 1u;
                } else if (h == 0u) {                                     // a G1 child is never entered
                    cursor = m + 1u;
                    if (g + 1 == bound && !((0xC3u >> m) & 1u)) {         // of this iteration's length, and not ending in a U or D turn
                        uint64_t tlo = lo, thi = hi;
                        ida_nib_set(tlo, thi, g, m);                      // g + 1 <= bound <= 32
                        tp1_emit(a, c, found, y, tlo, thi, g + 1);
                        if (++found == a.K) {
                            status = TP_FULL;
                            run = false;
                        }
                    }
                } else {                                                  // fv <= bound and h >= 1: g + 1 < 32
                    x = y;
                    ida_nib_set(lo, hi, g, m);
                    depth = g + 1;
                    cursor = 0;
                }
            } else if (back) {
                x = y;
                cursor = p1 + 1u;
                depth = g - 1;
            } else if (next > lim) {
                status = TP_EXHAUSTED;
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
        a.found[c] = found;
        a.status[c] = (uint8_t)status;
    }
    const unsigned long long bal = __ballot(run);
    if (threadIdx.x == 0 && bal) atomicAdd(a.running, (uint32_t)__popcll(bal));
}

struct Tp2Args {
    const uint8_t *cubies;
    int64_t n, pitch;
    int sh;
    TpTables t;
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

// min(limit, max_depth, floor + 32): the trail holds 32 generators
__device__ __forceinline__ int32_t tp2_lim(const Tp2Args &a, int64_t c, int32_t f) {
    int32_t lim = a.limit[c] < a.max_depth ? a.limit[c] : a.max_depth;
    return lim < f + kTpMaxTrail ? lim : f + kTpMaxTrail;
}

// the last two actions of the prefix (12: none); false: floor outside 0..max_depth or one of them is no action
__device__ __forceinline__ bool tp2_prefix(const Tp2Args &a, int64_t c, int32_t f, uint32_t &pre1, uint32_t &pre2) {
    pre1 = pre2 = kIdaNoMove;
    if (f < 0 || f > a.max_depth) return false;
    if (f >= 1) pre1 = a.path[(int64_t)(f - 1) * a.path_pitch + c];
    if (f >= 2) pre2 = a.path[(int64_t)(f - 2) * a.path_pitch + c];
    return (f < 1 || pre1 < kIdaNoMove) && (f < 2 || pre2 < kIdaNoMove);
}

__global__ void __launch_bounds__(kWave) k_tp2_init(Tp2Args a) {
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (c >= a.n) return;
    IdaCube x;
    uint32_t status = ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x) ? 0u : TP_ILLEGAL;
    const int32_t f = a.floor ? a.floor[c] : 0;
    uint32_t pre1, pre2;
    if (!tp2_prefix(a, c, f, pre1, pre2)) status |= TP_BAD_FRAME;
    if (!status && !tp_in_g1(x)) status = TP_OUTSIDE;
    const uint32_t h = tp_h2(x, a.t, status == 0u);
    if (!status && h == 0xFFu) status = TP_ILLEGAL;
    int32_t depth = 0, bound = 0, next = kIdaInf;
    if (!status) {
        depth = f;
        bound = f + (int32_t)h;
        if (bound > tp2_lim(a, c, f)) {                                    // before the goal test: an empty slot is skipped here
            status = TP_EXHAUSTED;
            next = bound;
        } else if (h == 0u) {
            status = TP_SOLVED;
        }
    }
    a.trail[2 * c] = 0;
    a.trail[2 * c + 1] = 0;
    a.cursor[c] = 0;
    a.depth[c] = depth;
    a.bound[c] = bound;
    a.next[c] = next;
    a.nodes[c] = 0;
    a.status[c] = (uint8_t)status;
}

__global__ void __launch_bounds__(kWave) k_tp2_search(Tp2Args a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_moves[kTpRows][16];
    tp_moves_load(s_moves);
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const bool mine = c < a.n && a.status[c] == 0u;
    IdaCube x{};
    uint64_t lo = 0, hi = 0, nodes = 0;
    uint32_t status = 0, cursor = 0, pre1 = kIdaNoMove, pre2 = kIdaNoMove;
    int32_t f = 0, g = 0, k = 0, bound = 0, next = kIdaInf, lim = 0;
    if (mine) {
        if (!ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x)) status = TP_ILLEGAL;
        f = a.floor ? a.floor[c] : 0;
        if (!tp2_prefix(a, c, f, pre1, pre2)) {
            status |= TP_BAD_FRAME;
            f = 0;
        }
        if (!status && !tp_in_g1(x)) status = TP_OUTSIDE;
        lo = a.trail[2 * c];
        hi = a.trail[2 * c + 1];
        cursor = a.cursor[c];
        g = a.depth[c];
        bound = a.bound[c];
        next = a.next[c];
        nodes = a.nodes[c];
        lim = tp2_lim(a, c, f);
        if (g < f || g > a.max_depth || g > bound || cursor > 8u || bound > lim) status |= TP_BAD_FRAME;
    }
    int32_t sum = f;
    for (int r = 0; r < kTpMaxTrail; ++r) {                                // the current node: generators until their costs reach g
        uint32_t row = kIdaNoMove;
        if (mine && !status && sum < g) {
            const uint32_t j = ida_nib(lo, hi, r);
            if (j >= 8u) {
                status |= TP_BAD_FRAME;
            } else {
                row = tp_gen_row(j);
                sum += 1 + (int32_t)tp_gen_half(j);
                ++k;
            }
        }
        x = ida_move(x, s_moves[row]);
    }
    if (mine && !status && sum != g) status |= TP_BAD_FRAME;
    bool run = mine && !status;
    for (int64_t step = 0; step < a.max_steps; ++step) {                  // the only loop
        if (__ballot(run) == 0ull) break;
        if (run) {
            const uint32_t j1 = k >= 1 ? ida_nib(lo, hi, k - 1) : 0u;
            uint32_t p1 = pre1, p2 = pre2;                                // the last two ACTIONS of prefix + generators
            if (k >= 1) {
                p1 = tp_gen_action(j1);
                p2 = tp_gen_half(j1) ? p1 : k >= 2 ? tp_gen_action(ida_nib(lo, hi, k - 2)) : pre1;
            }
            const uint32_t open = tp_gen_allowed(ida_allowed(p2, p1)) & (0xFFu << cursor) & 0xFFu;
            const bool gen = open != 0u, back = !gen && k > 0;
            const uint32_t j = gen ? (uint32_t)__ffs((int)open) - 1u : 8u;
            const IdaCube y = ida_move(x, s_moves[gen ? tp_gen_row(j) : back ? tp_gen_back(j1) : kIdaNoMove]);
            const uint32_t h = tp_h2(y, a.t, gen);
            if (gen) {
                ++nodes;
                const int32_t w = 1 + (int32_t)tp_gen_half(j), fv = g + w + (int32_t)h;
                if (h == 0xFFu) {
                    status = TP_ILLEGAL;
                    run = false;
                } else if (fv > bound) {
                    next = fv < next ? fv : next;
                    cursor = j + 1u;
                } else {                                                  // fv <= bound <= floor + 32: k < 32
                    x = y;
                    ida_nib_set(lo, hi, k, j);
                    ++k;
                    g += w;
                    cursor = 0;
                    if (h == 0u) {
                        status = TP_SOLVED;
                        run = false;
                    }
                }
            } else if (back) {
                x = y;
                cursor = j1 + 1u;
                --k;
                g -= 1 + (int32_t)tp_gen_half(j1);
            } else if (next > lim) {
                status = TP_EXHAUSTED;
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
        a.depth[c] = g;
        a.bound[c] = bound;
        a.next[c] = next;
        a.nodes[c] = nodes;
        a.status[c] = (uint8_t)status;
        if (status == TP_SOLVED) {
            int32_t r = f;
            for (int i = 0; i < kTpMaxTrail; ++i)
                if (i < k) {
                    const uint32_t j = ida_nib(lo, hi, i), act = tp_gen_action(j);
                    for (uint32_t t = 0; t <= tp_gen_half(j); ++t)
                        if (r < a.max_depth) a.path[(int64_t)r++ * a.path_pitch + c] = (uint8_t)act;   // r < g <= max_depth; the guard stays
                }
        }
    }
    const unsigned long long bal = __ballot(run);
    if (threadIdx.x == 0 && bal) atomicAdd(a.running, (uint32_t)__popcll(bal));
}

int tp_which_arg(const char *fn, int which) {
    return which < 0 || which > 3 ? fail(RC_EINVAL, "%s: which must be in 0..3", fn) : RC_OK;
}

int tp_tables_arg(const char *fn, int phase, const uint8_t *ta, int64_t bytes_a, const uint8_t *tb, int64_t bytes_b, TpTables &t) {
    const int w = phase == 1 ? 0 : 2;
    if (!ta || !aligned16(ta)) return fail(RC_EINVAL, "%s: table_a is NULL or not 16-byte aligned", fn);
    if (bytes_a < (int64_t)kTpN[w]) return fail(RC_EINVAL, "%s: bytes_a is smaller than tp_table_bytes(%s)", fn, w ? "2" : "0");
    if (!tb || !aligned16(tb)) return fail(RC_EINVAL, "%s: table_b is NULL or not 16-byte aligned", fn);
    if (bytes_b < (int64_t)kTpN[w + 1]) return fail(RC_EINVAL, "%s: bytes_b is smaller than tp_table_bytes(%s)", fn, w ? "3" : "1");
    t = TpTables{ta, tb};
    return RC_OK;
}

int tp1_args(const char *fn, const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *ta, int64_t bytes_a, const uint8_t *tb,
             int64_t bytes_b, const int32_t *limit, int K, int64_t stride, uint8_t *path, int max_depth, int64_t path_pitch,
             int32_t *cand_length, uint8_t *cand, int64_t cand_pitch, uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound,
             int32_t *next, uint64_t *nodes, int32_t *found, uint8_t *status, Tp1Args &a) {
    const auto bad = [fn](const char *what) { return fail(RC_EINVAL, "%s: %s", fn, what); };
    if (n < 0) return bad("n is negative");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    TpTables t{};
    if (int rc = tp_tables_arg(fn, 1, ta, bytes_a, tb, bytes_b, t)) return rc;
    if (!limit || !aligned16(limit)) return bad("limit is NULL or not 16-byte aligned");
    if (K < 1 || K > kTpMaxK) return bad("candidates must be in 1..4096");
    if (stride < n || stride < 16 || (stride & 15) != 0 || stride > ((int64_t)1 << 31) / K)
        return bad("stride: need stride % 16 == 0, stride >= max(n, 16) and candidates * stride <= 2^31");
    const int64_t cols = (int64_t)K * stride;
    if (!path || !aligned16(path)) return bad("path is NULL or not 16-byte aligned");
    if (max_depth < 1 || max_depth > kTpMaxDepth) return bad("max_depth must be in 1..48");
    if (path_pitch < cols || (path_pitch & 15) != 0) return bad("path_pitch: need path_pitch % 16 == 0 and path_pitch >= candidates * stride");
    if (!cand_length || !aligned16(cand_length)) return bad("cand_length is NULL or not 16-byte aligned");
    if (!cand || !aligned16(cand)) return bad("cand_cubies is NULL or not 16-byte aligned");
    const int cand_sh = tile_shift(cand_pitch, cols, Cube3::SLOTS);
    if (cand_sh < 0) return bad("cand_pitch: need pitch % 16 == 0 and pitch >= candidates * stride, or a power-of-two tile >= 512");
    if (!trail || !aligned16(trail)) return bad("trail is NULL or not 16-byte aligned");
    if (!cursor || !aligned16(cursor)) return bad("cursor is NULL or not 16-byte aligned");
    if (!depth || !aligned16(depth)) return bad("depth is NULL or not 16-byte aligned");
    if (!bound || !aligned16(bound)) return bad("bound is NULL or not 16-byte aligned");
    if (!next || !aligned16(next)) return bad("next is NULL or not 16-byte aligned");
    if (!nodes || !aligned16(nodes)) return bad("nodes is NULL or not 16-byte aligned");
    if (!found || !aligned16(found)) return bad("found is NULL or not 16-byte aligned");
    if (!status || !aligned16(status)) return bad("status is NULL or not 16-byte aligned");
    a = Tp1Args{cubies, n, cubie_pitch, sh, t, limit, K, stride, path, max_depth, path_pitch, cand_length, cand, cand_pitch, cand_sh,
                trail, cursor, depth, bound, next, nodes, found, status, 0, nullptr};
    return RC_OK;
}

int tp2_args(const char *fn, const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *ta, int64_t bytes_a, const uint8_t *tb,
             int64_t bytes_b, uint8_t *path, int max_depth, int64_t path_pitch, const int32_t *floor, const int32_t *limit, uint64_t *trail,
             uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next, uint64_t *nodes, uint8_t *status, Tp2Args &a) {
    const auto bad = [fn](const char *what) { return fail(RC_EINVAL, "%s: %s", fn, what); };
    if (n < 0) return bad("n is negative");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    TpTables t{};
    if (int rc = tp_tables_arg(fn, 2, ta, bytes_a, tb, bytes_b, t)) return rc;
    if (!path || !aligned16(path)) return bad("path is NULL or not 16-byte aligned");
    if (max_depth < 1 || max_depth > kTpMaxDepth) return bad("max_depth must be in 1..48");
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
    a = Tp2Args{cubies, n, cubie_pitch, sh, t, path, max_depth, path_pitch, floor, limit, trail, cursor, depth, bound, next, nodes, status, 0, nullptr};
    return RC_OK;
}

template <class F>
int by_which(int which, F &&f) {
    switch (which) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 3>{});
    }
}

template <class Args, class Kernel>
int tp_launch(Kernel kernel, Args &a, int64_t max_steps, uint32_t *running, hipStream_t st) {
    const int64_t blocks = ceil_div(a.n, kWave);
    RC_GRID(blocks);
    if (running) {
        a.max_steps = max_steps;
        a.running = running;
        hipLaunchKernelGGL(k_zero32, dim3(1), dim3(1), 0, st, running);
        RC_HIP(RC_EHIP, hipGetLastError());
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kWave), 0, st, a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

int tp_steps_arg(const char *fn, int64_t max_steps, const uint32_t *running) {
    if (max_steps < 1 || max_steps > kTpMaxSteps) return fail(RC_EINVAL, "%s: max_steps must be in 1..tp_max_steps()", fn);
    if (!running || !aligned16(running)) return fail(RC_EINVAL, "%s: running is NULL or not 16-byte aligned", fn);
    return RC_OK;
}

}  // namespace

extern "C" {

int64_t tp_table_bytes(int which) { return which < 0 || which > 3 ? -1 : (int64_t)kTpN[which]; }

int64_t tp_max_steps(void) { return kTpMaxSteps; }

int tp_generators(int phase, uint8_t *gens, uint8_t *cost, int *count) {
    if (phase != 1 && phase != 2) return fail(RC_EINVAL, "tp_generators: phase must be 1 or 2");
    const int stage = phase == 1 ? 0 : 2, ngen = Cube3::chain_ngen[stage];
    for (int g = 0; g < 12; ++g) {
        const int code = Cube3::chain_gen[stage][g];
        const bool have = g < ngen, half = have && (code >> 4);
        if (gens) {
            gens[2 * g] = have ? (uint8_t)(code & 15) : 0xFFu;
            gens[2 * g + 1] = half ? (uint8_t)(code & 15) : 0xFFu;
        }
        if (cost) cost[g] = have ? (uint8_t)(half ? 2 : 1) : 0u;
    }
    if (count) *count = ngen;
    return RC_OK;
}

int tp_build_begin(uint8_t *table, int64_t bytes, int which, void *stream) {
    RC_NEED_INIT();
    if (int rc = tp_which_arg("tp_build_begin", which)) return rc;
    if (int rc = table_arg("tp_build_begin", table, bytes, kTpN[which], "tp_table_bytes(which)")) return rc;
    const uint32_t goal = which == 0 ? kChainSliceHome * 2187u : which == 1 ? kChainSliceHome * 2048u : 0u;
    hipLaunchKernelGGL(k_tp_fill, dim3((kTpN[which] + 255u) / 256u), dim3(256), 0, S(stream), table, kTpN[which], goal);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

int tp_build_level(uint8_t *table, int64_t bytes, int which, int depth, uint32_t *count, void *stream) {
    RC_NEED_INIT();
    if (int rc = tp_which_arg("tp_build_level", which)) return rc;
    if (int rc = table_arg("tp_build_level", table, bytes, kTpN[which], "tp_table_bytes(which)")) return rc;
    return by_which(which, [&](auto wc) {
        constexpr int W = decltype(wc)::value;
        return table_build_level<(W >= 2)>("tp_build_level", table, TpLevels<W>{}, depth, count, S(stream), RC_EHIP);
    });
}

int tp_index(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, int which, uint32_t *index, void *stream) {
    RC_NEED_INIT();
    const auto bad = [](const char *what) { return fail(RC_EINVAL, "tp_index: %s", what); };
    if (int rc = tp_which_arg("tp_index", which)) return rc;
    if (n < 0) return bad("n is negative");
    if (!cubies || !aligned16(cubies)) return bad("cubies is NULL or not 16-byte aligned");
    const int sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return bad("cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
    if (!index || !aligned16(index)) return bad("index is NULL or not 16-byte aligned");
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, 256);
    RC_GRID(blocks);
    return by_which(which, [&](auto wc) {
        hipLaunchKernelGGL(k_tp_index<decltype(wc)::value>, dim3((unsigned)blocks), dim3(256), 0, S(stream), cubies, n, cubie_pitch, sh, index);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

int tp_phase1_init(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                   int64_t bytes_b, const int32_t *limit, int candidates, int64_t stride, uint8_t *path, int max_depth, int64_t path_pitch,
                   int32_t *cand_length, uint8_t *cand_cubies, int64_t cand_pitch, uint64_t *trail, uint8_t *cursor, int32_t *depth,
                   int32_t *bound, int32_t *next, uint64_t *nodes, int32_t *found, uint8_t *status, void *stream) {
    RC_NEED_INIT();
    Tp1Args a;
    if (int rc = tp1_args("tp_phase1_init", cubies, n, cubie_pitch, table_a, bytes_a, table_b, bytes_b, limit, candidates, stride, path, max_depth,
                          path_pitch, cand_length, cand_cubies, cand_pitch, trail, cursor, depth, bound, next, nodes, found, status, a))
        return rc;
    if (n == 0) return RC_OK;
    return tp_launch(k_tp1_init, a, 0, nullptr, S(stream));
}

int tp_phase1_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                     int64_t bytes_b, const int32_t *limit, int candidates, int64_t stride, uint8_t *path, int max_depth, int64_t path_pitch,
                     int32_t *cand_length, uint8_t *cand_cubies, int64_t cand_pitch, uint64_t *trail, uint8_t *cursor, int32_t *depth,
                     int32_t *bound, int32_t *next, uint64_t *nodes, int32_t *found, uint8_t *status, int64_t max_steps, uint32_t *running,
                     void *stream) {
    RC_NEED_INIT();
    Tp1Args a;
    if (int rc = tp1_args("tp_phase1_search", cubies, n, cubie_pitch, table_a, bytes_a, table_b, bytes_b, limit, candidates, stride, path,
                          max_depth, path_pitch, cand_length, cand_cubies, cand_pitch, trail, cursor, depth, bound, next, nodes, found, status, a))
        return rc;
    if (int rc = tp_steps_arg("tp_phase1_search", max_steps, running)) return rc;
    if (n == 0) return RC_OK;
    return tp_launch(k_tp1_search, a, max_steps, running, S(stream));
}

int tp_phase2_init(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                   int64_t bytes_b, uint8_t *path, int max_depth, int64_t path_pitch, const int32_t *floor, const int32_t *limit,
                   uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next, uint64_t *nodes, uint8_t *status,
                   void *stream) {
    RC_NEED_INIT();
    Tp2Args a;
    if (int rc = tp2_args("tp_phase2_init", cubies, n, cubie_pitch, table_a, bytes_a, table_b, bytes_b, path, max_depth, path_pitch, floor, limit,
                          trail, cursor, depth, bound, next, nodes, status, a))
        return rc;
    if (n == 0) return RC_OK;
    return tp_launch(k_tp2_init, a, 0, nullptr, S(stream));
}

int tp_phase2_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                     int64_t bytes_b, uint8_t *path, int max_depth, int64_t path_pitch, const int32_t *floor, const int32_t *limit,
                     uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next, uint64_t *nodes, uint8_t *status,
                     int64_t max_steps, uint32_t *running, void *stream) {
    RC_NEED_INIT();
    Tp2Args a;
    if (int rc = tp2_args("tp_phase2_search", cubies, n, cubie_pitch, table_a, bytes_a, table_b, bytes_b, path, max_depth, path_pitch, floor,
                          limit, trail, cursor, depth, bound, next, nodes, status, a))
        return rc;
    if (int rc = tp_steps_arg("tp_phase2_search", max_steps, running)) return rc;
    if (n == 0) return RC_OK;
    return tp_launch(k_tp2_search, a, max_steps, running, S(stream));
}

}  // extern "C"
