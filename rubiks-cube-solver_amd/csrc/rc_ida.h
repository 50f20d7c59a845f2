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
