// rc_ida.h -- cost-bounded depth-first search, one lane per cube, no node memory: the ida_* entry points (include/rubikhip.h
// "Iterative-deepening A*", DESIGN.md "IDA*") and the tp_* entry points (include/rubikhip.h "Two-phase", DESIGN.md "Two-phase").  A part
// of rubikhip.hip's translation unit, after rc_edge.h (EdgeSet, edge_table_arg) and rc_chain.h (load_cubie_bytes, TpLevels).  3x3x3 only.
//   the core        move rows (move_row, MoveTable, moves_load), the cube (IdaCube, ida_move), the frame (SearchFrame, IdaLane,
//                   frame_load, frame_store), the trail replayed (ida_replay), the state machine (ida_passes) and the host's argument
//                   checks and launcher -- each written once; a two-phase search is a policy type (Tp1Search, Tp2Search).  k_ida_search
//                   keeps its own copy of the pass loop: through ida_passes it measured 2.8 % slower under the corner table
//                   (DESIGN.md "IDA*"), so whoever changes a pass changes it there and in ida_passes
//   k_ida_init      legality, the prefix replayed, the first bound, the frame's first contents
//   k_ida_search    Korf's IDA* under the maximum of the corner table and up to four edge tables (read through rc_table.h table_at)
//   k_tp1_init / k_tp1_search   Kociemba's phase 1 under max(twist-slice, flip-slice): up to K G1 candidates per cube are emitted
//                               (path column, length, cubie rows), the search never enters G1
//   k_tp2_init / k_tp2_search   phase 2, one lane per candidate column, under max(corner-slice, edge-slice): stage 2's generators with
//                               a half turn costing 2; the first goal ends the lane
//   k_cg_product / k_cg_inverse / k_cg_random / k_cg_invert_actions   the cg_* entry points (include/rubikhip.h "Cube group"), at the
//                               end of the file: whole cubes multiplied, inverted and drawn uniformly, on IdaCube; both cube sizes
// A search kernel makes at most max_steps passes per cube; a pass applies ONE move to the cube in registers -- the next canonical
// child, or the inverse of the last move to go back a level -- then ranks, reads the tables and compares.  The cube lives in five
// registers of cubie bytes (IdaCube); a move is a byte gather (v_perm_b32) whose selectors come from a row of s_moves in LDS (13 rows:
// 12 actions and the identity; the tp searches add the half turns F2, R2, B2, L2, so a phase-2 generator is one gather): the move
// varies by lane, so nothing here is a compile-time gather and nothing is a switch.  The trail lives in two 64-bit registers of
// nibbles.  No indexed array, no scratch.
#pragma once

namespace {

constexpr int kIdaTrail = 32;                                               // nibbles in the two words of a trail
constexpr int kIdaMaxDepth = kIdaTrail, kIdaMaxEdge = 4;
constexpr uint32_t kIdaNoMove = 12u;
constexpr int32_t kIdaInf = 0x7FFFFFFF;
constexpr int64_t kIdaMaxSteps = (int64_t)1 << 14;                          // DESIGN.md "IDA*": 0.83 s a launch at 2^20 cubes, three tables
constexpr int kTpMaxDepth = 48, kTpMaxTrail = kIdaTrail, kTpRows = 17, kTpMaxK = 4096;
constexpr int64_t kTpMaxSteps = (int64_t)1 << 17;                           // DESIGN.md "Two-phase": 0.73 | 0.89 s a launch at 2^20 lanes
static_assert(TP_SOLVED == IDA_SOLVED && TP_EXHAUSTED == IDA_EXHAUSTED && TP_ILLEGAL == IDA_ILLEGAL && TP_BAD_FRAME == IDA_BAD_FRAME,
              "the core below sets the IDA_ codes for both families");

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

// ---------------------------------------------------------------------------------------------------------------- move rows
// One row of the move table: 0, 1 the corner selectors; 2, 3 the twists in the high nibbles; 4 + 2j, 5 + 2j the selectors of edge
// dword j from (e1, e0) and from e2 (0x0c: a zero byte); 10..12 the flips.
constexpr void move_row(uint32_t (&w)[16], const uint8_t *csrc, const uint8_t *ctwist, const uint8_t *esrc, const uint8_t *eflip) {
    for (int q = 0; q < 8; ++q) {
        w[q >> 2] |= (uint32_t)csrc[q] << (8 * (q & 3));
        w[2 + (q >> 2)] |= ((uint32_t)ctwist[q] << 4) << (8 * (q & 3));
    }
    for (int q = 0; q < 12; ++q) {
        const uint32_t s = esrc[q];
        w[4 + 2 * (q >> 2)] |= (s < 8u ? s : 0x0cu) << (8 * (q & 3));
        w[5 + 2 * (q >> 2)] |= (s < 8u ? 0x0cu : s - 8u) << (8 * (q & 3));
        w[10 + (q >> 2)] |= (uint32_t)eflip[q] << (8 * (q & 3));
    }
}

// Rows 0..11 the actions, 12 the identity; R = 17 adds 13..16 = F2, R2, B2, L2 (among stage 3's U2 F2 R2 D2 B2 L2)
template <int R>
struct MoveTable {
    uint32_t w[R][16];
    constexpr MoveTable() : w{} {
        const uint8_t same[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, none[12] = {}, half[4] = {1, 2, 4, 5};
        for (int a = 0; a < 12; ++a) move_row(w[a], Cube3::cmove_src[a], Cube3::cmove_twist[a], Cube3::emove_src[a], Cube3::emove_flip[a]);
        move_row(w[12], same, none, same, none);
        for (int k = 0; k < R - 13; ++k) {
            const ChainGen g = chain_gen(3, half[k]);
            move_row(w[13 + k], g.csrc, g.ctw, g.esrc, g.eflip);
        }
    }
};
__constant__ MoveTable<13> c_ida_moves{};
__constant__ MoveTable<kTpRows> c_tp_moves{};

template <int R>
__device__ __forceinline__ void moves_load(uint32_t (*s_moves)[16], const uint32_t (&w)[R][16]) {
    for (uint32_t i = threadIdx.x; i < (uint32_t)R * 16u; i += blockDim.x) s_moves[i >> 4][i & 15u] = w[i >> 4][i & 15u];
    __syncthreads();
}

// ----------------------------------------------------------------------------------------------------------------- the cube
struct IdaCube {
    uint32_t c0, c1;       // byte q: corner slot q, piece | ori << 4
    uint32_t e0, e1, e2;   // byte q: edge slot q, the cubie byte piece * 2 + ori
};

// the corner bytes after two ori were added in the high nibbles: ori 3, 4 -> 0, 1
__device__ __forceinline__ uint32_t ida_twist(uint32_t v) { return v - (((v + 0x10101010u) >> 6) & 0x01010101u) * 0x30u; }

__device__ __forceinline__ IdaCube ida_move(const IdaCube &x, const uint32_t *row) {
    const u32x4 a = *reinterpret_cast<const u32x4 *>(row), b = *reinterpret_cast<const u32x4 *>(row + 4),
                c = *reinterpret_cast<const u32x4 *>(row + 8);
    const uint32_t f2 = row[12];
    IdaCube y;
    const auto twist = ida_twist;
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

__device__ __forceinline__ uint32_t ida_nib(uint64_t lo, uint64_t hi, int i) {   // i in 0..31
    return (uint32_t)((i & 16 ? hi : lo) >> (4 * (i & 15))) & 15u;
}
__device__ __forceinline__ void ida_nib_set(uint64_t &lo, uint64_t &hi, int i, uint32_t v) {
    const uint64_t keep = ~(15ull << (4 * (i & 15))), put = (uint64_t)v << (4 * (i & 15));
    if (i & 16) hi = (hi & keep) | put;
    else lo = (lo & keep) | put;
}

// ---------------------------------------------------------------------------------------------------------------- the frame
// The caller's arrays, one entry per lane (trail: two), and the two arguments of a search launch; a part of every kernel's arguments.
struct SearchFrame {
    uint64_t *trail;
    uint8_t *cursor;
    int32_t *depth, *bound, *next;
    uint64_t *nodes;
    uint8_t *status;
    int64_t max_steps;
    uint32_t *running;
};

// One lane's frame in registers.  k, the nibbles in the trail, is not stored: where every generator costs 1 it is depth itself,
// otherwise ida_replay counts it.
struct IdaLane {
    uint64_t lo = 0, hi = 0, nodes = 0;
    uint32_t cursor = 0, status = 0;
    int32_t depth = 0, bound = 0, next = kIdaInf, k = 0;
};

__device__ __forceinline__ IdaLane frame_load(const SearchFrame &fr, int64_t c) {   // of a lane whose stored status is 0
    return IdaLane{fr.trail[2 * c], fr.trail[2 * c + 1], fr.nodes[c], fr.cursor[c], 0u, fr.depth[c], fr.bound[c], fr.next[c], 0};
}

__device__ __forceinline__ void frame_store(const SearchFrame &fr, int64_t c, const IdaLane &l) {
    fr.trail[2 * c] = l.lo;
    fr.trail[2 * c + 1] = l.hi;
    fr.cursor[c] = (uint8_t)l.cursor;
    fr.depth[c] = l.depth;
    fr.bound[c] = l.bound;
    fr.next[c] = l.next;
    fr.nodes[c] = l.nodes;
    fr.status[c] = (uint8_t)l.status;
}

// A frame's first contents beside its status: nothing spent, the first bound f + h.  first_over: that bound is beyond the limit.
__device__ __forceinline__ void first_bound(IdaLane &l, int32_t f, uint32_t h) {
    l.depth = f;
    l.bound = f + (int32_t)h;
}
__device__ __forceinline__ bool first_over(IdaLane &l, int32_t lim) {
    if (l.bound <= lim) return false;
    l.status = IDA_EXHAUSTED;
    l.next = l.bound;
    return true;
}

// -------------------------------------------------------------------------------------------------------- the state machine
// A search is a policy type P.  What it says of its generators (the nibbles of the trail, the bits of the open mask):
//   NGEN, NONE           their number; the `last` of an empty trail
//   UNIT                 every generator costs 1: depth is the trail's length, and no second count is kept
//   row(j), undo(j)      the rows of s_moves that apply generator j and take it back
//   cost(j)              1, or 2 for a half turn
//   allowed(l, k, last)  the generators that may follow a trail of k nibbles ending in `last`
// and of the search:
//   floor                the trail length below which it does not go back
//   h(y, live)           the heuristic, 0xFF for a cube no table knows; !live: no table is read
//   enters(h)            an admissible child (f <= bound) becomes the current node; otherwise it is passed over after
//   emit(l, y, j)        -> 0 or the status that ends the lane
//   goal(y, h)           the child just entered ends the lane as SOLVED

// The current node: the root moved along the trail, generators until their costs reach l.depth from `from`.  A nibble that is no
// generator, or costs that step over l.depth, make a bad frame.  Every lane makes every move: a lane with nothing to replay, the identity.
template <class P>
__device__ __forceinline__ void ida_replay(uint32_t (*s_moves)[16], IdaCube &x, IdaLane &l, bool live, int32_t from) {
    int32_t sum = from;
    for (int r = 0; r < kIdaTrail; ++r) {
        uint32_t row = kIdaNoMove;
        if (live && !l.status && (P::UNIT ? r < l.depth : sum < l.depth)) {
            const uint32_t j = ida_nib(l.lo, l.hi, r);
            if (j >= P::NGEN) {
                l.status |= IDA_BAD_FRAME;
            } else {
                row = P::row(j);
                sum += P::cost(j);
                ++l.k;
            }
        }
        x = ida_move(x, s_moves[row]);
    }
    if (!P::UNIT && live && !l.status && sum != l.depth) l.status |= IDA_BAD_FRAME;
}

// At most fr.max_steps passes of the lanes that run, then their count added to *fr.running.
template <class P>
__device__ __forceinline__ void ida_passes(P &p, uint32_t (*s_moves)[16], const SearchFrame &fr, IdaCube &x, IdaLane &l, int32_t lim, bool run) {
    constexpr uint32_t ALL = (1u << P::NGEN) - 1u;
    const int32_t steps = __builtin_amdgcn_readfirstlane((int32_t)fr.max_steps);   // <= 2^17, one value per wave
    for (int32_t step = 0; step < steps; ++step) {                 // the only loop: whatever the tables hold, it ends
        if (__ballot(run) == 0ull) break;
        if (run) {
            const int32_t g = l.depth, k = P::UNIT ? g : l.k;
            const uint32_t last = k >= 1 ? ida_nib(l.lo, l.hi, k - 1) : P::NONE;
            const uint32_t open = p.allowed(l, k, last) & (ALL << l.cursor) & ALL;
            const bool gen = open != 0u, back = !gen && k > p.floor;
            const uint32_t m = gen ? (uint32_t)__ffs((int)open) - 1u : P::NGEN;
            const IdaCube y = ida_move(x, s_moves[gen ? P::row(m) : back ? P::undo(last) : kIdaNoMove]);
            const uint32_t h = p.h(y, gen);
            if (gen) {
                ++l.nodes;
                const int32_t w = P::cost(m), fv = g + w + (int32_t)h;
                if (h == 0xFFu) {
                    l.status = IDA_ILLEGAL;
                    run = false;
                } else if (fv > l.bound) {
                    l.next = fv < l.next ? fv : l.next;
                    l.cursor = m + 1u;
                } else if (!p.enters(h)) {
                    l.cursor = m + 1u;
                    if (const uint32_t over = p.emit(l, y, m)) {
                        l.status = over;
                        run = false;
                    }
                } else {                                                  // fv <= bound <= the limit: nibble k and row g exist
                    x = y;
                    ida_nib_set(l.lo, l.hi, k, m);
                    l.k = k + 1;
                    l.depth = g + w;
                    l.cursor = 0;
                    l.status = p.goal(y, h) ? IDA_SOLVED : 0u;           // a running lane's status is 0
                    run = !l.status;
                }
            } else if (back) {
                x = y;
                l.cursor = last + 1u;
                l.k = k - 1;
                l.depth = g - P::cost(last);
            } else if (l.next > lim) {                                    // the iteration is exhausted
                l.status = IDA_EXHAUSTED;
                run = false;
            } else {
                l.bound = l.next;
                l.next = kIdaInf;
                l.cursor = 0;
            }
        }
    }
    const unsigned long long bal = __ballot(run);
    if (threadIdx.x == 0 && bal) atomicAdd(fr.running, (uint32_t)__popcll(bal));
}

// ------------------------------------------------------------------------------------------------- host: arguments, launches
int cubie_arg(const char *fn, const uint8_t *cubies, int64_t n, int64_t cubie_pitch, int &sh) {
    if (n < 0) return fail(RC_EINVAL, "%s: n is negative", fn);
    if (!cubies || !aligned16(cubies)) return fail(RC_EINVAL, "%s: cubies is NULL or not 16-byte aligned", fn);
    sh = tile_shift(cubie_pitch, n, Cube3::SLOTS);
    if (sh < 0) return fail(RC_EINVAL, "%s: cubie_pitch: need pitch %% 16 == 0 and pitch >= n, or a power-of-two tile >= 512", fn);
    return RC_OK;
}

// cap: 32 or 48 rows; cols: the columns path must hold, and how the message names them
int path_arg(const char *fn, const uint8_t *path, int max_depth, int64_t path_pitch, int cap, int64_t cols, const char *cols_name) {
    if (!path || !aligned16(path)) return fail(RC_EINVAL, "%s: path is NULL or not 16-byte aligned", fn);
    if (max_depth < 1 || max_depth > cap) return fail(RC_EINVAL, "%s: max_depth must be in 1..%s", fn, cap == kIdaMaxDepth ? "32" : "48");
    if (path_pitch < cols || (path_pitch & 15) != 0)
        return fail(RC_EINVAL, "%s: path_pitch: need path_pitch %% 16 == 0 and path_pitch >= %s", fn, cols_name);
    return RC_OK;
}

// found: phase 1's extra field (NULL: the search has none), checked where its argument stands
int frame_arg(const char *fn, const SearchFrame &fr, const int32_t *const *found = nullptr) {
    const auto need = [fn](const void *p, const char *name) {
        return p && aligned16(p) ? RC_OK : fail(RC_EINVAL, "%s: %s is NULL or not 16-byte aligned", fn, name);
    };
    if (int rc = need(fr.trail, "trail")) return rc;
    if (int rc = need(fr.cursor, "cursor")) return rc;
    if (int rc = need(fr.depth, "depth")) return rc;
    if (int rc = need(fr.bound, "bound")) return rc;
    if (int rc = need(fr.next, "next")) return rc;
    if (int rc = need(fr.nodes, "nodes")) return rc;
    if (found)
        if (int rc = need(*found, "found")) return rc;
    return need(fr.status, "status");
}

int steps_arg(const char *fn, const SearchFrame &fr, int64_t cap, const char *cap_name) {
    if (fr.max_steps < 1 || fr.max_steps > cap) return fail(RC_EINVAL, "%s: max_steps must be in 1..%s", fn, cap_name);
    if (!fr.running || !aligned16(fr.running)) return fail(RC_EINVAL, "%s: running is NULL or not 16-byte aligned", fn);
    return RC_OK;
}

// One lane per cube in blocks of a wave; a search (a.fr.running set) zeroes its counter in front of the kernel
template <class Args, class Kernel>
int ida_launch(Kernel kernel, const Args &a, hipStream_t st) {
    if (a.n == 0) return RC_OK;
    const int64_t blocks = ceil_div(a.n, kWave);
    RC_GRID(blocks);
    if (a.fr.running) {
        hipLaunchKernelGGL(k_zero32, dim3(1), dim3(1), 0, st, a.fr.running);
        RC_HIP(RC_EHIP, hipGetLastError());
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kWave), 0, st, a);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

// ======================================================================================================================= IDA*
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

struct IdaArgs {
    const uint8_t *cubies;
    int64_t n, pitch;
    int sh;
    IdaTables t;
    uint8_t *path;
    int32_t max_depth;
    int64_t path_pitch;
    const int32_t *floor, *limit;
    SearchFrame fr;
};

__global__ void __launch_bounds__(kWave) k_ida_init(IdaArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_moves[13][16];
    moves_load(s_moves, c_ida_moves.w);
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (c >= a.n) return;
    IdaCube x;
    IdaLane l;
    l.status = ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x) ? 0u : IDA_ILLEGAL;
    const int32_t f = a.floor ? a.floor[c] : 0;
    if (f < 0 || f > a.max_depth) l.status |= IDA_BAD_FRAME;
    uint64_t lo = 0, hi = 0;
    for (int r = 0; r < kIdaMaxDepth; ++r) {                              // the prefix: rows below floor <= max_depth are the caller's
        uint32_t m = kIdaNoMove;
        if (!l.status && r < f) {
            m = a.path[(int64_t)r * a.path_pitch + c];
            if (m >= kIdaNoMove) {
                l.status |= IDA_BAD_FRAME;
                m = kIdaNoMove;
            }
        }
        x = ida_move(x, s_moves[m]);
        if (r < f) ida_nib_set(lo, hi, r, m);
    }
    const uint32_t h = ida_h(x, a.t, l.status == 0u);
    if (!l.status && h == 0xFFu) l.status = IDA_ILLEGAL;
    if (!l.status) {
        l.lo = lo;
        l.hi = hi;
        first_bound(l, f, h);
        if (ida_goal(x)) l.status = IDA_SOLVED;
        else first_over(l, a.limit[c] < a.max_depth ? a.limit[c] : a.max_depth);
    }
    frame_store(a.fr, c, l);
}

__global__ void __launch_bounds__(kWave) k_ida_search(IdaArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_moves[13][16];
    moves_load(s_moves, c_ida_moves.w);
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const bool mine = c < a.n && a.fr.status[c] == 0u;                       // a cube with a nonzero status is not touched
    IdaCube x{};
    uint64_t lo = 0, hi = 0, nodes = 0;
    uint32_t status = 0, cursor = 0;
    int32_t f = 0, depth = 0, bound = 0, next = kIdaInf, lim = 0;
    if (mine) {
        if (!ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x)) status = IDA_ILLEGAL;
        f = a.floor ? a.floor[c] : 0;
        lo = a.fr.trail[2 * c];
        hi = a.fr.trail[2 * c + 1];
        cursor = a.fr.cursor[c];
        depth = a.fr.depth[c];
        bound = a.fr.bound[c];
        next = a.fr.next[c];
        nodes = a.fr.nodes[c];
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
    for (int64_t step = 0; step < a.fr.max_steps; ++step) {                  // the only loop: whatever the tables hold, it ends
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
        a.fr.trail[2 * c] = lo;
        a.fr.trail[2 * c + 1] = hi;
        a.fr.cursor[c] = (uint8_t)cursor;
        a.fr.depth[c] = depth;
        a.fr.bound[c] = bound;
        a.fr.next[c] = next;
        a.fr.nodes[c] = nodes;
        a.fr.status[c] = (uint8_t)status;
        if (status == IDA_SOLVED)
            for (int r = 0; r < kIdaMaxDepth; ++r)
                if (r >= f && r < depth) a.path[(int64_t)r * a.path_pitch + c] = (uint8_t)ida_nib(lo, hi, r);   // depth <= max_depth
    }
    const unsigned long long bal = __ballot(run);
    if (threadIdx.x == 0 && bal) atomicAdd(a.fr.running, (uint32_t)__popcll(bal));
}

int ida_args(const char *fn, const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *corner, int64_t corner_bytes, int n_edge,
             const int *masks, const uint8_t *const *edge_tables, const int64_t *edge_bytes, uint8_t *path, int max_depth, int64_t path_pitch,
             const int32_t *floor, const int32_t *limit, const SearchFrame &fr, IdaArgs &a) {
    const auto bad = [fn](const char *what) { return fail(RC_EINVAL, "%s: %s", fn, what); };
    int sh;
    if (int rc = cubie_arg(fn, cubies, n, cubie_pitch, sh)) return rc;
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
    if (int rc = path_arg(fn, path, max_depth, path_pitch, kIdaMaxDepth, n, "n")) return rc;
    if (floor && !aligned16(floor)) return bad("floor is not 16-byte aligned");
    if (!limit || !aligned16(limit)) return bad("limit is NULL or not 16-byte aligned");
    if (int rc = frame_arg(fn, fr)) return rc;
    a = IdaArgs{cubies, n, cubie_pitch, sh, t, path, max_depth, path_pitch, floor, limit, fr};
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
                          path_pitch, floor, limit, SearchFrame{trail, cursor, depth, bound, next, nodes, status, 0, nullptr}, a))
        return rc;
    return ida_launch(k_ida_init, a, S(stream));
}

int ida_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *corner_table, int64_t corner_bytes, int n_edge,
               const int *masks, const uint8_t *const *edge_tables, const int64_t *edge_bytes, uint8_t *path, int max_depth, int64_t path_pitch,
               const int32_t *floor, const int32_t *limit, uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next,
               uint64_t *nodes, uint8_t *status, int64_t max_steps, uint32_t *running, void *stream) {
    RC_NEED_INIT();
    IdaArgs a;
    if (int rc = ida_args("ida_search", cubies, n, cubie_pitch, corner_table, corner_bytes, n_edge, masks, edge_tables, edge_bytes, path,
                          max_depth, path_pitch, floor, limit, SearchFrame{trail, cursor, depth, bound, next, nodes, status, max_steps, running}, a))
        return rc;
    if (int rc = steps_arg("ida_search", a.fr, kIdaMaxSteps, "ida_max_steps()")) return rc;
    return ida_launch(k_ida_search, a, S(stream));
}

}  // extern "C"

// ================================================================================================================== two-phase
// Kociemba's two phases as two more policies of the state machine above.  The tables and tp_index are rc_chain.h's TpLevels /
// k_tp_index.  Both tables of a phase are ranked before either is read.
namespace {

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

// ----------------------------------------------------------------------------------------------------------------- phase 1
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
    int32_t *found;
    SearchFrame fr;
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

// A G1 child (h == 0) is never entered: it is emitted if it is of this iteration's length and does not end in a U or D turn, and
// the K-th one ends the lane; so an entered child has h >= 1 and the trail stays below 32
struct Tp1Search {
    static constexpr uint32_t NGEN = 12u, NONE = kIdaNoMove;
    static constexpr bool UNIT = true;
    __device__ static uint32_t row(uint32_t j) { return j; }
    __device__ static uint32_t undo(uint32_t j) { return j ^ 1u; }
    __device__ static int32_t cost(uint32_t) { return 1; }
    __device__ static uint32_t allowed(const IdaLane &l, int32_t k, uint32_t last) {
        return ida_allowed(k >= 2 ? ida_nib(l.lo, l.hi, k - 2) : kIdaNoMove, last);
    }
    const Tp1Args &a;
    int64_t c;
    int32_t found;
    static constexpr int32_t floor = 0;
    __device__ uint32_t h(const IdaCube &y, bool live) const { return tp_h1(y, a.t, live); }
    __device__ static bool enters(uint32_t h) { return h != 0u; }
    __device__ uint32_t emit(const IdaLane &l, const IdaCube &y, uint32_t m) {
        if (l.depth + 1 != l.bound || ((0xC3u >> m) & 1u)) return 0u;
        uint64_t lo = l.lo, hi = l.hi;
        ida_nib_set(lo, hi, l.depth, m);                                  // depth + 1 <= bound <= 32
        tp1_emit(a, c, found, y, lo, hi, l.depth + 1);
        return ++found == a.K ? TP_FULL : 0u;
    }
    __device__ static bool goal(const IdaCube &, uint32_t) { return false; }
};

__global__ void __launch_bounds__(kWave) k_tp1_init(Tp1Args a) {
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (c >= a.n) return;
    IdaCube x;
    IdaLane l;
    l.status = ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x) ? 0u : TP_ILLEGAL;
    const uint32_t h = tp_h1(x, a.t, l.status == 0u);
    if (!l.status && h == 0xFFu) l.status = TP_ILLEGAL;
    int32_t found = 0;
    if (!l.status) {
        first_bound(l, 0, h);
        if (h == 0u) {                                                     // the root is in G1: candidate 0, of length 0
            tp1_emit(a, c, 0, x, 0, 0, 0);
            found = 1;
            if (found == a.K) l.status = TP_FULL;
        }
        if (!l.status) first_over(l, tp1_lim(a, c));
    }
    frame_store(a.fr, c, l);
    a.found[c] = found;
}

__global__ void __launch_bounds__(kWave) k_tp1_search(Tp1Args a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_moves[kTpRows][16];
    moves_load(s_moves, c_tp_moves.w);
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const bool mine = c < a.n && a.fr.status[c] == 0u;
    IdaCube x{};
    IdaLane l;
    Tp1Search p{a, c, 0};
    int32_t lim = 0;
    if (mine) {
        // the cube before the frame: the frame's registers live across the 20 byte loads would cost a wave per SIMD (80 VGPRs, not 59)
        const bool legal = ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x);
        l = frame_load(a.fr, c);
        if (!legal) l.status = TP_ILLEGAL;
        p.found = a.found[c];
        lim = tp1_lim(a, c);
        if (l.depth < 0 || l.depth >= kTpMaxTrail || l.cursor > kIdaNoMove || l.bound > lim || l.depth > l.bound || p.found < 0 || p.found >= a.K)
            l.status |= TP_BAD_FRAME;
    }
    ida_replay<Tp1Search>(s_moves, x, l, mine, 0);
    ida_passes(p, s_moves, a.fr, x, l, lim, mine && !l.status);
    if (mine) {
        frame_store(a.fr, c, l);
        a.found[c] = p.found;
    }
}

// ----------------------------------------------------------------------------------------------------------------- phase 2
struct Tp2Args {
    const uint8_t *cubies;
    int64_t n, pitch;
    int sh;
    TpTables t;
    uint8_t *path;
    int32_t max_depth;
    int64_t path_pitch;
    const int32_t *floor, *limit;
    SearchFrame fr;
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

// The trail holds generators, depth their cost beyond the floor's; the canonical rule is ida_allowed on the last two ACTIONS that the
// prefix and the trail spell.  Every admissible child is entered; h == 0 ends the lane
struct Tp2Search {
    static constexpr uint32_t NGEN = 8u, NONE = 0u;
    static constexpr bool UNIT = false;
    const TpTables &t;
    uint32_t pre1, pre2;
    static constexpr int32_t floor = 0;
    __device__ static uint32_t row(uint32_t j) { return tp_gen_row(j); }
    __device__ static uint32_t undo(uint32_t j) { return tp_gen_back(j); }
    __device__ static int32_t cost(uint32_t j) { return 1 + (int32_t)tp_gen_half(j); }
    __device__ uint32_t allowed(const IdaLane &l, int32_t k, uint32_t last) const {
        uint32_t p1 = pre1, p2 = pre2;
        if (k >= 1) {
            p1 = tp_gen_action(last);
            p2 = tp_gen_half(last) ? p1 : k >= 2 ? tp_gen_action(ida_nib(l.lo, l.hi, k - 2)) : pre1;
        }
        return tp_gen_allowed(ida_allowed(p2, p1));
    }
    __device__ uint32_t h(const IdaCube &y, bool live) const { return tp_h2(y, t, live); }
    __device__ static bool enters(uint32_t) { return true; }
    __device__ static uint32_t emit(const IdaLane &, const IdaCube &, uint32_t) { return 0u; }
    __device__ static bool goal(const IdaCube &, uint32_t h) { return h == 0u; }
};

__global__ void __launch_bounds__(kWave) k_tp2_init(Tp2Args a) {
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (c >= a.n) return;
    IdaCube x;
    IdaLane l;
    l.status = ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x) ? 0u : TP_ILLEGAL;
    const int32_t f = a.floor ? a.floor[c] : 0;
    uint32_t pre1, pre2;
    if (!tp2_prefix(a, c, f, pre1, pre2)) l.status |= TP_BAD_FRAME;
    if (!l.status && !tp_in_g1(x)) l.status = TP_OUTSIDE;
    const uint32_t h = tp_h2(x, a.t, l.status == 0u);
    if (!l.status && h == 0xFFu) l.status = TP_ILLEGAL;
    if (!l.status) {
        first_bound(l, f, h);
        if (!first_over(l, tp2_lim(a, c, f)) && h == 0u) l.status = TP_SOLVED;   // the limit before the goal: an empty slot is skipped here
    }
    frame_store(a.fr, c, l);
}

__global__ void __launch_bounds__(kWave) k_tp2_search(Tp2Args a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_moves[kTpRows][16];
    moves_load(s_moves, c_tp_moves.w);
    const int64_t c = (int64_t)blockIdx.x * kWave + threadIdx.x;
    const bool mine = c < a.n && a.fr.status[c] == 0u;
    IdaCube x{};
    IdaLane l;
    Tp2Search p{a.t, kIdaNoMove, kIdaNoMove};
    int32_t f = 0, lim = 0;
    if (mine) {
        uint32_t status = ida_load(a.cubies + cubie_off(c, a.pitch, a.sh, Cube3::SLOTS), a.pitch, x) ? 0u : TP_ILLEGAL;
        f = a.floor ? a.floor[c] : 0;
        if (!tp2_prefix(a, c, f, p.pre1, p.pre2)) {
            status |= TP_BAD_FRAME;
            f = 0;
        }
        if (!status && !tp_in_g1(x)) status = TP_OUTSIDE;
        l = frame_load(a.fr, c);                                           // after the cube, as in phase 1: 53 VGPRs, not 71
        l.status = status;
        lim = tp2_lim(a, c, f);
        if (l.depth < f || l.depth > a.max_depth || l.depth > l.bound || l.cursor > 8u || l.bound > lim) l.status |= TP_BAD_FRAME;
    }
    ida_replay<Tp2Search>(s_moves, x, l, mine, f);
    ida_passes(p, s_moves, a.fr, x, l, lim, mine && !l.status);
    if (mine) {
        frame_store(a.fr, c, l);
        if (l.status == TP_SOLVED) {
            int32_t r = f;
            for (int i = 0; i < kTpMaxTrail; ++i)
                if (i < l.k) {
                    const uint32_t j = ida_nib(l.lo, l.hi, i), act = tp_gen_action(j);
                    for (uint32_t t = 0; t <= tp_gen_half(j); ++t)
                        if (r < a.max_depth) a.path[(int64_t)r++ * a.path_pitch + c] = (uint8_t)act;   // r < depth <= max_depth; the guard stays
                }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- host
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
             int32_t *cand_length, uint8_t *cand, int64_t cand_pitch, int32_t *found, const SearchFrame &fr, Tp1Args &a) {
    const auto bad = [fn](const char *what) { return fail(RC_EINVAL, "%s: %s", fn, what); };
    int sh;
    if (int rc = cubie_arg(fn, cubies, n, cubie_pitch, sh)) return rc;
    TpTables t{};
    if (int rc = tp_tables_arg(fn, 1, ta, bytes_a, tb, bytes_b, t)) return rc;
    if (!limit || !aligned16(limit)) return bad("limit is NULL or not 16-byte aligned");
    if (K < 1 || K > kTpMaxK) return bad("candidates must be in 1..4096");
    if (stride < n || stride < 16 || (stride & 15) != 0 || stride > ((int64_t)1 << 31) / K)
        return bad("stride: need stride % 16 == 0, stride >= max(n, 16) and candidates * stride <= 2^31");
    const int64_t cols = (int64_t)K * stride;
    if (int rc = path_arg(fn, path, max_depth, path_pitch, kTpMaxDepth, cols, "candidates * stride")) return rc;
    if (!cand_length || !aligned16(cand_length)) return bad("cand_length is NULL or not 16-byte aligned");
    if (!cand || !aligned16(cand)) return bad("cand_cubies is NULL or not 16-byte aligned");
    const int cand_sh = tile_shift(cand_pitch, cols, Cube3::SLOTS);
    if (cand_sh < 0) return bad("cand_pitch: need pitch % 16 == 0 and pitch >= candidates * stride, or a power-of-two tile >= 512");
    if (int rc = frame_arg(fn, fr, &found)) return rc;
    a = Tp1Args{cubies, n, cubie_pitch, sh, t, limit, K, stride, path, max_depth, path_pitch, cand_length, cand, cand_pitch, cand_sh, found, fr};
    return RC_OK;
}

int tp2_args(const char *fn, const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *ta, int64_t bytes_a, const uint8_t *tb,
             int64_t bytes_b, uint8_t *path, int max_depth, int64_t path_pitch, const int32_t *floor, const int32_t *limit,
             const SearchFrame &fr, Tp2Args &a) {
    const auto bad = [fn](const char *what) { return fail(RC_EINVAL, "%s: %s", fn, what); };
    int sh;
    if (int rc = cubie_arg(fn, cubies, n, cubie_pitch, sh)) return rc;
    TpTables t{};
    if (int rc = tp_tables_arg(fn, 2, ta, bytes_a, tb, bytes_b, t)) return rc;
    if (int rc = path_arg(fn, path, max_depth, path_pitch, kTpMaxDepth, n, "n")) return rc;
    if (floor && !aligned16(floor)) return bad("floor is not 16-byte aligned");
    if (!limit || !aligned16(limit)) return bad("limit is NULL or not 16-byte aligned");
    if (int rc = frame_arg(fn, fr)) return rc;
    a = Tp2Args{cubies, n, cubie_pitch, sh, t, path, max_depth, path_pitch, floor, limit, fr};
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
    if (int rc = tp_which_arg("tp_index", which)) return rc;
    int sh;
    if (int rc = cubie_arg("tp_index", cubies, n, cubie_pitch, sh)) return rc;
    if (!index || !aligned16(index)) return fail(RC_EINVAL, "tp_index: index is NULL or not 16-byte aligned");
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
                          path_pitch, cand_length, cand_cubies, cand_pitch, found,
                          SearchFrame{trail, cursor, depth, bound, next, nodes, status, 0, nullptr}, a))
        return rc;
    return ida_launch(k_tp1_init, a, S(stream));
}

int tp_phase1_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                     int64_t bytes_b, const int32_t *limit, int candidates, int64_t stride, uint8_t *path, int max_depth, int64_t path_pitch,
                     int32_t *cand_length, uint8_t *cand_cubies, int64_t cand_pitch, uint64_t *trail, uint8_t *cursor, int32_t *depth,
                     int32_t *bound, int32_t *next, uint64_t *nodes, int32_t *found, uint8_t *status, int64_t max_steps, uint32_t *running,
                     void *stream) {
    RC_NEED_INIT();
    Tp1Args a;
    if (int rc = tp1_args("tp_phase1_search", cubies, n, cubie_pitch, table_a, bytes_a, table_b, bytes_b, limit, candidates, stride, path,
                          max_depth, path_pitch, cand_length, cand_cubies, cand_pitch, found,
                          SearchFrame{trail, cursor, depth, bound, next, nodes, status, max_steps, running}, a))
        return rc;
    if (int rc = steps_arg("tp_phase1_search", a.fr, kTpMaxSteps, "tp_max_steps()")) return rc;
    return ida_launch(k_tp1_search, a, S(stream));
}

int tp_phase2_init(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                   int64_t bytes_b, uint8_t *path, int max_depth, int64_t path_pitch, const int32_t *floor, const int32_t *limit,
                   uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next, uint64_t *nodes, uint8_t *status,
                   void *stream) {
    RC_NEED_INIT();
    Tp2Args a;
    if (int rc = tp2_args("tp_phase2_init", cubies, n, cubie_pitch, table_a, bytes_a, table_b, bytes_b, path, max_depth, path_pitch, floor, limit,
                          SearchFrame{trail, cursor, depth, bound, next, nodes, status, 0, nullptr}, a))
        return rc;
    return ida_launch(k_tp2_init, a, S(stream));
}

int tp_phase2_search(const uint8_t *cubies, int64_t n, int64_t cubie_pitch, const uint8_t *table_a, int64_t bytes_a, const uint8_t *table_b,
                     int64_t bytes_b, uint8_t *path, int max_depth, int64_t path_pitch, const int32_t *floor, const int32_t *limit,
                     uint64_t *trail, uint8_t *cursor, int32_t *depth, int32_t *bound, int32_t *next, uint64_t *nodes, uint8_t *status,
                     int64_t max_steps, uint32_t *running, void *stream) {
    RC_NEED_INIT();
    Tp2Args a;
    if (int rc = tp2_args("tp_phase2_search", cubies, n, cubie_pitch, table_a, bytes_a, table_b, bytes_b, path, max_depth, path_pitch, floor,
                          limit, SearchFrame{trail, cursor, depth, bound, next, nodes, status, max_steps, running}, a))
        return rc;
    if (int rc = steps_arg("tp_phase2_search", a.fr, kTpMaxSteps, "tp_max_steps()")) return rc;
    return ida_launch(k_tp2_search, a, S(stream));
}

}  // extern "C"

// ================================================================================================================= cube group
// The cg_* entry points (include/rubikhip.h "Cube group", DESIGN.md "Cube group"): product, inverse, uniform random cubes and the
// inverse of an action list.  One lane per cube, the cube in the five registers of an IdaCube, both cube sizes through the same code
// (the 2x2x2: 7 rows, corner slot 7 holds piece 7 untwisted, the edge half compiled out).  The product is ida_move with the selector,
// twist and flip words taken from y's registers instead of a move row; the inverse places byte (q, -ori) at byte `piece` of the
// result by a shift, which is no register index; a random cube is 26 | 12 draws of a WalkRng.  No LDS, no indexed array, no scratch.
namespace {

__host__ __device__ constexpr IdaCube cg_identity() { return IdaCube{0x03020100u, 0x07060504u, 0x06040200u, 0x0E0C0A08u, 0x16141210u}; }
constexpr uint32_t kCgBadByte = 1u, kCgDupPiece = 2u;

// the T::SLOTS cubie bytes of cube `at` into x; kCgBadByte: a byte names no (piece, ori), kCgDupPiece: a piece occurs twice
template <class T>
__device__ __forceinline__ uint32_t cg_load(const uint8_t *at, int64_t pitch, IdaCube &x) {
    uint32_t w[5] = {0u, 0u, 0u, 0u, 0u}, cseen = 0, eseen = 0, bad = 0, dup = 0;
    sfor<T::NC>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t b = at[(int64_t)q * pitch], t = (b * 171u) >> 9, p = t & 7u;               // t = b / 3 for a byte
        bad |= (uint32_t)(b >= 3u * (uint32_t)T::NC);
        dup |= (cseen >> p) & 1u;
        cseen |= 1u << p;
        w[q >> 2] |= (p | ((b - 3u * t) << 4)) << (8 * (q & 3));
    });
    if constexpr (T::NC == 7) w[1] |= 0x07000000u;                                               // the fixed DLB cubie
    if constexpr (T::NE != 0) {
        sfor<12>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const uint32_t b = at[(int64_t)(T::NC + q) * pitch], p = (b >> 1) & 15u;
            bad |= (uint32_t)(b >= 24u);
            dup |= (eseen >> p) & 1u;
            eseen |= 1u << p;
            w[2 + (q >> 2)] |= (b & 31u) << (8 * (q & 3));
        });
    } else {
        w[2] = cg_identity().e0, w[3] = cg_identity().e1, w[4] = cg_identity().e2;
    }
    x = IdaCube{w[0], w[1], w[2], w[3], w[4]};
    return (bad ? kCgBadByte : 0u) | (dup ? kCgDupPiece : 0u);
}

template <class T>
__device__ __forceinline__ void cg_store(uint8_t *at, int64_t pitch, const IdaCube &x) {
    sfor<T::NC>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        const uint32_t v = ((q < 4 ? x.c0 : x.c1) >> (8 * (q & 3))) & 0xFFu;
        at[(int64_t)q * pitch] = (uint8_t)((v & 15u) * 3u + (v >> 4));
    });
    if constexpr (T::NE != 0)
        sfor<12>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            at[(int64_t)(T::NC + q) * pitch] = (uint8_t)(((q < 4 ? x.e0 : q < 8 ? x.e1 : x.e2) >> (8 * (q & 3))) & 0xFFu);
        });
}

// x then y: slot q of the result holds what x has in slot piece(y[q]), turned by ori(y[q]) -- the gather as written, for any bytes
template <class T>
__device__ __forceinline__ IdaCube cg_mul(const IdaCube &x, const IdaCube &y) {
    IdaCube o = cg_identity();
    o.c0 = ida_twist(__builtin_amdgcn_perm(x.c1, x.c0, y.c0 & 0x07070707u) + (y.c0 & 0x30303030u));
    o.c1 = ida_twist(__builtin_amdgcn_perm(x.c1, x.c0, y.c1 & 0x07070707u) + (y.c1 & 0x30303030u));
    if constexpr (T::NE != 0) {
        const auto edge = [&](uint32_t ye) {
            const uint32_t p = ye >> 1, high = ((p >> 3) & 0x01010101u) * 0xFFu;                   // 0xFF where the piece is 8..11
            const uint32_t lo = __builtin_amdgcn_perm(x.e1, x.e0, p & 0x07070707u), hi = __builtin_amdgcn_perm(0u, x.e2, p & 0x03030303u);
            return ((hi & high) | (lo & ~high)) ^ (ye & 0x01010101u);
        };
        o.e0 = edge(y.e0);
        o.e1 = edge(y.e1);
        o.e2 = edge(y.e2);
    }
    return o;
}

// out[piece(x[q])] = (q, -ori(x[q])): byte `piece` of the result's words, reached by a shift (x a permutation: no two meet)
template <class T>
__device__ __forceinline__ IdaCube cg_inv(const IdaCube &x) {
    IdaCube o = cg_identity();
    uint64_t c = 0;
    sfor<8>([&](auto qc) {
        constexpr uint32_t q = decltype(qc)::value;
        const uint32_t v = ((q < 4 ? x.c0 : x.c1) >> (8 * (q & 3))) & 0xFFu, ori = v >> 4, neg = ((ori << 1) | (ori >> 1)) & 3u;
        c |= (uint64_t)(q | (neg << 4)) << (8u * (v & 7u));
    });
    o.c0 = (uint32_t)c;
    o.c1 = (uint32_t)(c >> 32);
    if constexpr (T::NE != 0) {
        uint64_t lo = 0;
        uint32_t hi = 0;
        sfor<12>([&](auto qc) {
            constexpr uint32_t q = decltype(qc)::value;
            const uint32_t v = ((q < 4 ? x.e0 : q < 8 ? x.e1 : x.e2) >> (8 * (q & 3))) & 0xFFu, p = v >> 1, put = 2u * q + (v & 1u);
            lo |= p < 8u ? (uint64_t)put << (8u * (p & 7u)) : 0ull;
            hi |= p < 8u ? 0u : put << (8u * (p & 3u));
        });
        o.e0 = (uint32_t)lo;
        o.e1 = (uint32_t)(lo >> 32);
        o.e2 = hi;
    }
    return o;
}

struct CgRows {
    const uint8_t *at;
    int64_t pitch;
    int sh;
};
struct CgArgs {
    CgRows x, y;
    int64_t n;
    uint8_t *out;
    int64_t out_pitch;
    int out_sh;
    uint8_t *bad;
};

template <class T>
__global__ void __launch_bounds__(256) k_cg_product(CgArgs a) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n) return;
    IdaCube x, y;
    const uint32_t fx = cg_load<T>(a.x.at + cubie_off(c, a.x.pitch, a.x.sh, T::SLOTS), a.x.pitch, x);
    const uint32_t fy = cg_load<T>(a.y.at + cubie_off(c, a.y.pitch, a.y.sh, T::SLOTS), a.y.pitch, y);
    IdaCube o = cg_mul<T>(x, y);
    if ((fx | fy) & kCgBadByte) {
        o = cg_identity();
        *a.bad = 1;
    }
    cg_store<T>(a.out + cubie_off(c, a.out_pitch, a.out_sh, T::SLOTS), a.out_pitch, o);             // after both loads: out may be x or y
}

template <class T>
__global__ void __launch_bounds__(256) k_cg_inverse(CgArgs a) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.n) return;
    IdaCube x;
    const uint32_t fx = cg_load<T>(a.x.at + cubie_off(c, a.x.pitch, a.x.sh, T::SLOTS), a.x.pitch, x);
    IdaCube o = cg_inv<T>(x);
    if (fx) {
        o = cg_identity();
        *a.bad = 1;
    }
    cg_store<T>(a.out + cubie_off(c, a.out_pitch, a.out_sh, T::SLOTS), a.out_pitch, o);
}

// THE RULE's generator: the walk generator's state, its whole 64-bit output, a draw by the high half of a 64 x 64 product
struct CgRng : WalkRng {
    __device__ __forceinline__ uint64_t next64() {
        const uint64_t r = s0 + s1;
        (void)action(1u);                                                     // the state step
        return r;
    }
    __device__ __forceinline__ uint32_t draw(uint32_t m) { return (uint32_t)__umul64hi(next64(), (uint64_t)m); }
};

template <class T>
__global__ void __launch_bounds__(256) k_cg_random(uint64_t seed, uint64_t stream_id, int64_t first, int64_t n, uint8_t *out, int64_t pitch, int sh) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    CgRng g;
    g.seed(seed, stream_id, (uint64_t)(first + c));
    uint32_t cp = 0x76543210u, odd = 0, sum = 0, co = 0;                      // nibble q: the piece | the ori of corner slot q
    sfor<T::NC - 1>([&](auto kc) {
        constexpr uint32_t i = T::NC - 1 - decltype(kc)::value;
        const uint32_t j = g.draw(i + 1u), d = ((cp >> (4u * i)) ^ (cp >> (4u * j))) & 15u;
        cp ^= (d << (4u * i)) | (d << (4u * j));
        odd ^= (uint32_t)(j != i);
    });
    sfor<T::NC - 1>([&](auto qc) {
        const uint32_t t = g.draw(3u);
        sum += t;
        co |= t << (4u * decltype(qc)::value);
    });
    co |= ((3u - sum % 3u) % 3u) << (4u * (T::NC - 1));           // the last twist makes the sum 0 mod 3
    IdaCube x = cg_identity();
    x.c0 = x.c1 = 0u;
    sfor<8>([&](auto qc) {
        constexpr uint32_t q = decltype(qc)::value;
        const uint32_t v = (((cp >> (4u * q)) & 15u) | (((co >> (4u * q)) & 3u) << 4)) << (8u * (q & 3u));
        if (q < 4u) x.c0 |= v;
        else x.c1 |= v;
    });
    if constexpr (T::NE != 0) {
        uint64_t ep = 0xBA9876543210ull;
        uint32_t eodd = 0;
        sfor<11>([&](auto kc) {
            constexpr uint32_t i = 11u - decltype(kc)::value;
            const uint32_t j = g.draw(i + 1u);
            const uint64_t d = ((ep >> (4u * i)) ^ (ep >> (4u * j))) & 15ull;
            ep ^= (d << (4u * i)) | (d << (4u * j));
            eodd ^= (uint32_t)(j != i);
        });
        const uint64_t r = g.next64();
        uint32_t w[3] = {0u, 0u, 0u};
        sfor<12>([&](auto qc) {
            constexpr uint32_t q = decltype(qc)::value;
            const uint32_t flip = q < 11u ? (uint32_t)(r >> (63u - q)) & 1u : (uint32_t)__popcll(r >> 53) & 1u;
            w[q >> 2] |= (2u * ((uint32_t)(ep >> (4u * q)) & 15u) + flip) << (8u * (q & 3u));
        });
        if (odd != eodd) w[2] = __builtin_amdgcn_perm(0u, w[2], 0x02030100u);                      // slots 10 and 11 change places
        x.e0 = w[0], x.e1 = w[1], x.e2 = w[2];
    }
    cg_store<T>(out + cubie_off(c, pitch, sh, T::SLOTS), pitch, x);
}

// One lane per column: the entries below A go to the top of out's column, each ^ 1, in order; the rest of the column is A; then the
// top is reversed in place.  Every row a lane writes it has read before, so out may be the actions themselves.
__global__ void __launch_bounds__(256) k_cg_invert_actions(const uint8_t *actions, int64_t rows, int64_t n, int64_t act_pitch, uint32_t A,
                                                           uint8_t *out, int64_t out_pitch, uint8_t *bad) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    int64_t k = 0;
    uint32_t above = 0;
    for (int64_t r = 0; r < rows; ++r) {
        const uint32_t a = actions[r * act_pitch + c];
        above |= (uint32_t)(a > A);
        if (a < A) out[k++ * out_pitch + c] = (uint8_t)(a ^ 1u);
    }
    for (int64_t r = k; r < rows; ++r) out[r * out_pitch + c] = (uint8_t)A;
    for (int64_t lo = 0, hi = k - 1; lo < hi; ++lo, --hi) {
        const uint8_t u = out[lo * out_pitch + c], v = out[hi * out_pitch + c];
        out[lo * out_pitch + c] = v;
        out[hi * out_pitch + c] = u;
    }
    if (above) *bad = 1;
}

// the bytes a tiled cubie operand spans, from its first byte to one past cube n - 1's last row
inline int64_t cg_extent(int64_t n, int64_t pitch, int slots) {
    const int64_t t = tiles_of(n, pitch) - 1;
    return t * slots * pitch + (slots - 1) * pitch + (n - t * pitch);
}
inline bool cg_overlap(const void *p, int64_t pb, const void *q, int64_t qb) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)qb && b < a + (uintptr_t)pb;
}

// a cubie operand of a cg_* call: present, 16-byte aligned, a valid tiling for n cubes
int cg_rows_arg(const char *fn, const char *name, const void *p, int64_t pitch, int64_t n, int slots, int &sh) {
    if (!p || !aligned16(p)) return fail(RC_EINVAL, "%s: %s is NULL or not 16-byte aligned", fn, name);
    if ((sh = tile_shift(pitch, n, slots)) < 0)
        return fail(RC_EINVAL, "%s: %s_pitch: need pitch %% 16 == 0 and pitch >= n, or a power-of-two tile >= 512", fn, name);
    return RC_OK;
}

}  // namespace

extern "C" {

int cg_product(const uint8_t *x, int64_t x_pitch, const uint8_t *y, int64_t y_pitch, int64_t n, int cube_size, uint8_t *out, int64_t out_pitch,
               uint8_t *bad, void *stream) {
    RC_NEED_INIT();
    if (cube_size != 2 && cube_size != 3) return fail(RC_EINVAL, "cg_product: cube_size must be 2 or 3");
    if (n < 0) return fail(RC_EINVAL, "cg_product: n is negative");
    const int slots = cube_size == 3 ? Cube3::SLOTS : Cube2::SLOTS;
    CgArgs a{};
    if (int rc = cg_rows_arg("cg_product", "x", x, x_pitch, n, slots, a.x.sh)) return rc;
    if (int rc = cg_rows_arg("cg_product", "y", y, y_pitch, n, slots, a.y.sh)) return rc;
    if (int rc = cg_rows_arg("cg_product", "out", out, out_pitch, n, slots, a.out_sh)) return rc;
    if (!bad) return fail(RC_EINVAL, "cg_product: bad is NULL");
    if (n == 0) return RC_OK;
    const int64_t ob = cg_extent(n, out_pitch, slots);
    if (!(out == x && out_pitch == x_pitch) && cg_overlap(out, ob, x, cg_extent(n, x_pitch, slots)))
        return fail(RC_EINVAL, "cg_product: out overlaps x (out may be exactly x, with x's pitch)");
    if (!(out == y && out_pitch == y_pitch) && cg_overlap(out, ob, y, cg_extent(n, y_pitch, slots)))
        return fail(RC_EINVAL, "cg_product: out overlaps y (out may be exactly y, with y's pitch)");
    if (cg_overlap(bad, 1, out, ob)) return fail(RC_EINVAL, "cg_product: bad lies inside out");
    a.x.at = x, a.x.pitch = x_pitch, a.y.at = y, a.y.pitch = y_pitch;
    a.n = n, a.out = out, a.out_pitch = out_pitch, a.bad = bad;
    const int64_t blocks = ceil_div(n, 256);
    RC_GRID(blocks);
    return by_size(cube_size, [&](auto t) {
        hipLaunchKernelGGL(k_cg_product<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, S(stream), a);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

int cg_inverse(const uint8_t *x, int64_t x_pitch, int64_t n, int cube_size, uint8_t *out, int64_t out_pitch, uint8_t *bad, void *stream) {
    RC_NEED_INIT();
    if (cube_size != 2 && cube_size != 3) return fail(RC_EINVAL, "cg_inverse: cube_size must be 2 or 3");
    if (n < 0) return fail(RC_EINVAL, "cg_inverse: n is negative");
    const int slots = cube_size == 3 ? Cube3::SLOTS : Cube2::SLOTS;
    CgArgs a{};
    if (int rc = cg_rows_arg("cg_inverse", "x", x, x_pitch, n, slots, a.x.sh)) return rc;
    if (int rc = cg_rows_arg("cg_inverse", "out", out, out_pitch, n, slots, a.out_sh)) return rc;
    if (!bad) return fail(RC_EINVAL, "cg_inverse: bad is NULL");
    if (n == 0) return RC_OK;
    const int64_t ob = cg_extent(n, out_pitch, slots);
    if (!(out == x && out_pitch == x_pitch) && cg_overlap(out, ob, x, cg_extent(n, x_pitch, slots)))
        return fail(RC_EINVAL, "cg_inverse: out overlaps x (out may be exactly x, with x's pitch)");
    if (cg_overlap(bad, 1, out, ob)) return fail(RC_EINVAL, "cg_inverse: bad lies inside out");
    a.x.at = x, a.x.pitch = x_pitch;
    a.n = n, a.out = out, a.out_pitch = out_pitch, a.bad = bad;
    const int64_t blocks = ceil_div(n, 256);
    RC_GRID(blocks);
    return by_size(cube_size, [&](auto t) {
        hipLaunchKernelGGL(k_cg_inverse<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, S(stream), a);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

int cg_random(uint64_t seed, uint64_t stream_id, int64_t first, int64_t n, int cube_size, uint8_t *out, int64_t out_pitch, void *stream) {
    RC_NEED_INIT();
    if (cube_size != 2 && cube_size != 3) return fail(RC_EINVAL, "cg_random: cube_size must be 2 or 3");
    if (n < 0) return fail(RC_EINVAL, "cg_random: n is negative");
    if (first < 0 || first > INT64_MAX - n) return fail(RC_EINVAL, "cg_random: first is negative, or first + n overflows");
    int sh;
    if (int rc = cg_rows_arg("cg_random", "out", out, out_pitch, n, cube_size == 3 ? Cube3::SLOTS : Cube2::SLOTS, sh)) return rc;
    if (n == 0) return RC_OK;
    const int64_t blocks = ceil_div(n, 256);
    RC_GRID(blocks);
    return by_size(cube_size, [&](auto t) {
        hipLaunchKernelGGL(k_cg_random<decltype(t)>, dim3((unsigned)blocks), dim3(256), 0, S(stream), seed, stream_id, first, n, out, out_pitch, sh);
        RC_HIP(RC_EHIP, hipGetLastError());
        return RC_OK;
    });
}

int cg_invert_actions(const uint8_t *actions, int64_t rows, int64_t n, int64_t act_pitch, int cube_size, uint8_t *out, int64_t out_pitch,
                      uint8_t *bad, void *stream) {
    RC_NEED_INIT();
    const auto no = [](const char *what) { return fail(RC_EINVAL, "cg_invert_actions: %s", what); };
    if (cube_size != 2 && cube_size != 3) return no("cube_size must be 2 or 3");
    if (rows < 0) return no("rows is negative");
    if (n < 0) return no("n is negative");
    if (!actions || !aligned16(actions)) return no("actions is NULL or not 16-byte aligned");
    if (act_pitch < n || act_pitch <= 0 || (act_pitch & 15) != 0) return no("act_pitch: need act_pitch % 16 == 0 and act_pitch >= max(n, 16)");
    if (!out || !aligned16(out)) return no("out is NULL or not 16-byte aligned");
    if (out_pitch < n || out_pitch <= 0 || (out_pitch & 15) != 0) return no("out_pitch: need out_pitch % 16 == 0 and out_pitch >= max(n, 16)");
    if (rows > INT64_MAX / act_pitch || rows > INT64_MAX / out_pitch) return no("rows: rows * pitch overflows");
    if (!bad) return no("bad is NULL");
    if (n == 0 || rows == 0) return RC_OK;
    const int64_t ab = (rows - 1) * act_pitch + n, ob = (rows - 1) * out_pitch + n;
    if (!(out == actions && out_pitch == act_pitch) && cg_overlap(out, ob, actions, ab))
        return no("out overlaps actions (out may be exactly actions, with act_pitch)");
    if (cg_overlap(bad, 1, out, ob)) return no("bad lies inside out");
    const int64_t blocks = ceil_div(n, 256);
    RC_GRID(blocks);
    hipLaunchKernelGGL(k_cg_invert_actions, dim3((unsigned)blocks), dim3(256), 0, S(stream), actions, rows, n, act_pitch,
                       (uint32_t)(cube_size == 3 ? Cube3::A : Cube2::A), out, out_pitch, bad);
    RC_HIP(RC_EHIP, hipGetLastError());
    return RC_OK;
}

}  // extern "C"
