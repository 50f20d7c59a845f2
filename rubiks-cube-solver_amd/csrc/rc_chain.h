// rc_chain.h -- subgroup chain: the rct_* entry points (include/rubikhip.h "Subgroup chain", DESIGN.md "Subgroup chain"):
// Thistlethwaite's four coset-distance tables and the descent that walks any cube home through them, on rc_table.h's table core; a
// part of rubikhip.hip's translation unit, after rc_edge.h.  3x3x3 only; the stage is a template argument, so a stage's kernels hold
// its generators and its coordinate alone.
//   k_chain_fill      every entry 0xFF, the goals 0
//   ChainLevels       a stage's index space under k_table_level: its generators are an entry's neighbours
//   k_chain_index     20 cubie rows -> the stage's index, one lane per cube
//   k_chain_unrank    index -> the 20 cubie rows of a reachable cube of the stage's domain, one lane per cube
//   k_chain_descend   the walk: one lane per cube, at most kChainWalk generators, every table read through table_at
// The cube lives in four registers of nibbles and bits (ChainCube), never in an indexed array (no scratch); a generator is a
// compile-time gather on them, and what a stage's coordinate does not read the compiler drops.
#pragma once

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

// The 20 cubie bytes of cube `at`, read down the rows and validated: pack(slot, piece, ori, b) for every slot 0..19 (a compile-time
// constant), b the byte itself; piece is b / 3 mod 8 and ori b - 3 (b / 3) of a corner, (b >> 1) & 15 and b & 1 of an edge.
// false: a byte names no cubie, or a piece occurs twice.
template <class Pack>
__device__ __forceinline__ bool load_cubie_bytes(const uint8_t *at, int64_t pitch, Pack &&pack) {
    uint32_t cseen = 0, eseen = 0, bad = 0;
    sfor<8>([&](auto qc) {
        const uint32_t b = at[(int64_t)decltype(qc)::value * pitch], t = (b * 171u) >> 9, p = t & 7u;   // t = b / 3 for a byte
        bad |= (uint32_t)(b >= 24u) | ((cseen >> p) & 1u);
        cseen |= 1u << p;
        pack(qc, p, b - 3u * t, b);
    });
    sfor<12>([&](auto qc) {
        constexpr int q = 8 + decltype(qc)::value;
        const uint32_t b = at[(int64_t)q * pitch], p = (b >> 1) & 15u;
        bad |= (uint32_t)(b >= 24u) | ((eseen >> p) & 1u);
        eseen |= 1u << p;
        pack(std::integral_constant<int, q>{}, p, b & 1u, b);
    });
    return bad == 0u;
}

// load_cubie_bytes into the nibbles and bits of c
__device__ __forceinline__ bool chain_load(const uint8_t *at, int64_t pitch, ChainCube &c) {
    c = ChainCube{0u, 0u, 0ull, 0u};
    return load_cubie_bytes(at, pitch, [&](auto sc, uint32_t piece, uint32_t ori, uint32_t) {
        constexpr int s = decltype(sc)::value, q = s < 8 ? s : s - 8;
        if constexpr (s < 8) {
            c.cp |= piece << (4 * q);
            c.co |= ori << (4 * q);
        } else {
            c.ep |= (uint64_t)piece << (4 * q);
            c.eo |= ori << q;
        }
    });
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
struct ChainLevels {
    static constexpr int kNeighbours = Cube3::chain_ngen[STAGE];
    __host__ __device__ static constexpr uint32_t n() { return kChainN[STAGE]; }
    // stage 3 ranks and unranks through H in LDS: the block's copy, made before any lane needs it (no other stage reads it)
    __device__ static uint16_t *h() {
        __shared__ uint16_t s_h[kChainNH];
        return s_h;
    }
    __device__ void block_begin() const {
        if constexpr (STAGE == 3) chain_h_load(h());
    }
    __device__ ChainCube unrank(uint32_t i) const {
        ChainCube c;
        chain_unrank<STAGE>(i, h(), c);
        return c;
    }
    template <int G>
    __device__ uint32_t neighbour(const ChainCube &c) const { return chain_index<STAGE>(chain_move<STAGE, G>(c), h()); }
};

template <int STAGE>
__global__ void __launch_bounds__(256) k_chain_index(const uint8_t *cubies, int64_t n, int64_t pitch, int sh, uint32_t *index) {
    __shared__ uint16_t h[kChainNH];
    if constexpr (STAGE == 3) chain_h_load(h);
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    ChainCube c;
    const bool ok = chain_load(cubies + cubie_off(b, pitch, sh, Cube3::SLOTS), pitch, c) && chain_domain<STAGE>(c);
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
    chain_store(cubies + cubie_off(b, pitch, sh, Cube3::SLOTS), pitch, c);
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
    uint8_t *at = a.cubies + cubie_off(b, a.pitch, a.sh, Cube3::SLOTS);
    ChainCube c;
    uint32_t status = 0, d = 0xFFu;
    if (!chain_load(at, a.pitch, c)) {
        status = RCT_ILLEGAL;
    } else {
        d = table_at(a.table, chain_domain<STAGE>(c) ? chain_index<STAGE>(c, h) : 0xffffffffu, N);
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
                    const bool take = act == 0xFFu && table_at(a.table, chain_index<STAGE>(child, h), N) == d - 1u;
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

// ---- the two-phase coset spaces (include/rubikhip.h "Two-phase", the tp_* entry points of rc_ida.h): tables 0, 1 over every cube
// under the 12 actions, tables 2, 3 over G1 = stage 2's domain under stage 2's generators, a half turn costing 2
constexpr uint32_t kTpN[4] = {2187u * 495u, 2048u * 495u, 40320u * 24u, 40320u * 24u};

// bit q = edge slot q holds one of the pieces 8..11
__device__ __forceinline__ uint32_t chain_slice_mask(uint64_t ep) {
    uint32_t slice = 0;
    sfor<12>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        slice |= ((uint32_t)(ep >> (4 * q + 3)) & 1u) << q;
    });
    return slice;
}

template <int W>
__device__ __forceinline__ bool tp_domain(const ChainCube &c) {
    return W < 2 || chain_domain<2>(c);
}

template <int W>
__device__ __forceinline__ uint32_t tp_index(const ChainCube &c) {
    if constexpr (W == 0) {
        return chain_index<1>(c, nullptr);                                    // twist + 2187 * C: stage 1's, whatever eo is
    } else if constexpr (W == 1) {
        return (c.eo & 0x7FFu) + 2048u * chain_subset_rank<12>(chain_slice_mask(c.ep));
    } else if constexpr (W == 2) {
        return chain_lehmer<8>(c.cp) * 24u + chain_lehmer<4>((uint32_t)(c.ep >> 32) & 0x3333u);
    } else {
        return chain_lehmer<8>((uint32_t)c.ep) * 24u + chain_lehmer<4>((uint32_t)(c.ep >> 32) & 0x3333u);
    }
}

// a cube of table W's domain with index idx < N: what the index does not say is home (no neighbour's index reads it)
template <int W>
__device__ __forceinline__ ChainCube tp_unrank(uint32_t idx) {
    ChainCube c{kChainCornersHome, 0u, kChainEdgesHome, 0u};
    if constexpr (W == 0) {
        chain_unrank<1>(idx, nullptr, c);
    } else if constexpr (W == 1) {
        const uint32_t flip = idx % 2048u, slice = chain_subset_unrank<12>(idx / 2048u);
        c.eo = flip | (((uint32_t)__popc(flip) & 1u) << 11);
        c.ep = chain_place(slice, 0xBA98ull) | chain_place(~slice & 0xFFFu, 0x76543210ull);
    } else {
        const uint64_t low = chain_unlehmer<8>(idx / 24u, kChainCornersHome);
        if constexpr (W == 2) c.cp = (uint32_t)low;
        c.ep = (chain_unlehmer<4>(idx % 24u, 0xBA98ull) << 32) | (W == 3 ? low : (uint64_t)kChainCornersHome);
    }
    return c;
}

template <int W>
struct TpLevels {
    static constexpr int kStage = W < 2 ? 0 : 2, kNeighbours = Cube3::chain_ngen[kStage];
    __host__ __device__ static constexpr uint32_t n() { return kTpN[W]; }
    template <int G>
    __host__ __device__ static constexpr uint32_t cost() { return 1u + (uint32_t)(Cube3::chain_gen[kStage][G] >> 4); }
    __device__ void block_begin() const {}
    __device__ ChainCube unrank(uint32_t i) const { return tp_unrank<W>(i); }
    template <int G>
    __device__ uint32_t neighbour(const ChainCube &c) const { return tp_index<W>(chain_move<kStage, G>(c)); }
};

__global__ void __launch_bounds__(256) k_tp_fill(uint8_t *table, uint32_t n, uint32_t goal) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) table[i] = i == goal ? 0u : 0xFFu;
}

template <int W>
__global__ void __launch_bounds__(256) k_tp_index(const uint8_t *cubies, int64_t n, int64_t pitch, int sh, uint32_t *index) {
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    ChainCube c;
    const bool ok = chain_load(cubies + cubie_off(b, pitch, sh, Cube3::SLOTS), pitch, c) && tp_domain<W>(c);
    const uint32_t idx = tp_index<W>(c);
    index[b] = ok && idx < kTpN[W] ? idx : 0xffffffffu;
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
    return table_arg(fn, table, bytes, kChainN[stage], "rct_table_bytes(stage)");
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
    return by_stage(stage, [&](auto sc) {
        return table_build_level("rct_build_level", table, ChainLevels<decltype(sc)::value>{}, depth, count, S(stream), RC_EHIP);
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
