// rc_search.hip -- kernels and C ABI of librubiksearch.so (include/rubiksearch.h): the device half of the batched beam search
// (DESIGN.md "Beam search").  gfx950 only.  Built on rc_device.h: packed moves (fixed_move, action_masks + apply_move), the solved
// test (unsolved / done_bytes), the compact code (encode) and buffer row access.
//
//   k_init       roots -> slot 0 of every problem; solved roots end at length 0
//   k_expand     all A children of every beam slot: RC_FMT_CODE rows, valid / solved flags, exact sticker keys
//   k_insert     exact dedup: every valid candidate into a global open-addressing table (64-bit CAS); equal keys keep the lowest
//                candidate by atomicMin, so the owner of a key does not depend on the order in which the atomics land
//   k_select     one workgroup per problem: solved check, survivor marks, radix select of the W best (score desc, c asc), the kept
//                candidates listed in ascending c
//   k_advance    gather + move the kept parents into the other beam buffer, last action, history row
//   k_backtrack  history -> actions [D][P]
//
// The workgroup helpers under k_select and the A* kernels further down (every thread of a 256-thread workgroup calls them):
//   block_reduce     one value per workgroup from one per thread (min, sum; 32- or 64-bit)
//   radix_kth        the rank of the k-th best element: the threshold of a top-k
//   ordered_compact  the kept elements numbered in ascending index: where a top-k or a list of new nodes is written
//   owns_key         the exact dedup's answer for one candidate: it is the one that holds its key's slot of the scratch table
//   copy_root        a root's stickers into a beam slot or a pool node, with the solved test
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "../../include/rubiksearch.h"
#include "rc_device.h"
#include "rc_host.h"
#include "rc_table.h"

using namespace rc;

namespace {

constexpr int kWave = 64;
constexpr int kSpan = kWave * 4;                 // cubes per wave in the packed kernels (4 per lane, one dword per sticker row)
constexpr int kSelThreads = 256;
constexpr uint64_t kEmpty = ~0ull;

// Key layout: the stickers that can change, 3 bits each, 16 per 64-bit word (3x3x3: the 48 non-centre stickers; centres never move).
template <class T>
struct Key {
    static constexpr int N = T::SIZE == 3 ? 48 : 24;
    static constexpr int KW = (N + 15) / 16;
    static constexpr int sticker(int k) { return T::SIZE == 3 ? (k / 8) * 9 + (k % 8 < 4 ? k % 8 : k % 8 + 1) : k; }
};

// ------------------------------------------------------------------------------------- workgroup helpers
// One word per wave of a 256-thread workgroup: the scratch of block_reduce and ordered_compact, one array per word type.  Both
// end on a barrier after their last read of it, so calls may follow one another.
template <class V>
__device__ __forceinline__ V *wave_words() {
    __shared__ V w[kSelThreads / kWave];
    return w;
}

template <class V>
__device__ __forceinline__ V lane_xor(V v, int o) {
    if constexpr (sizeof(V) == 8)                              // the shuffle moves 32 bits
        return ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o);
    else return (V)__shfl_xor((int)v, o);
}

// op over the v of all 256 threads (op associative and commutative; V = uint32_t or uint64_t), returned to every thread
template <class V, class Op>
__device__ __forceinline__ V block_reduce(V v, Op op) {
    V *red = wave_words<V>();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, lane_xor(v, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const V r = op(op(red[0], red[1]), op(red[2], red[3]));
    __syncthreads();
    return r;
}
struct Min {
    template <class V>
    __device__ V operator()(V x, V y) const { return y < x ? y : x; }
};
struct Sum {
    template <class V>
    __device__ V operator()(V x, V y) const { return x + y; }
};

// The elements i < n with pred(i), numbered in ascending i: emit(i, slot) runs for each of them with slot = how many kept elements
// precede it.  Returns their number.  A caller that wants the first k only tests slot < k in emit.  n is the same for the whole
// workgroup; thread t sees the elements i = t + 256 r and nobody else's, so pred may read what the thread's own earlier emit (or
// earlier code at the same i) wrote without a barrier.  Barriers: two per round of 256 elements, the second after the round's
// last read of the shared words -- it is the trailing barrier that lets another call, or a block_reduce, follow at once.  They
// order the helper's own words only: a caller whose pred reads what OTHER threads wrote puts its own barrier before the call.
template <class P, class E>
__device__ __forceinline__ uint32_t ordered_compact(uint32_t n, P &&pred, E &&emit) {
    uint32_t *red = wave_words<uint32_t>();
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += kSelThreads) {
        const uint32_t i = i0 + tid;
        const bool keep = i < n && pred(i);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) red[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base;
        for (int q = 0; q < wv; ++q) off += red[q];
        const uint32_t tot = red[0] + red[1] + red[2] + red[3];
        if (keep) emit(i, off + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull)));
        base += tot;
        __syncthreads();
    }
    return base;
}

// rank of a candidate: larger is better.  Score order with NaN lowest and -0 == +0 in the high word, then the lower c.
__device__ __forceinline__ uint64_t rank_of(float v, uint32_t c) {
    uint32_t u = __float_as_uint(v);
    uint32_t o;
    if (v != v) o = 0u;
    else {
        if (u == 0x80000000u) u = 0u;
        o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);      // never 0: ~u == 0 only for a NaN pattern
    }
    return ((uint64_t)o << 32) | (0xFFFFFFFFu - c);
}

// The `need`-th best of the distinct 64-bit ranks of the eligible elements i < n (the caller has counted more than `need` of them):
// MSB-first radix select, 8 bits per pass, one 256-thread workgroup; rank(i, r) says whether i is eligible and gives its rank.
// Returns the threshold: the elements with rank >= it are exactly the `need` best.  Every thread of the workgroup calls it.
template <class F>
__device__ __forceinline__ uint64_t radix_kth(uint32_t n, uint32_t need_, F &&rank) {
    __shared__ uint32_t hist[256];
    __shared__ uint64_t s_prefix, s_mask;
    __shared__ uint32_t s_need, s_done;
    const int tid = threadIdx.x;
    if (tid == 0) { s_prefix = 0; s_mask = 0; s_need = need_; s_done = 0; }
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        const uint64_t prefix = s_prefix, mask = s_mask;
        for (uint32_t i = tid; i < n; i += kSelThreads) {
            uint64_t r;
            if (!rank(i, r)) continue;
            if ((r & mask) == prefix) atomicAdd(&hist[(r >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t need = s_need;
            uint32_t cum = 0;
            int bin = 255;
            for (; bin > 0 && cum + hist[bin] < need; --bin) cum += hist[bin];
            s_prefix = prefix | ((uint64_t)bin << shift);
            s_mask = mask | (255ull << shift);
            s_need = need - cum;
            s_done = hist[bin] == need - cum;                  // the whole bin is kept: ranks >= the prefix are exactly the best `need`
        }
        __syncthreads();
        if (s_done) break;
    }
    const uint64_t thr = s_prefix;
    __syncthreads();                                           // the shared words may be reused by the next call
    return thr;
}

// ------------------------------------------------------------------------------------------------- roots
// Root p of the roots buffer (one tile when rshift >= 63, else tiles of rpitch = 1 << rshift) -> the row at dst, sticker i at
// dst[i * dpitch]; each(i, v) sees every sticker on its way.  Returns whether the root is solved.
template <class T, class F>
__device__ __forceinline__ bool copy_root(const uint8_t *roots, int64_t p, int64_t rpitch, int rshift, uint8_t *dst, int64_t dpitch, F &&each) {
    const uint8_t *src = roots + (rshift >= 63 ? p : tiled(p, rpitch, rshift, T::S));
    bool solved = true;
    uint8_t first = 0;
    for (int i = 0; i < T::S; ++i) {
        const uint8_t v = src[(int64_t)i * rpitch];
        dst[(int64_t)i * dpitch] = v;
        if (i % T::FACE == 0) first = v;
        else solved = solved && v == first;                    // py333.py:229-233: every face equals its first sticker
        each(i, v);
    }
    return solved;
}

template <class T>
__global__ void __launch_bounds__(256) k_init(const uint8_t *roots, int64_t n, int64_t rpitch, int rshift, uint8_t *beam, int64_t pitch,
                                              int shift, int width, uint8_t *last, int32_t *live, uint8_t *active, int32_t *length,
                                              int32_t *solution) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int64_t b = p * width;
    const bool solved = copy_root<T>(roots, p, rpitch, rshift, beam + tiled(b, pitch, shift, T::S), pitch, [](int, uint8_t) {});
    last[b] = (uint8_t)T::A;
    live[p] = solved ? 0 : 1;
    active[p] = solved ? 0 : 1;
    length[p] = solved ? 0 : -1;
    solution[p] = -1;
}

// ------------------------------------------------------------------------------------------------ expand
struct ExpandArgs {
    const uint8_t *beam, *last_action;
    const int32_t *live;
    const uint8_t *active;
    uint8_t *code, *flags;
    uint64_t *keys;
    int64_t nb, nbp, pitch;       // nb = P * W slots, nbp = tiles * pitch
    int width, shift;
};

// One lane = 4 consecutive beam slots (one dword per sticker row), all A children in registers: a child is a renaming of the
// parent's registers (fixed_move).  Its codes come from its own look-ups (encode): the parent's shared family look-ups
// (family_codes) would stay live across all A children and spill.
template <class T>
__global__ void __launch_bounds__(kWave) k_expand(ExpandArgs a) {
    using K = Key<T>;
    const int64_t g0 = (int64_t)blockIdx.x * kSpan;            // a wave never straddles a tile (pitch >= 512)
    const uint32_t lo = threadIdx.x * 4;
    const int64_t col = g0 & (a.pitch - 1), tile = g0 >> a.shift;
    const uint32_t rs = (uint32_t)a.pitch;
    Pk<1> s[T::S];
    {
        const __amdgpu_buffer_rsrc_t r = make_srd(a.beam + tile * T::S * a.pitch + col);
#pragma unroll
        for (int i = 0; i < T::S; ++i) s[i] = bld<1, kAuxCached>(r, lo, i * rs);
    }
    uint32_t live = 0;                                         // 0x01 in byte q: slot g0 + lo + q is live
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t b = g0 + lo + q;
        if (b < a.nb) {
            const int64_t p = b / a.width, w = b - p * a.width;
            if (a.active[p] && w < a.live[p]) live |= 1u << (8 * q);
        }
    }
    const uint32_t last = *reinterpret_cast<const uint32_t *>(a.last_action + g0 + lo);
    sfor<T::A>([&](auto ac) {
        constexpr int A_ = decltype(ac)::value;
        Pk<1> c[T::S];
        fixed_move<T, 1, A_>(s, c);
        const uint32_t solved = done_bytes(unsolved<T, 1>(c)).d[0];
        Pk<1> x;
        x.d[0] = last ^ ((uint32_t)(A_ ^ 1) * 0x01010101u);
        const uint32_t undo = done_bytes(x).d[0];              // 0x01 where the slot was made by the inverse of A_
        const int64_t j0 = (int64_t)A_ * a.nbp + g0;
        *reinterpret_cast<uint32_t *>(a.flags + j0 + lo) = (live & ~undo) | (solved << 1);
        Pk<1> cc[T::SLOTS];
        encode<T, 1>(c, cc);                                   // the child's own look-ups: exact for any colouring
        store_rows<kAuxCached>(make_srd(a.code + ((int64_t)A_ * a.nbp + tile * a.pitch) * T::SLOTS + col), lo, rs, cc);
        uint64_t *kp = a.keys + j0 + lo;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint64_t w[K::KW] = {};
            sfor<K::N>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                w[k / 16] |= (uint64_t)((c[K::sticker(k)].d[0] >> (8 * q)) & 7u) << (3 * (k % 16));
            });
#pragma unroll
            for (int k = 0; k < K::KW; ++k) kp[(int64_t)k * T::A * a.nbp + q] = w[k];
        }
    });
}

// ------------------------------------------------------------------------------------------ dedup + select
// the candidates of one step (k_expand's output, scored) with the per-problem state they update and the scratch table of their keys
struct Cands {
    uint8_t *flags;
    const uint64_t *keys;
    const float *scores;
    const int32_t *live;
    uint8_t *active;
    int32_t *length, *solution;
    unsigned long long *table;
    uint64_t tmask;
    int64_t nbp;
    int width;
};
// ... and what the beam's select makes of them
struct SelectArgs : Cands {
    const int32_t *depth;
    uint16_t *sel_parent;
    uint8_t *sel_action;
    int32_t *sel_count;
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

template <class T>
__device__ __forceinline__ int64_t cand_j(const Cands &a, int64_t p, uint32_t c) {
    return (int64_t)(c % T::A) * a.nbp + p * a.width + c / T::A;
}

template <class T>
__device__ __forceinline__ void load_key(const Cands &a, int64_t j, uint64_t (&k)[Key<T>::KW]) {
#pragma unroll
    for (int x = 0; x < Key<T>::KW; ++x) k[x] = a.keys[(int64_t)x * T::A * a.nbp + j];
}

template <class T>
__device__ __forceinline__ uint64_t slot_of(const uint64_t (&k)[Key<T>::KW], int64_t p, uint64_t tmask) {
    uint64_t h = mix64((uint64_t)p + 0x9E3779B97F4A7C15ull);
#pragma unroll
    for (int x = 0; x < Key<T>::KW; ++x) h = mix64(h ^ k[x]);
    return h & tmask;
}

// the candidate `id` = (p << 32) | c holds the same key as (k, p)
template <class T>
__device__ __forceinline__ bool same_key(const Cands &a, uint64_t id, const uint64_t (&k)[Key<T>::KW], int64_t p) {
    if ((int64_t)(id >> 32) != p) return false;
    uint64_t o[Key<T>::KW];
    load_key<T>(a, cand_j<T>(a, p, (uint32_t)id), o);
    bool eq = true;
#pragma unroll
    for (int x = 0; x < Key<T>::KW; ++x) eq = eq && o[x] == k[x];
    return eq;
}

template <class T>
__global__ void __launch_bounds__(256) k_insert(Cands a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= T::A * a.nbp || !(a.flags[j] & RC_SEARCH_VALID)) return;        // valid implies a slot of a real problem
    const int64_t ac = j / a.nbp, b = j - ac * a.nbp, p = b / a.width, w = b - p * a.width;
    const unsigned long long id = ((uint64_t)p << 32) | (uint64_t)(w * T::A + ac);
    uint64_t k[Key<T>::KW];
    load_key<T>(a, j, k);
    uint64_t h = slot_of<T>(k, p, a.tmask);
    while (true) {                                             // the table has >= 2 slots per candidate: an empty one is reached
        const unsigned long long old = atomicCAS(&a.table[h], (unsigned long long)kEmpty, id);
        if (old == kEmpty) return;
        if (same_key<T>(a, old, k, p)) {                       // a slot's key never changes once set: only equal ids compete
            atomicMin(&a.table[h], id);
            return;
        }
        h = (h + 1) & a.tmask;
    }
}

// Candidate c of problem p (row j = cand_j, valid, so k_insert has put it into the scratch table): its key into k, and whether it
// is the entry its key's slot holds, i.e. the lowest c of the problem with that key.  Read-only on the table.
template <class T>
__device__ __forceinline__ bool owns_key(const Cands &a, int64_t p, uint32_t c, int64_t j, uint64_t (&k)[Key<T>::KW]) {
    load_key<T>(a, j, k);
    const uint64_t id = ((uint64_t)p << 32) | c;
    for (uint64_t h = slot_of<T>(k, p, a.tmask);; h = (h + 1) & a.tmask) {
        const uint64_t v = a.table[h];
        if (v == kEmpty) return false;                         // cannot happen: every valid candidate was inserted
        if (same_key<T>(a, v, k, p)) return v == id;
    }
}

// One workgroup per problem.  Every phase walks the candidates in c order with c = tid + 256 k, so a thread only ever re-reads
// the survivor flags it wrote itself.
template <class T>
__global__ void __launch_bounds__(kSelThreads) k_select(SelectArgs a) {
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    if (!a.active[p]) {
        if (tid == 0) a.sel_count[p] = 0;
        return;
    }
    const uint32_t W = (uint32_t)a.width;
    const uint32_t M = (uint32_t)min(max(a.live[p], 0), a.width) * T::A;
    // 1. solved check: the lowest valid solved candidate
    uint32_t best = ~0u;
    for (uint32_t c = tid; c < M; c += kSelThreads) {
        const uint8_t f = a.flags[cand_j<T>(a, p, c)];
        if ((f & RC_SEARCH_VALID) && (f & RC_SEARCH_SOLVED)) { best = c; break; }   // c grows: the thread's first is its lowest
    }
    best = block_reduce(best, Min{});
    if (best != ~0u) {
        if (tid == 0) {
            a.length[p] = *a.depth;
            a.solution[p] = (int32_t)best;
            a.active[p] = 0;
            a.sel_count[p] = 0;
        }
        return;
    }
    // 2. survivors: the candidate that owns its key's table slot
    uint32_t cnt = 0;
    for (uint32_t c = tid; c < M; c += kSelThreads) {
        const int64_t j = cand_j<T>(a, p, c);
        const uint8_t f = a.flags[j];
        if (!(f & RC_SEARCH_VALID)) continue;
        uint64_t k[Key<T>::KW];
        if (owns_key<T>(a, p, c, j, k)) {
            a.flags[j] = f | RC_SEARCH_SURVIVOR;
            ++cnt;
        }
    }
    const uint32_t nsurv = block_reduce(cnt, Sum{});
    // 3. the W-th best rank among the survivors (ranks are distinct)
    uint64_t thr = 0;
    if (nsurv > W)
        thr = radix_kth(M, W, [&](uint32_t c, uint64_t &r) {
            const int64_t j = cand_j<T>(a, p, c);
            if (!(a.flags[j] & RC_SEARCH_SURVIVOR)) return false;
            r = rank_of(a.scores[j], c);
            return true;
        });
    // 4. the kept candidates in ascending c
    const uint32_t kept = ordered_compact(
        M,
        [&](uint32_t c) {
            const int64_t j = cand_j<T>(a, p, c);
            return (a.flags[j] & RC_SEARCH_SURVIVOR) && (nsurv <= W || rank_of(a.scores[j], c) >= thr);
        },
        [&](uint32_t c, uint32_t slot) {
            if (slot < W) {
                a.sel_parent[p * a.width + slot] = (uint16_t)(c / T::A);
                a.sel_action[p * a.width + slot] = (uint8_t)(c % T::A);
            }
        });
    if (tid == 0) a.sel_count[p] = (int32_t)min(kept, W);
}

// ----------------------------------------------------------------------------------------------- advance
struct AdvanceArgs {
    const uint8_t *in;
    uint8_t *out;
    const uint16_t *sel_parent;
    const uint8_t *sel_action;
    const int32_t *sel_count;
    int32_t *live;
    uint8_t *last_action;
    uint16_t *hist_parent;
    uint8_t *hist_action;
    const int32_t *depth;
    int64_t nb, nbp, pitch;
    int width, shift, max_depth;
};

// One lane = 4 consecutive new slots: their parents' stickers gathered byte by byte, then ONE packed move with per-byte actions.
template <class T>
__global__ void __launch_bounds__(kWave) k_advance(AdvanceArgs a) {
    const int64_t g0 = (int64_t)blockIdx.x * kSpan;
    const uint32_t lo = threadIdx.x * 4;
    const int t = *a.depth;
    const bool record = t >= 1 && t <= a.max_depth;
    uint32_t act = 0;
    int64_t src[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t n = g0 + lo + q;
        uint32_t aq = T::A, wq = 0;
        src[q] = n;                                            // dead slots copy themselves under the no-op
        if (n < a.nb) {
            const int64_t p = n / a.width, i = n - p * a.width;
            const int32_t cnt = a.sel_count[p];
            if (i < cnt) {
                wq = min((uint32_t)a.sel_parent[n], (uint32_t)a.width - 1u);
                aq = min((uint32_t)a.sel_action[n], (uint32_t)T::A);
                src[q] = p * a.width + wq;
            }
            if (i == 0) a.live[p] = cnt;
        }
        act |= aq << (8 * q);
        a.last_action[n] = (uint8_t)aq;
        if (record) {
            a.hist_parent[(int64_t)(t - 1) * a.nbp + n] = (uint16_t)wq;
            a.hist_action[(int64_t)(t - 1) * a.nbp + n] = (uint8_t)aq;
        }
    }
    Pk<1> s[T::S];
#pragma unroll
    for (int i = 0; i < T::S; ++i) {
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) v |= (uint32_t)a.in[tiled(src[q], a.pitch, a.shift, T::S) + (int64_t)i * a.pitch] << (8 * q);
        s[i].d[0] = v;
    }
    Pk<1> ap;
    ap.d[0] = act;
    (void)move_rows<T, 1>(s, ap);                              // actions are 0..A by construction
    store_rows<kAuxCached>(make_srd(a.out + tiled(g0, a.pitch, a.shift, T::S)), lo, (uint32_t)a.pitch, s);
}

// --------------------------------------------------------------------------------------------- backtrack
__global__ void __launch_bounds__(256) k_backtrack(const uint16_t *hp, const uint8_t *ha, int64_t n, int width, int64_t nbp, int A,
                                                   int D, const int32_t *length, const int32_t *solution, uint8_t *actions) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    for (int d = 0; d < D; ++d) actions[(int64_t)d * n + p] = (uint8_t)A;
    const int L = length[p];
    const int32_t c = solution[p];
    if (L < 1 || L > D || c < 0 || c >= width * A) return;
    int64_t w = c / A;
    actions[(int64_t)(L - 1) * n + p] = (uint8_t)(c % A);
    for (int t = L - 1; t >= 1; --t) {                         // slot w of the beam after depth t came from history row t - 1
        const int64_t idx = (int64_t)(t - 1) * nbp + p * width + w;
        actions[(int64_t)(t - 1) * n + p] = ha[idx];
        w = hp[idx];
        if (w >= width) return;
    }
}

// --------------------------------------------------------------------------------------------------- fills
// The launchers clear their tables with these and not with hipMemsetAsync.  Observed on an MI355X with torch 2.10's HIP runtime
// 7.0.51831 (ROCm 7.2.0 installed), torch.cuda.graph on a side stream: a captured hipMemsetAsync(p, 0xFF, n) replays with other
// bytes -- all 0x00 for 3.6 MB, a mix of 0x00 and stale values for 64 KiB, with or without a kernel node in front of it;
// tools/probe_graph_memset.py shows it with the runtime call alone.  rcp_build_begin captured on its own then left a zeroed table and
// rc_search_select's table was never empty, so k_insert probed for ever (tests/test_gpu_stream_order.py).  Why the runtime does this
// is not known here; a kernel node replays as launched.  The probe says whether a later runtime lets the memset come back.
// p[0 .. n16) = 16 bytes of the 32-bit pattern v each, the first word of all `first`.
__global__ void __launch_bounds__(256) k_fill16(uint4 *p, int64_t n16, uint32_t v, uint32_t first) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = make_uint4(i == 0 ? first : v, v, v, v);
}

// ------------------------------------------------------------------------------------------------- host side
// -1: bad argument, -2: a HIP call failed (include/rubiksearch.h)
inline int fail(const char *msg) { return fail(-1, "%s", msg); }
inline int fail(const char *fn, const char *msg) { return fail(-1, "%s: %s", fn, msg); }

// `bytes` (a multiple of 16) at the 16-byte aligned p = the pattern v, the first word `first`: one launch on `st`
int fill16(void *p, int64_t bytes, uint32_t v, uint32_t first, hipStream_t st) {
    const int64_t n16 = bytes / 16;
    if (n16 <= 0) return 0;
    hipLaunchKernelGGL(k_fill16, dim3((unsigned)ceil_div(n16, (int64_t)256)), dim3(256), 0, st, static_cast<uint4 *>(p), n16, v, first);
    RC_HIP(-2, hipGetLastError());
    return 0;
}

struct Geo {
    int64_t nb, nbp;
    int shift;
};
// beam tiling of P problems x W slots at `pitch` (include/rubiksearch.h "Conventions")
template <class T>
int geometry(int64_t n_problems, int width, int64_t pitch, Geo &g) {
    if (n_problems < 1 || width < 1 || width > 65536) return fail("need n_problems >= 1 and 1 <= width <= 65536");
    if ((g.shift = tile_shift(pitch, INT64_MAX, T::S)) < 0) return fail("pitch must be a power of two >= 512 with S * pitch < 2^32");   // tiled even where one tile would do
    g.nb = n_problems * width;
    g.nbp = ceil_div(g.nb, pitch) * pitch;
    if ((int64_t)T::A * g.nbp / 256 > 0x7fffffff) return fail("too many candidates for one launch");
    return 0;
}

// Where fn's roots lie: one tile (root_pitch >= n, root_pitch % 16 == 0: rshift 63) or power-of-two tiles of root_pitch = 1 << rshift
template <class T>
int root_shift(const char *fn, int64_t n, int64_t root_pitch, int &rshift) {
    rshift = tile_shift(root_pitch, n, T::S);
    if (rshift == -1) return fail(fn, "bad root_pitch");
    if (rshift < 0) return fail(fn, "several root tiles need a power-of-two pitch >= 512");
    return 0;
}

// slots of an open-addressing table that holds `need` / 2 entries: a power of two, half empty at the least
int64_t pow2_slots(int64_t need) {
    int64_t s = 1024;
    while (s < need) s <<= 1;
    return s;
}
int64_t table_slots(int A, int64_t n_problems, int width) { return pow2_slots(2 * (int64_t)A * n_problems * width); }

}  // namespace

RC_BUILD_ID(rc_search_build_id)

const char *rc_search_last_error(void) { return t_err; }

int64_t rc_search_workspace_bytes(int cube_size, int64_t n_problems, int width) {
    if ((cube_size != 2 && cube_size != 3) || n_problems < 1 || width < 1 || width > 65536) return -1;
    return table_slots(cube_size == 3 ? 12 : 6, n_problems, width) * 8;
}

int rc_search_init(const uint8_t *roots, int64_t n, int64_t root_pitch, int cube_size, int width, uint8_t *beam, int64_t pitch,
                   uint8_t *last_action, int32_t *live, uint8_t *active, int32_t *length, int32_t *solution, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        if (int rc = geometry<T>(n, width, pitch, g)) return rc;
        if (any_null(roots, beam, last_action, live, active, length, solution)) return fail("rc_search_init: null buffer");
        int rshift;
        if (int rc = root_shift<T>("rc_search_init", n, root_pitch, rshift)) return rc;
        hipLaunchKernelGGL((k_init<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), roots, n, root_pitch, rshift, beam, pitch,
                           g.shift, width, last_action, live, active, length, solution);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rc_search_expand(const uint8_t *beam, int64_t n, int width, int64_t pitch, int cube_size, const uint8_t *last_action,
                     const int32_t *live, const uint8_t *active, uint8_t *code, uint8_t *flags, uint64_t *keys, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        if (int rc = geometry<T>(n, width, pitch, g)) return rc;
        if (any_null(beam, last_action, live, active, code, flags, keys)) return fail("rc_search_expand: null buffer");
        if (!all_aligned16(beam, last_action, code, flags, keys)) return fail("rc_search_expand: buffers must be 16-byte aligned");
        const ExpandArgs a{beam, last_action, live, active, code, flags, keys, g.nb, g.nbp, pitch, width, g.shift};
        hipLaunchKernelGGL((k_expand<T>), dim3((unsigned)(g.nbp / kSpan)), dim3(kWave), 0, S(stream), a);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rc_search_select(uint8_t *flags, const uint64_t *keys, const float *scores, int64_t n, int width, int64_t pitch, int cube_size,
                     const int32_t *live, uint8_t *active, int32_t *length, int32_t *solution, const int32_t *depth, uint16_t *sel_parent,
                     uint8_t *sel_action, int32_t *sel_count, void *workspace, int64_t workspace_bytes, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        if (int rc = geometry<T>(n, width, pitch, g)) return rc;
        if (any_null(flags, keys, scores, live, active, length, solution, depth, sel_parent, sel_action, sel_count, workspace))
            return fail("rc_search_select: null buffer");
        if (!aligned16(workspace)) return fail("rc_search_select: workspace must be 16-byte aligned");
        const int64_t slots = table_slots(T::A, n, width);
        if (workspace_bytes < slots * 8) return fail("rc_search_select: workspace smaller than rc_search_workspace_bytes()");
        if (n > 0x7fffffff) return fail("rc_search_select: too many problems for one launch");
        const Cands c{flags, keys, scores, live, active, length, solution, static_cast<unsigned long long *>(workspace), (uint64_t)(slots - 1),
                      g.nbp, width};
        const SelectArgs a{c, depth, sel_parent, sel_action, sel_count};
        if (int rc = fill16(workspace, slots * 8, ~0u, ~0u, S(stream))) return rc;       // every slot kEmpty
        hipLaunchKernelGGL((k_insert<T>), dim3((unsigned)((T::A * g.nbp + 255) / 256)), dim3(256), 0, S(stream), c);
        RC_HIP(-2, hipGetLastError());
        hipLaunchKernelGGL((k_select<T>), dim3((unsigned)n), dim3(kSelThreads), 0, S(stream), a);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rc_search_advance(const uint8_t *beam_in, uint8_t *beam_out, int64_t n, int width, int64_t pitch, int cube_size, const uint16_t *sel_parent,
                      const uint8_t *sel_action, const int32_t *sel_count, int32_t *live, uint8_t *last_action, uint16_t *hist_parent,
                      uint8_t *hist_action, const int32_t *depth, int max_depth, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        if (int rc = geometry<T>(n, width, pitch, g)) return rc;
        if (any_null(beam_in, beam_out, sel_parent, sel_action, sel_count, live, last_action, hist_parent, hist_action, depth))
            return fail("rc_search_advance: null buffer");
        if (max_depth < 1) return fail("rc_search_advance: max_depth must be >= 1");
        if (!aligned16(beam_out)) return fail("rc_search_advance: beam_out must be 16-byte aligned");
        const int64_t bytes = g.nbp * T::S;
        if (beam_in < beam_out + bytes && beam_out < beam_in + bytes) return fail("rc_search_advance: beam_in and beam_out overlap");
        const AdvanceArgs a{beam_in, beam_out, sel_parent, sel_action, sel_count, live, last_action, hist_parent, hist_action, depth,
                            g.nb, g.nbp, pitch, width, g.shift, max_depth};
        hipLaunchKernelGGL((k_advance<T>), dim3((unsigned)(g.nbp / kSpan)), dim3(kWave), 0, S(stream), a);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rc_search_backtrack(const uint16_t *hist_parent, const uint8_t *hist_action, int64_t n, int width, int64_t pitch, int cube_size,
                        int max_depth, const int32_t *length, const int32_t *solution, uint8_t *actions, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        if (int rc = geometry<T>(n, width, pitch, g)) return rc;
        if (any_null(hist_parent, hist_action, length, solution, actions)) return fail("rc_search_backtrack: null buffer");
        if (max_depth < 1) return fail("rc_search_backtrack: max_depth must be >= 1");
        hipLaunchKernelGGL(k_backtrack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), hist_parent, hist_action, n, width, g.nbp,
                           T::A, max_depth, length, solution, actions);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

// =========================================================================================== batch-weighted A*
// The rca_* entry points (include/rubiksearch.h "Batch-weighted A*", DESIGN.md "A* search"): a persistent node pool per problem
// around the beam's expand and the caller's net.
//
//   k_astar_init       root -> node 0 of every problem's pool (open, prio +inf), its key into the persistent table
//   k_astar_pop        one workgroup per problem: radix select of the B best open nodes (prio desc, node index desc), closed and
//                      gathered in ascending node index into the beam
//   k_insert           (the beam's) the iteration's valid candidates into the scratch table: equal keys keep the lowest c
//   k_astar_merge      one workgroup per problem: solved check, new = owner of its scratch slot and key absent from the persistent
//                      table, the new candidates appended in ascending c, their keys into the persistent table
//   k_astar_backtrack  parent links -> actions [D][P]
namespace {

constexpr uint8_t kOpen = RCA_OPEN, kClosed = RCA_CLOSED;

struct Pool {
    uint8_t *stickers;            // tiled [ptiles][S][ppitch], node gid = p * cap + n
    uint64_t *keys;               // [KW][np]
    int32_t *parent;
    uint8_t *action;
    int32_t *g;
    float *score, *prio;
    uint8_t *state;
    int32_t *count;
    uint8_t *overflow;
    unsigned long long *table;    // persistent: node gids, kEmpty elsewhere
    uint64_t tmask;
    int64_t np, ppitch;           // np = P * cap
    int pshift;
    int32_t cap;
};

// node `gid` of the pool holds key k
template <class T>
__device__ __forceinline__ bool node_has_key(const Pool &o, int64_t gid, const uint64_t (&k)[Key<T>::KW]) {
    bool eq = true;
#pragma unroll
    for (int x = 0; x < Key<T>::KW; ++x) eq = eq && o.keys[(int64_t)x * o.np + gid] == k[x];
    return eq;
}

// Insert node gid under a key no node of the table holds (merge has checked, init's table is empty): the first empty slot of the
// probe sequence.  Distinct keys only ever compete for a slot, never for an owner, so where the entries land does not matter.
__device__ __forceinline__ void table_put(const Pool &o, uint64_t h, int64_t gid) {
    while (atomicCAS(&o.table[h], (unsigned long long)kEmpty, (unsigned long long)gid) != kEmpty) h = (h + 1) & o.tmask;
}

template <class T>
__global__ void __launch_bounds__(256) k_astar_init(const uint8_t *roots, int64_t n, int64_t rpitch, int rshift, Pool o, int32_t *live,
                                                    uint8_t *active, int32_t *length, int32_t *solution, int32_t *ended) {
    using K = Key<T>;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int64_t gid = p * o.cap;
    uint64_t k[K::KW] = {};
    int kk = 0;
    const bool solved = copy_root<T>(roots, p, rpitch, rshift, o.stickers + tiled(gid, o.ppitch, o.pshift, T::S), o.ppitch, [&](int i, uint8_t v) {
        if (!(T::SIZE == 3 && i % 9 == 4)) {                   // Key<T>::sticker enumerates the non-centre stickers in ascending order
            k[kk / 16] |= (uint64_t)(v & 7u) << (3 * (kk % 16));
            ++kk;
        }
    });
#pragma unroll
    for (int x = 0; x < K::KW; ++x) o.keys[(int64_t)x * o.np + gid] = k[x];
    o.parent[gid] = -1;
    o.action[gid] = (uint8_t)T::A;
    o.g[gid] = 0;
    o.score[gid] = 0.0f;
    o.prio[gid] = __uint_as_float(0x7F800000u);                // +inf: popped first whatever the net says
    o.state[gid] = kOpen;
    o.count[p] = 1;
    o.overflow[p] = 0;
    table_put(o, slot_of<T>(k, p, o.tmask), gid);
    live[p] = 0;
    active[p] = solved ? 0 : 1;
    length[p] = solved ? 0 : -1;
    solution[2 * p] = -1;
    solution[2 * p + 1] = T::A;
    ended[p] = 0;
}

struct PopArgs {
    const uint8_t *stickers, *action;                          // the pool: only `state` is written
    const float *prio;
    uint8_t *state;
    const int32_t *count;
    int64_t ppitch;
    int pshift;
    int32_t cap;
    const int32_t *iteration;
    uint8_t *beam, *last_action;
    int32_t *live;
    uint8_t *active;
    int32_t *ended, *pop_node;
    int64_t pitch;
    int shift, batch;
};

// One workgroup per problem.  Ranks are distinct (the node index is their low word), so the radix select keeps exactly B nodes.
template <class T>
__global__ void __launch_bounds__(kSelThreads) k_astar_pop(PopArgs a) {
    const PopArgs &o = a;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    if (!a.active[p]) return;
    const int64_t g0 = p * o.cap;
    const uint32_t n = (uint32_t)min(max(o.count[p], 0), o.cap), B = (uint32_t)a.batch;
    uint32_t cnt = 0;
    for (uint32_t i = tid; i < n; i += kSelThreads) cnt += o.state[g0 + i] == kOpen;
    const uint32_t nopen = block_reduce(cnt, Sum{});
    if (nopen == 0) {                                          // exhausted: length stays -1
        if (tid == 0) {
            a.active[p] = 0;
            a.live[p] = 0;
            a.ended[p] = *a.iteration;
        }
        return;
    }
    uint64_t thr = 0;
    if (nopen > B)                                             // the B-th best rank; the node index is the low word: the higher one wins a tie
        thr = radix_kth(n, B, [&](uint32_t i, uint64_t &r) {
            if (o.state[g0 + i] != kOpen) return false;
            r = rank_of(o.prio[g0 + i], 0xFFFFFFFFu - i);
            return true;
        });
    const uint32_t npop = ordered_compact(                     // the popped nodes in ascending node index
        n, [&](uint32_t i) { return o.state[g0 + i] == kOpen && (nopen <= B || rank_of(o.prio[g0 + i], 0xFFFFFFFFu - i) >= thr); },
        [&](uint32_t i, uint32_t slot) {
            if (slot >= B) return;
            const int64_t b = p * a.batch + slot;
            o.state[g0 + i] = kClosed;
            a.pop_node[b] = (int32_t)i;
            a.last_action[b] = o.action[g0 + i];
            const uint8_t *src = o.stickers + tiled(g0 + i, o.ppitch, o.pshift, T::S);
            uint8_t *dst = a.beam + tiled(b, a.pitch, a.shift, T::S);
#pragma unroll
            for (int s = 0; s < T::S; ++s) dst[(int64_t)s * a.pitch] = src[(int64_t)s * o.ppitch];
        });
    if (tid == 0) a.live[p] = (int32_t)min(npop, B);
}

// prio = score - weight * g as TWO roundings, never an fma: numpy float32 bit for bit.  HIP's __fmul_rn / __fsub_rn are the plain
// operators, which the compiler contracted into one v_fma_f32 once they were inlined next to each other; the pragma takes the
// permission to contract from the two operations of this function, wherever it is inlined.
__device__ __forceinline__ float prio_of(float score, float weight, int32_t g) {
#pragma clang fp contract(off)
    const float prod = weight * (float)g;
    return score - prod;
}

struct MergeArgs {
    Cands s;                      // the iteration's candidates and the scratch table k_insert filled
    Pool o;
    const int32_t *iteration, *pop_node;
    int32_t *ended;
    float weight;
};

// the node beam slot i of problem p was popped from (a node of the pool by construction; clamped like k_advance's parents)
__device__ __forceinline__ int32_t popped(const MergeArgs &a, int64_t p, uint32_t i, int32_t count) {
    return min(max(a.pop_node[p * a.s.width + i], 0), count - 1);
}

template <class T>
__global__ void __launch_bounds__(kSelThreads) k_astar_merge(MergeArgs a) {
    using K = Key<T>;
    const Cands &s = a.s;
    const Pool &o = a.o;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    if (!s.active[p]) return;
    const int64_t g0 = p * o.cap;
    const uint32_t M = (uint32_t)min(max(s.live[p], 0), s.width) * T::A;
    const int32_t count = min(max(o.count[p], 1), o.cap);      // >= 1: the root; read by every thread before thread 0 writes it
    // 1. solved check: the smallest g(parent) + 1, then the lowest c
    uint64_t best = ~0ull;
    for (uint32_t c = tid; c < M; c += kSelThreads) {
        const uint8_t f = s.flags[cand_j<T>(s, p, c)];
        if ((f & RC_SEARCH_VALID) && (f & RC_SEARCH_SOLVED)) {
            const uint64_t v = ((uint64_t)(uint32_t)(o.g[g0 + popped(a, p, c / T::A, count)] + 1) << 32) | c;
            best = v < best ? v : best;
        }
    }
    best = block_reduce(best, Min{});
    if (best != ~0ull) {
        if (tid == 0) {
            const uint32_t c = (uint32_t)best;
            s.length[p] = (int32_t)(best >> 32);
            s.solution[2 * p] = popped(a, p, c / T::A, count);
            s.solution[2 * p + 1] = (int32_t)(c % T::A);
            s.active[p] = 0;
            a.ended[p] = *a.iteration;
        }
        return;
    }
    // 2. new candidates: the owner of its key's scratch slot (the lowest c with that key), and no node of this problem holds the key.
    //    Read-only on the persistent table; other problems' workgroups may be inserting (phase 3) meanwhile, which only turns empty
    //    slots into entries of THEIR nodes: skipped by the problem test before any key is loaded.  Nodes of p enter after the barrier.
    for (uint32_t c = tid; c < M; c += kSelThreads) {
        const int64_t j = cand_j<T>(s, p, c);
        const uint8_t f = s.flags[j];
        if (!(f & RC_SEARCH_VALID)) continue;
        uint64_t k[K::KW];
        if (!owns_key<T>(s, p, c, j, k)) continue;
        bool known = false;
        for (uint64_t h = slot_of<T>(k, p, o.tmask);; h = (h + 1) & o.tmask) {
            const uint64_t v = o.table[h];
            if (v == kEmpty) break;
            if ((int64_t)v >= g0 && (int64_t)v < g0 + count && node_has_key<T>(o, (int64_t)v, k)) {
                known = true;
                break;
            }
        }
        if (!known) s.flags[j] = f | RCA_NEW;
    }
    __syncthreads();
    // 3. append in ascending c: node count + r = the r-th new candidate, while the pool has room
    const uint32_t room = (uint32_t)(o.cap - count);
    const uint32_t nnew = ordered_compact(
        M, [&](uint32_t c) { return (s.flags[cand_j<T>(s, p, c)] & RCA_NEW) != 0; },
        [&](uint32_t c, uint32_t r) {
            if (r >= room) return;
            const int64_t j = cand_j<T>(s, p, c), gid = g0 + count + r;
            const int32_t par = popped(a, p, c / T::A, count);
            uint64_t k[K::KW];
            load_key<T>(s, j, k);
            // the child's stickers are its key's 3-bit fields; a centre (3x3x3) never moves: the parent's
            const uint8_t *src = o.stickers + tiled(g0 + par, o.ppitch, o.pshift, T::S);
            uint8_t *dst = o.stickers + tiled(gid, o.ppitch, o.pshift, T::S);
            sfor<T::S>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if constexpr (T::SIZE == 3 && i % 9 == 4) dst[(int64_t)i * o.ppitch] = src[(int64_t)i * o.ppitch];
                else {
                    constexpr int kk = T::SIZE == 3 ? (i / 9) * 8 + (i % 9 < 4 ? i % 9 : i % 9 - 1) : i;
                    static_assert(K::sticker(kk) == i);
                    dst[(int64_t)i * o.ppitch] = (uint8_t)((k[kk / 16] >> (3 * (kk % 16))) & 7u);
                }
            });
#pragma unroll
            for (int x = 0; x < K::KW; ++x) o.keys[(int64_t)x * o.np + gid] = k[x];
            const int32_t g = o.g[g0 + par] + 1;
            const float sc = s.scores[j];
            o.parent[gid] = par;
            o.action[gid] = (uint8_t)(c % T::A);
            o.g[gid] = g;
            o.score[gid] = sc;
            o.prio[gid] = prio_of(sc, a.weight, g);
            o.state[gid] = kOpen;
            table_put(o, slot_of<T>(k, p, o.tmask), gid);
        });
    if (tid == 0) {
        o.count[p] = count + (int32_t)min(nnew, room);
        if (nnew > room) o.overflow[p] = 1;
    }
}

__global__ void __launch_bounds__(256) k_astar_backtrack(const int32_t *parent, const uint8_t *action, int64_t n, int32_t cap, int A, int D,
                                                         const int32_t *length, const int32_t *solution, uint8_t *actions) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    for (int d = 0; d < D; ++d) actions[(int64_t)d * n + p] = (uint8_t)A;
    const int L = length[p];
    int32_t node = solution[2 * p];
    const int32_t act = solution[2 * p + 1];
    if (L < 1 || L > D || node < 0 || node >= cap || act < 0 || act >= A) return;
    actions[(int64_t)(L - 1) * n + p] = (uint8_t)act;
    for (int t = L - 1; t >= 1; --t) {                         // node has g = t: the move that made it is the solution's t-th
        actions[(int64_t)(t - 1) * n + p] = action[p * cap + node];
        node = parent[p * cap + node];
        if (node < 0 || node >= cap) return;
    }
}

// node indices, and gids p * C + n, are int32
bool pool_limits(int64_t n, int64_t capacity) {
    return n >= 1 && capacity >= 1 && n < ((int64_t)1 << 31) && capacity < ((int64_t)1 << 31) && n * capacity < ((int64_t)1 << 31);
}
const char kPoolLimits[] = "need n_problems >= 1, capacity >= 1 and n_problems * capacity < 2^31";

struct PoolGeo {
    int pshift;
    int64_t slots;
};
// the pool of P problems x C nodes at pool_pitch, and its table
template <class T>
int pool_geometry(int64_t n, int64_t capacity, int64_t pool_pitch, PoolGeo &g) {
    if (!pool_limits(n, capacity)) return fail(kPoolLimits);
    if ((g.pshift = tile_shift(pool_pitch, INT64_MAX, T::S)) < 0) return fail("pool_pitch must be a power of two >= 512 with S * pool_pitch < 2^32");
    g.slots = pow2_slots(2 * n * capacity);
    return 0;
}

Pool make_pool(uint8_t *stickers, uint64_t *keys, int32_t *parent, uint8_t *action, int32_t *g, float *score, float *prio, uint8_t *state,
               int32_t *count, uint8_t *overflow, void *table, const PoolGeo &pg, int64_t n, int64_t capacity, int64_t pool_pitch) {
    return Pool{stickers, keys, parent, action, g, score, prio, state, count, overflow, static_cast<unsigned long long *>(table),
                (uint64_t)(pg.slots - 1), n * capacity, pool_pitch, pg.pshift, (int32_t)capacity};
}

}  // namespace

int64_t rca_workspace_bytes(int cube_size, int64_t n_problems, int64_t capacity) {
    if ((cube_size != 2 && cube_size != 3) || !pool_limits(n_problems, capacity)) return -1;
    return pow2_slots(2 * n_problems * capacity) * 8;
}

int rca_init(const uint8_t *roots, int64_t n, int64_t root_pitch, int cube_size, int64_t capacity, int64_t pool_pitch, uint8_t *pool_stickers,
             uint64_t *pool_keys, int32_t *pool_parent, uint8_t *pool_action, int32_t *pool_g, float *pool_score, float *pool_prio,
             uint8_t *pool_state, int32_t *count, uint8_t *overflow, int32_t *live, uint8_t *active, int32_t *length, int32_t *solution,
             int32_t *ended, void *table, int64_t table_bytes, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        PoolGeo pg;
        if (int rc = pool_geometry<T>(n, capacity, pool_pitch, pg)) return rc;
        if (any_null(roots, pool_stickers, pool_keys, pool_parent, pool_action, pool_g, pool_score, pool_prio, pool_state, count, overflow, live,
                     active, length, solution, ended, table))
            return fail("rca_init: null buffer");
        if (!all_aligned16(roots, pool_stickers, pool_keys, pool_parent, pool_action, pool_g, pool_score, pool_prio, pool_state, count, overflow,
                           live, active, length, solution, ended, table))
            return fail("rca_init: buffers must be 16-byte aligned");
        if (table_bytes < pg.slots * 8) return fail("rca_init: table smaller than rca_workspace_bytes()");
        int rshift;
        if (int rc = root_shift<T>("rca_init", n, root_pitch, rshift)) return rc;
        const Pool o = make_pool(pool_stickers, pool_keys, pool_parent, pool_action, pool_g, pool_score, pool_prio, pool_state, count, overflow,
                                 table, pg, n, capacity, pool_pitch);
        if (int rc = fill16(table, pg.slots * 8, ~0u, ~0u, S(stream))) return rc;           // every slot kEmpty, once per search
        hipLaunchKernelGGL((k_astar_init<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), roots, n, root_pitch, rshift, o, live,
                           active, length, solution, ended);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rca_pop(int64_t n, int cube_size, int batch, int64_t capacity, int64_t pool_pitch, const uint8_t *pool_stickers, const uint8_t *pool_action,
            const float *pool_prio, uint8_t *pool_state, const int32_t *count, const int32_t *iteration, uint8_t *beam, int64_t pitch,
            uint8_t *last_action, int32_t *live, uint8_t *active, int32_t *ended, int32_t *pop_node, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        PoolGeo pg;
        if (int rc = geometry<T>(n, batch, pitch, g)) return rc;
        if (int rc = pool_geometry<T>(n, capacity, pool_pitch, pg)) return rc;
        if (any_null(pool_stickers, pool_action, pool_prio, pool_state, count, iteration, beam, last_action, live, active, ended, pop_node))
            return fail("rca_pop: null buffer");
        if (!all_aligned16(pool_stickers, pool_action, pool_prio, pool_state, count, iteration, beam, last_action, live, active, ended, pop_node))
            return fail("rca_pop: buffers must be 16-byte aligned");
        const PopArgs a{pool_stickers, pool_action, pool_prio, pool_state, count, pool_pitch, pg.pshift, (int32_t)capacity,
                        iteration, beam, last_action, live, active, ended, pop_node, pitch, g.shift, batch};
        hipLaunchKernelGGL((k_astar_pop<T>), dim3((unsigned)n), dim3(kSelThreads), 0, S(stream), a);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rca_merge(int64_t n, int cube_size, int batch, int64_t pitch, int64_t capacity, int64_t pool_pitch, float weight, uint8_t *flags,
              const uint64_t *keys, const float *scores, const int32_t *live, uint8_t *active, int32_t *length, int32_t *solution,
              int32_t *ended, const int32_t *iteration, const int32_t *pop_node, uint8_t *pool_stickers, uint64_t *pool_keys,
              int32_t *pool_parent, uint8_t *pool_action, int32_t *pool_g, float *pool_score, float *pool_prio, uint8_t *pool_state,
              int32_t *count, uint8_t *overflow, void *table, int64_t table_bytes, void *scratch, int64_t scratch_bytes, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        PoolGeo pg;
        if (int rc = geometry<T>(n, batch, pitch, g)) return rc;
        if (int rc = pool_geometry<T>(n, capacity, pool_pitch, pg)) return rc;
        if (!(weight >= 0.0f) || weight > 3.0e38f) return fail("rca_merge: weight must be finite and >= 0");
        if (any_null(flags, keys, scores, live, active, length, solution, ended, iteration, pop_node, pool_stickers, pool_keys, pool_parent,
                     pool_action, pool_g, pool_score, pool_prio, pool_state, count, overflow, table, scratch))
            return fail("rca_merge: null buffer");
        if (!all_aligned16(flags, keys, scores, live, active, length, solution, ended, iteration, pop_node, pool_stickers, pool_keys, pool_parent,
                           pool_action, pool_g, pool_score, pool_prio, pool_state, count, overflow, table, scratch))
            return fail("rca_merge: buffers must be 16-byte aligned");
        const int64_t sslots = table_slots(T::A, n, batch);
        if (table_bytes < pg.slots * 8) return fail("rca_merge: table smaller than rca_workspace_bytes()");
        if (scratch_bytes < sslots * 8) return fail("rca_merge: scratch smaller than rc_search_workspace_bytes()");
        const Cands s{flags, keys, scores, live, active, length, solution, static_cast<unsigned long long *>(scratch), (uint64_t)(sslots - 1),
                      g.nbp, batch};
        const MergeArgs a{s, make_pool(pool_stickers, pool_keys, pool_parent, pool_action, pool_g, pool_score, pool_prio, pool_state, count, overflow,
                                       table, pg, n, capacity, pool_pitch),
                          iteration, pop_node, ended, weight};
        if (int rc = fill16(scratch, sslots * 8, ~0u, ~0u, S(stream))) return rc;
        hipLaunchKernelGGL((k_insert<T>), dim3((unsigned)((T::A * g.nbp + 255) / 256)), dim3(256), 0, S(stream), s);
        RC_HIP(-2, hipGetLastError());
        hipLaunchKernelGGL((k_astar_merge<T>), dim3((unsigned)n), dim3(kSelThreads), 0, S(stream), a);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rca_backtrack(int64_t n, int cube_size, int64_t capacity, const int32_t *pool_parent, const uint8_t *pool_action, const int32_t *length,
                  const int32_t *solution, uint8_t *actions, int max_length, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        if (!pool_limits(n, capacity)) return fail(kPoolLimits);
        if (max_length < 1) return fail("rca_backtrack: max_length must be >= 1");
        if (any_null(pool_parent, pool_action, length, solution, actions)) return fail("rca_backtrack: null buffer");
        if (!all_aligned16(pool_parent, pool_action, length, solution, actions)) return fail("rca_backtrack: buffers must be 16-byte aligned");
        hipLaunchKernelGGL(k_astar_backtrack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), pool_parent, pool_action, n,
                           (int32_t)capacity, T::A, max_length, length, solution, actions);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

// =========================================================================================== corner pattern database
// The rcp_* entry points (include/rubiksearch.h "Corner pattern database", DESIGN.md "Corner pattern database"), on rc_device.h's
// corner coordinates (corners_of / corner_index_of: stickers -> index; corner_unrank / corner_move / corner_rank: the index space).
//
//   CornerLevels   the corner index space of a cube size under rc_table.h k_table_level: A neighbours per entry
//   k_pdb_unrank   index -> cubie rows, 4 cubes per lane (one dword per row; the ragged last pack byte by byte)
//   k_pdb_lookup   the 24 corner sticker rows (+ the 3 fixed ones of the 2x2x2) -> dist, 4 cubes per lane
//   k_pdb_score    4 consecutive key slots per lane -> their corner stickers as packed bytes -> scores
// Every table read goes through rc_table.h table_at with the compile-time table size N; corner_index_of gives all-ones for an illegal
// corner state, which the guard turns into 0xFF.
namespace {

template <class T>
struct CornerLevels {
    static constexpr int kNeighbours = T::A;
    __host__ __device__ static constexpr uint32_t n() { return CornerSpace<T>::N; }
    __device__ void block_begin() const {}
    __device__ CornerCoord unrank(uint32_t i) const { return corner_unrank<T>(i); }
    template <int A_>
    __device__ uint32_t neighbour(CornerCoord c) const { return corner_rank<T>(corner_move<T, A_>(c)); }
};

struct UnrankArgs {
    const uint32_t *index;
    int64_t n;
    uint8_t *cubies;
    int64_t pitch;
    int sh;
    uint8_t *bad;
};

template <class T>
__global__ void __launch_bounds__(256) k_pdb_unrank(UnrankArgs a) {
    const int64_t n0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (n0 >= a.n) return;
    const bool full = n0 + 4 <= a.n;
    uint32_t idx[4];
    load_index4(a.index, n0, a.n, full, 0u, idx);
    uint32_t row[T::SLOTS] = {};
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = idx[j] < CornerSpace<T>::N;
        bad = bad || !ok;
        const uint32_t ix = ok ? idx[j] : 0u;                             // out of range: the solved cube
        const CornerCoord c = corner_unrank<T>(ix);
        sfor<T::NC>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            row[q] |= (((c.piece >> (4 * q)) & 15u) * 3u + ((c.ori >> (4 * q)) & 3u)) << (8 * j);
        });
        if constexpr (T::NE > 0) {
            // the permutation's parity = the parity of its inversion count = that of the sum of the Lehmer digits
            uint32_t lehmer = ix / CornerSpace<T>::POW3, odd = 0;
            sfor<T::NC>([&](auto qc) {
                constexpr uint32_t radix = 1 + decltype(qc)::value;
                odd ^= lehmer % radix;
                lehmer /= radix;
            });
            odd &= 1u;
            sfor<T::NE>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                // an odd corner permutation needs an odd edge permutation: the last two edges trade places
                const uint32_t piece = e >= T::NE - 2 ? (uint32_t)e ^ (odd & (uint32_t)(((T::NE - 2) ^ (T::NE - 1)))) : (uint32_t)e;
                row[T::NC + e] |= (2u * piece) << (8 * j);
            });
        }
    }
    if (bad) *a.bad = 1;                                                  // every writer stores the same byte
    store_cubie_rows4(a.cubies, n0, a.n, full, a.pitch, a.sh, row);
}

// the 4 distances of a pack as bytes
template <class T>
__device__ __forceinline__ void pack_distances(const Corners<T, 1> &c, const uint8_t *table, uint32_t (&d)[4]) {
    sfor<4>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        d[j] = table_at(table, corner_index_of<T, 1, j>(c), CornerSpace<T>::N);
    });
}

struct LookupArgs {
    const uint8_t *st;
    int64_t n, pitch;
    int sh;
    const uint8_t *table;
    uint8_t *dist;
};

template <class T>
__global__ void __launch_bounds__(kWave) k_pdb_lookup(LookupArgs a) {
    const int64_t g0 = (int64_t)blockIdx.x * kSpan;
    const uint32_t lo = threadIdx.x * 4;
    const int64_t n0 = g0 + lo;
    if (n0 >= a.n) return;
    const __amdgpu_buffer_rsrc_t r = make_srd(a.st + tile_off(g0, a.pitch, a.sh, T::S));
    const uint32_t rs = (uint32_t)a.pitch;
    Pk<1> cc[T::NC][3], fixed = splat<1>(0);
    sfor<T::NC>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        sfor<3>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            cc[q][k] = bld<1, kAuxCached>(r, lo, (uint32_t)T::ccw[q][k] * rs);
        });
    });
    if constexpr (T::SIZE == 2)
        sfor<T::NFIX>([&](auto fc) {
            constexpr int i = T::fixed[decltype(fc)::value];
            fixed = fixed | (bld<1, kAuxCached>(r, lo, (uint32_t)i * rs) ^ solved_row<T, 1>(i));
        });
    Corners<T, 1> c;
    corners_of<T, 1>(cc, fixed, c);
    uint32_t d[4];
    pack_distances<T>(c, a.table, d);
    Pk<1> out;
    out.d[0] = d[0] | (d[1] << 8) | (d[2] << 16) | (d[3] << 24);
    st_tail<1>(a.dist, n0, a.n, out);
}

// where sticker i sits in a key: Key<T>::sticker's inverse (i is no centre)
template <class T>
constexpr int key_pos(int i) { return T::SIZE == 3 ? (i / 9) * 8 + (i % 9 < 4 ? i % 9 : i % 9 - 1) : i; }

template <class T>
__global__ void __launch_bounds__(256) k_pdb_score(const uint64_t *keys, int64_t total, const uint8_t *table, float *scores) {
    using K = Key<T>;
    const int64_t j0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;     // total % 4 == 0: a pack is whole or absent
    if (j0 >= total) return;
    uint64_t w[K::KW][4];
#pragma unroll
    for (int x = 0; x < K::KW; ++x)
#pragma unroll
        for (int j = 0; j < 4; ++j) w[x][j] = keys[(int64_t)x * total + j0 + j];
    const auto colour = [&](auto ic) {                                    // sticker i of the 4 slots as packed bytes
        constexpr int kk = key_pos<T>(decltype(ic)::value);
        static_assert(K::sticker(kk) == decltype(ic)::value);
        Pk<1> p;
        p.d[0] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) p.d[0] |= (uint32_t)((w[kk / 16][j] >> (3 * (kk % 16))) & 7u) << (8 * j);
        return p;
    };
    Pk<1> cc[T::NC][3], fixed = splat<1>(0);
    sfor<T::NC>([&](auto qc) {
        constexpr int q = decltype(qc)::value;
        sfor<3>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            cc[q][k] = colour(std::integral_constant<int, T::ccw[q][k]>{});
        });
    });
    if constexpr (T::SIZE == 2)
        sfor<T::NFIX>([&](auto fc) {
            constexpr int i = T::fixed[decltype(fc)::value];
            fixed = fixed | (colour(std::integral_constant<int, i>{}) ^ solved_row<T, 1>(i));
        });
    Corners<T, 1> c;
    corners_of<T, 1>(cc, fixed, c);
    uint32_t d[4];
    pack_distances<T>(c, table, d);
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const f32x4 s = {-(float)d[0], -(float)d[1], -(float)d[2], -(float)d[3]};
    *reinterpret_cast<f32x4 *>(scores + j0) = s;
}

// ---- rcp_relax: the step the A* rule leaves out, for an admissible table.  After rca_merge of an iteration, a VALID candidate that
// is not NEW names a state the pool knows.  If that node is still OPEN and the candidate reaches it by fewer moves, the node takes
// the candidate's g, parent, action and the prio that follows.  One workgroup per problem, three phases over the candidates
// c = tid + 256 r, each ending on a barrier, so that the winner among several candidates for one node is (least g, then least c) by
// rule: A lowers pool_g with atomicMin and marks the node (parent = INT_MIN, the same store from every writer); B: the candidates
// whose g the node now holds bid -(c + 2) into the marked parent with atomicMax; C: the one whose bid stands writes the node.
// Only this problem's workgroup touches this problem's nodes, and nothing inserts into the table meanwhile: it is read-only here.
struct RelaxArgs {
    Cands s;                      // flags, keys, live, active, nbp, width; the rest unused
    Pool o;                       // keys, parent, action, g, score, prio, state, count, table; the rest unused
    const int32_t *pop_node;
    float weight;
};

template <class T>
__global__ void __launch_bounds__(kSelThreads) k_pdb_relax(RelaxArgs a) {
    using K = Key<T>;
    const Cands &s = a.s;
    const Pool &o = a.o;
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    if (!s.active[p]) return;                                  // ended in this iteration's pop or merge: nothing to improve
    const int64_t g0 = p * o.cap;
    const uint32_t M = (uint32_t)min(max(s.live[p], 0), s.width) * T::A;
    const int32_t count = min(max(o.count[p], 1), o.cap);
    constexpr int32_t kMark = INT32_MIN;
    // the OPEN node of this problem that holds candidate c's key and the g the candidate offers; -1: none, or nothing to gain
    const auto target = [&](uint32_t c, int32_t &newg) -> int64_t {
        const int64_t j = cand_j<T>(s, p, c);
        const uint8_t f = s.flags[j];
        if (!(f & RC_SEARCH_VALID) || (f & RCA_NEW)) return -1;
        const int32_t par = min(max(a.pop_node[p * s.width + c / T::A], 0), count - 1);
        newg = o.g[g0 + par] + 1;                              // the parent is CLOSED: its g does not move
        uint64_t k[K::KW];
        load_key<T>(s, j, k);
        for (uint64_t h = slot_of<T>(k, p, o.tmask);; h = (h + 1) & o.tmask) {
            const uint64_t v = o.table[h];
            if (v == kEmpty) return -1;
            if ((int64_t)v >= g0 && (int64_t)v < g0 + count && node_has_key<T>(o, (int64_t)v, k)) return o.state[v] == kOpen ? (int64_t)v : -1;
        }
    };
    for (uint32_t c = tid; c < M; c += kSelThreads) {          // A
        int32_t newg;
        const int64_t v = target(c, newg);
        if (v >= 0 && atomicMin(&o.g[v], newg) > newg) o.parent[v] = kMark;
    }
    __syncthreads();
    for (uint32_t c = tid; c < M; c += kSelThreads) {          // B
        int32_t newg;
        const int64_t v = target(c, newg);
        if (v >= 0 && o.g[v] == newg && o.parent[v] < -1) atomicMax(&o.parent[v], -(int32_t)c - 2);
    }
    __syncthreads();
    for (uint32_t c = tid; c < M; c += kSelThreads) {          // C
        int32_t newg;
        const int64_t v = target(c, newg);
        if (v < 0 || o.parent[v] != -(int32_t)c - 2) continue;
        o.parent[v] = min(max(a.pop_node[p * s.width + c / T::A], 0), count - 1);
        o.action[v] = (uint8_t)(c % T::A);
        o.prio[v] = prio_of(o.score[v], a.weight, newg);
    }
}

template <class T>
int corner_table_arg(const char *fn, const void *table, int64_t bytes) {
    return table_arg(fn, table, bytes, CornerSpace<T>::N, "rcp_table_bytes()");
}

}  // namespace

int64_t rcp_table_bytes(int cube_size) {
    return cube_size == 3 ? (int64_t)CornerSpace<Cube3>::N : cube_size == 2 ? (int64_t)CornerSpace<Cube2>::N : -1;
}

int rcp_tables(int cube_size, uint8_t *src, uint8_t *twist) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        if (src) memcpy(src, T::cmove_src, (size_t)T::A * T::NC);
        if (twist) memcpy(twist, T::cmove_twist, (size_t)T::A * T::NC);
        return 0;
    });
}

int rcp_build_begin(uint8_t *table, int64_t bytes, int cube_size, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        if (int rc = corner_table_arg<T>("rcp_build_begin", table, bytes)) return rc;
        static_assert(CornerSpace<T>::N % 16 == 0, "the table is filled 16 bytes at a time");
        return fill16(table, (int64_t)CornerSpace<T>::N, ~0u, 0xFFFFFF00u, S(stream));   // every entry 0xFF; corner_index(solved) = 0: byte 0 is 0
    });
}

int rcp_build_level(uint8_t *table, int64_t bytes, int cube_size, int depth, uint32_t *count, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        if (int rc = corner_table_arg<T>("rcp_build_level", table, bytes)) return rc;
        return table_build_level("rcp_build_level", table, CornerLevels<T>{}, depth, count, S(stream), -2);
    });
}

int rcp_unrank(const uint32_t *index, int64_t n, int cube_size, uint8_t *cubies, int64_t cubie_pitch, uint8_t *bad, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        if (n < 0) return fail("rcp_unrank: n is negative");
        if (!index || !aligned16(index)) return fail("rcp_unrank: index is NULL or not 16-byte aligned");
        if (!cubies || !aligned16(cubies)) return fail("rcp_unrank: cubies is NULL or not 16-byte aligned");
        const int sh = tile_shift(cubie_pitch, n, T::SLOTS);
        if (sh < 0) return fail("rcp_unrank: cubie_pitch: need pitch % 16 == 0 and pitch >= n, or a power-of-two tile >= 512");
        if (!bad) return fail("rcp_unrank: bad is NULL");
        if (n == 0) return 0;
        const int64_t blocks = ceil_div(n, 1024);
        if (!grid_ok(blocks)) return fail("rcp_unrank: too many cubes for one launch");
        const UnrankArgs a{index, n, cubies, cubie_pitch, sh, bad};
        hipLaunchKernelGGL((k_pdb_unrank<T>), dim3((unsigned)blocks), dim3(256), 0, S(stream), a);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rcp_lookup(const uint8_t *stp, int64_t n, int64_t pitch, int cube_size, const uint8_t *table, int64_t bytes, uint8_t *dist,
               void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        if (n < 0) return fail("rcp_lookup: n_cubes is negative");
        if (!stp || !aligned16(stp)) return fail("rcp_lookup: st is NULL or not 16-byte aligned");
        const int sh = tile_shift(pitch, n, T::S);
        if (sh < 0) return fail("rcp_lookup: pitch: need pitch % 16 == 0 and pitch >= n_cubes, or a power-of-two tile >= 512");
        if (int rc = corner_table_arg<T>("rcp_lookup", table, bytes)) return rc;
        if (!dist || !aligned16(dist)) return fail("rcp_lookup: dist is NULL or not 16-byte aligned");
        if (n == 0) return 0;
        const int64_t blocks = ceil_div(n, kSpan);
        if (!grid_ok(blocks)) return fail("rcp_lookup: too many cubes for one launch");
        const LookupArgs a{stp, n, pitch, sh, table, dist};
        hipLaunchKernelGGL((k_pdb_lookup<T>), dim3((unsigned)blocks), dim3(kWave), 0, S(stream), a);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rcp_score_keys(const uint64_t *keys, int64_t n, int width, int64_t pitch, int cube_size, const uint8_t *table, int64_t bytes,
                   float *scores, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        if (int rc = geometry<T>(n, width, pitch, g)) return rc;
        if (!keys || !aligned16(keys)) return fail("rcp_score_keys: keys is NULL or not 16-byte aligned");
        if (int rc = corner_table_arg<T>("rcp_score_keys", table, bytes)) return rc;
        if (!scores || !aligned16(scores)) return fail("rcp_score_keys: scores is NULL or not 16-byte aligned");
        const int64_t total = (int64_t)T::A * g.nbp;                       // a multiple of 512
        hipLaunchKernelGGL((k_pdb_score<T>), dim3((unsigned)ceil_div(total, 1024)), dim3(256), 0, S(stream), keys, total, table, scores);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rcp_relax(int64_t n, int cube_size, int batch, int64_t pitch, int64_t capacity, float weight, const uint8_t *flags, const uint64_t *keys,
              const int32_t *live, const uint8_t *active, const int32_t *pop_node, const uint64_t *pool_keys, int32_t *pool_parent,
              uint8_t *pool_action, int32_t *pool_g, const float *pool_score, float *pool_prio, const uint8_t *pool_state, const int32_t *count,
              const void *table, int64_t table_bytes, void *stream) {
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        Geo g;
        if (int rc = geometry<T>(n, batch, pitch, g)) return rc;
        if (!pool_limits(n, capacity)) return fail(kPoolLimits);
        if (!(weight >= 0.0f) || weight > 3.0e38f) return fail("rcp_relax: weight must be finite and >= 0");
        if (any_null(flags, keys, live, active, pop_node, pool_keys, pool_parent, pool_action, pool_g, pool_score, pool_prio, pool_state, count, table))
            return fail("rcp_relax: null buffer");
        if (!all_aligned16(flags, keys, live, active, pop_node, pool_keys, pool_parent, pool_action, pool_g, pool_score, pool_prio, pool_state, count,
                           table))
            return fail("rcp_relax: buffers must be 16-byte aligned");
        const int64_t slots = pow2_slots(2 * n * capacity);
        if (table_bytes < slots * 8) return fail("rcp_relax: table smaller than rca_workspace_bytes()");
        RelaxArgs a{};
        a.s.flags = const_cast<uint8_t *>(flags);              // read only here
        a.s.keys = keys;
        a.s.live = live;
        a.s.active = const_cast<uint8_t *>(active);
        a.s.nbp = g.nbp;
        a.s.width = batch;
        a.o.keys = const_cast<uint64_t *>(pool_keys);
        a.o.parent = pool_parent;
        a.o.action = pool_action;
        a.o.g = pool_g;
        a.o.score = const_cast<float *>(pool_score);
        a.o.prio = pool_prio;
        a.o.state = const_cast<uint8_t *>(pool_state);
        a.o.count = const_cast<int32_t *>(count);
        a.o.table = static_cast<unsigned long long *>(const_cast<void *>(table));
        a.o.tmask = (uint64_t)(slots - 1);
        a.o.np = n * capacity;
        a.o.cap = (int32_t)capacity;
        a.pop_node = pop_node;
        a.weight = weight;
        hipLaunchKernelGGL((k_pdb_relax<T>), dim3((unsigned)n), dim3(kSelThreads), 0, S(stream), a);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

// the cube symmetries (include/rubiksym.h): the rcs_* entry points of this library
#include "rc_sym.h"
