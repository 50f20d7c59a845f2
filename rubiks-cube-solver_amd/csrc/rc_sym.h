// rc_sym.h -- the cube symmetries on the device (include/rubiksym.h), the last part of rc_search.hip's translation unit: it uses
// that file's fail, rc_host.h and rc_device.h, and adds the rcs_* entry points to librubiksearch.so.
// The rule (rc_sym_tables.h): image[i] = relabel[s][ state[ perm[s][i] ] ].  DESIGN.md "Symmetries" has the byte and LDS models.
//
//   k_sym_uniform   one symmetry for every cube: the image is a ROW permutation of the tile.  One lane = 8 cubes; output row i is
//                   the input row perm[s][i], loaded at a scalar row offset, recoloured by one v_perm_b32 per dword against the
//                   6-entry relabel table held in two SGPRs (the sticker bytes are the selector), and stored.  The symmetry's
//                   perm row and relabel row travel in the kernel arguments: no table is read from memory.
//   k_sym_cubes     one symmetry per cube (MODE 0) or the canonical form (MODE 1).  A workgroup of 2 waves stages its 512-cube
//                   sticker block [S][512] and the K x S perm / K x 8 relabel tables in LDS; a lane gathers its own 4 cubes
//                   byte by byte (a lane only ever reads the columns it wrote: the sticker block needs no barrier, the tables
//                   one) and stores coalesced packs.  The canonical search walks s = 1 .. K-1 with the running best kept as an
//                   index per cube: the candidate row is ONE packed LDS read (s is uniform), the best's row is re-read through
//                   its index, and the comparison of a wave stops at the first row that decides all of its cubes.
#pragma once

#include "../../include/rubiksym.h"
#include "rc_sym_tables.h"

namespace {

constexpr int kSymSpan = 512;                    // cubes per workgroup of both kernels = the smallest tile: never straddles tiles

template <class T> struct SymOf;
template <> struct SymOf<Cube3> { using type = Sym3; };
template <> struct SymOf<Cube2> { using type = Sym2; };

struct SymArgs {
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *sym;      // k_sym_cubes MODE 0
    uint8_t *sym_out, *bad;  // MODE 1 / MODE 0
    int64_t n, pitch_in, pitch_out;
    int sh_in, sh_out;
};

// ------------------------------------------------------------------------------------------ one symmetry for all
template <class T>
struct SymRow {
    uint32_t perm[SymOf<T>::type::PW];   // perm[s] as bytes
    uint32_t rel[2];                     // relabel[s] as 8 bytes
};

template <class T, int POL>
__global__ void __launch_bounds__(kWave) k_sym_uniform(SymArgs a, SymRow<T> row) {
    constexpr int V = 2;
    static_assert(kWave * 4 * V == kSymSpan);
    using P = RowPolicy<POL>;                      // 0 / 1 / 2 by rc_host.h mall_policy
    const int64_t g0 = (int64_t)blockIdx.x * kSymSpan;
    const uint32_t lo = threadIdx.x * (4 * V);
    const int64_t n0 = g0 + lo;
    if (n0 >= a.n) return;
    const __amdgpu_buffer_rsrc_t rin = make_srd(a.in + tile_off(g0, a.pitch_in, a.sh_in, T::S));
    const __amdgpu_buffer_rsrc_t rout = make_srd(a.out + tile_off(g0, a.pitch_out, a.sh_out, T::S));
    const uint32_t pi = (uint32_t)a.pitch_in, po = (uint32_t)a.pitch_out;
    if (n0 + 4 * V <= a.n) {
        // every load before the first store, as the step kernel does: a store between two loads would order them (the compiler
        // cannot know that the buffers do not overlap) and leave one row in flight per wave
        Pk<V> img[T::S];
        sfor<T::S>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const uint32_t src = (row.perm[i / 4] >> (8 * (i % 4))) & 0xffu;                 // scalar
            img[i] = bld<V, P::LD>(rin, lo, src * pi);
        });
#pragma unroll
        for (int i = 0; i < T::S; ++i) bst<V, P::ST>(rout, lo, i * po, perm<V>(row.rel[1], row.rel[0], img[i]));
    } else {                                                                                 // the ragged last pack: pad columns keep their bytes
        Pk<V> keep;
        RC_V keep.d[k] = pack_valid(a.n - n0, k);
        sfor<T::S>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            const uint32_t src = (row.perm[i / 4] >> (8 * (i % 4))) & 0xffu;
            const Pk<V> img = perm<V>(row.rel[1], row.rel[0], bld<V, P::LD>(rin, lo, src * pi));
            bst<V, kAuxCached>(rout, lo, i * po, sel(keep, img, bld<V, kAuxCached>(rout, lo, i * po)));
        });
    }
}

// --------------------------------------------------------------------------- one symmetry per cube / canonical form
template <class Y>
struct SymDev {
    uint32_t perm[Y::K * Y::PW];
    uint32_t rel[Y::K * 2];
};
template <class Y>
constexpr SymDev<Y> make_sym_dev() {
    SymDev<Y> d{};
    for (int s = 0; s < Y::K; ++s) {
        for (int w = 0; w < Y::PW; ++w) d.perm[s * Y::PW + w] = Y::perm_dw[s][w];
        d.rel[2 * s] = Y::relabel_dw[s][0];
        d.rel[2 * s + 1] = Y::relabel_dw[s][1];
    }
    return d;
}
__constant__ SymDev<Sym3> g_sym3 = make_sym_dev<Sym3>();
__constant__ SymDev<Sym2> g_sym2 = make_sym_dev<Sym2>();

// byte q of t[q], q = 0..3: four look-ups of one packed dword, each cube under its own table
__device__ __forceinline__ uint32_t sym_pick(const uint32_t (&t)[4]) {
    const uint32_t l = (t[0] & 0x000000ffu) | (t[1] & ~0x000000ffu), h = (t[2] & 0x00ff0000u) | (t[3] & ~0x00ff0000u);
    return (l & 0x0000ffffu) | (h & ~0x0000ffffu);
}

constexpr int kSymThreads = kSymSpan / 4;        // 128: one lane = one pack of 4 cubes

template <class T, int MODE, int POL>
__global__ void __launch_bounds__(kSymThreads) k_sym_cubes(SymArgs a) {
    using Y = typename SymOf<T>::type;
    using P = RowPolicy<POL>;                      // 0 / 1 / 2 by rc_host.h mall_policy
    constexpr int PW = Y::PW, K = Y::K;
    __shared__ uint32_t s_st[T::S * kSymSpan / 4];    // [S][512] sticker bytes: row i of the lane's pack is dword i * 128 + tid
    __shared__ uint32_t s_perm[K * PW];
    __shared__ uint32_t s_rel[K * 2];
    const uint8_t *st8 = reinterpret_cast<const uint8_t *>(s_st);
    const uint8_t *perm8 = reinterpret_cast<const uint8_t *>(s_perm);
    const SymDev<Y> &dev = [&]() -> const SymDev<Y> & { if constexpr (T::SIZE == 3) return g_sym3; else return g_sym2; }();
    const uint32_t tid = threadIdx.x, lo = tid * 4;
    const int64_t g0 = (int64_t)blockIdx.x * kSymSpan, n0 = g0 + lo;
    for (uint32_t t = tid; t < K * PW; t += kSymThreads) s_perm[t] = dev.perm[t];
    for (uint32_t t = tid; t < K * 2; t += kSymThreads) s_rel[t] = dev.rel[t];
    const uint32_t valid = n0 < a.n ? pack_valid(a.n - n0, 0) : 0u;
    if (valid) {
        // stickers are 0..5: the mask keeps whatever else a buffer holds (pad columns, a caller's garbage) inside the 8-entry
        // look-ups and the packed byte comparisons below
        const __amdgpu_buffer_rsrc_t rin = make_srd(a.in + tile_off(g0, a.pitch_in, a.sh_in, T::S));
        const uint32_t pi = (uint32_t)a.pitch_in;
#pragma unroll
        for (int i = 0; i < T::S; ++i) s_st[i * (kSymSpan / 4) + tid] = bld<1, P::LD>(rin, lo, i * pi).d[0] & valid & 0x07070707u;
    }
    __syncthreads();                                  // the tables; the sticker columns are the lane's own
    if (!valid) return;

    uint32_t sy = 0;                                  // the pack's four symmetry indices, every byte < K
    if constexpr (MODE == 0) {
        const uint32_t raw = ld_tail<1>(a.sym, n0, a.n, 0).d[0] & valid;
        bool bad = false;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t sq = (raw >> (8 * q)) & 0xffu;
            if (sq >= (uint32_t)K) bad = true;        // the identity for that cube
            else sy |= sq << (8 * q);
        }
        if (bad && a.bad) *a.bad = 1;
    } else {
        constexpr uint32_t H = 0x80808080u;
        for (int s = 1; s < K; ++s) {
            const uint32_t cr0 = s_rel[2 * s], cr1 = s_rel[2 * s + 1];
            uint32_t br0[4], br1[4], bp[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t bq = (sy >> (8 * q)) & 0xffu;
                br0[q] = s_rel[2 * bq];
                br1[q] = s_rel[2 * bq + 1];
                bp[q] = bq * (4 * PW);
            }
            uint32_t open = H, win = 0;               // bit 7 of byte q: cube q is undecided / image s is the smaller one
            for (int i = 0; i < T::S; ++i) {
                const uint32_t c = __builtin_amdgcn_perm(cr1, cr0, s_st[(uint32_t)perm8[s * (4 * PW) + i] * (kSymSpan / 4) + tid]);
                uint32_t w = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) w |= (uint32_t)st8[(uint32_t)perm8[bp[q] + i] * kSymSpan + lo + q] << (8 * q);
                uint32_t t[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] = __builtin_amdgcn_perm(br1[q], br0[q], w);
                const uint32_t b = sym_pick(t);
                const uint32_t ge = ((c | H) - b) & H;                      // bytes are 0..5: no borrow crosses a byte
                const uint32_t ne = ((c ^ b) + 0x7f7f7f7fu) & H;
                win |= open & ~ge;
                open &= ~ne;
                if (__ballot(open != 0) == 0) break;                        // every cube of the wave is decided
            }
            const uint32_t m = (win >> 7) * 0xffu;
            sy = (((uint32_t)s * 0x01010101u) & m) | (sy & ~m);
        }
        Pk<1> so;
        so.d[0] = sy;
        st_tail<1>(a.sym_out, n0, a.n, so);
        if (!a.out) return;
    }

    // the image of each cube under its own symmetry: S x 4 byte reads of the lane's columns, one coalesced pack store per row
    uint32_t r0[4], r1[4], po4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t sq = (sy >> (8 * q)) & 0xffu;
        r0[q] = s_rel[2 * sq];
        r1[q] = s_rel[2 * sq + 1];
        po4[q] = sq * PW;
    }
    const __amdgpu_buffer_rsrc_t rout = make_srd(a.out + tile_off(g0, a.pitch_out, a.sh_out, T::S));
    const uint32_t po = (uint32_t)a.pitch_out;
    const bool full = valid == 0xffffffffu;
    Pk<1> keep;
    keep.d[0] = valid;
    uint32_t pd[4] = {0, 0, 0, 0};
    sfor<T::S>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        if constexpr (i % 4 == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) pd[q] = s_perm[po4[q] + i / 4];
        }
        uint32_t w = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) w |= (uint32_t)st8[((pd[q] >> (8 * (i % 4))) & 0xffu) * kSymSpan + lo + q] << (8 * q);
        uint32_t t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = __builtin_amdgcn_perm(r1[q], r0[q], w);
        Pk<1> img;
        img.d[0] = sym_pick(t);
        store_row<1, P::ST>(rout, lo, i * po, img, full, keep);                // the ragged last pack: pad columns keep their bytes
    });
}

// ------------------------------------------------------------------------------------------------- host side
// bytes from the buffer's start to the end of the last pack a kernel touches (packs of 8 cubes at most; pitch % 16 == 0)
inline int64_t sym_extent(int64_t n, int64_t pitch, int shift, int rows) {
    const int64_t last = ((n + 7) & ~(int64_t)7) - 1;
    const int64_t tile = shift >= 63 ? 0 : last >> shift;
    return tile * rows * pitch + (int64_t)(rows - 1) * pitch + (last - tile * pitch) + 1;
}

inline bool sym_overlap(const uint8_t *a, int64_t na, const uint8_t *b, int64_t nb) { return a < b + nb && b < a + na; }

template <class T>
int sym_host_tables(uint8_t *perm, uint8_t *relabel, uint8_t *amap, uint8_t *inverse, uint8_t *compose) {
    using Y = typename SymOf<T>::type;
    if (perm) memcpy(perm, Y::perm, sizeof Y::perm);
    if (relabel) memcpy(relabel, Y::relabel, sizeof Y::relabel);
    if (amap) memcpy(amap, Y::amap, sizeof Y::amap);
    if (inverse) memcpy(inverse, Y::inverse, sizeof Y::inverse);
    if (compose) memcpy(compose, Y::compose, sizeof Y::compose);
    return 0;
}

// the checks rcs_sym_apply and rcs_sym_canonical share; fills the layout fields of `a`
template <class T>
int sym_check(const char *fn, SymArgs &a, bool need_out) {
    if (a.n < 0) return fail(fn, "n_cubes is negative");
    if (!a.in || !aligned16(a.in)) return fail(fn, "in is NULL or not 16-byte aligned");
    if ((a.sh_in = tile_shift(a.pitch_in, a.n, T::S)) < 0)
        return fail(fn, "bad pitch_in: need pitch % 16 == 0 and pitch >= n_cubes, or a power-of-two tile >= 512, and S * pitch < 2^32");
    if (need_out && !a.out) return fail(fn, "out is NULL");
    if (!a.out) return 0;
    if (!aligned16(a.out)) return fail(fn, "out is not 16-byte aligned");
    if ((a.sh_out = tile_shift(a.pitch_out, a.n, T::S)) < 0)
        return fail(fn, "bad pitch_out: need pitch % 16 == 0 and pitch >= n_cubes, or a power-of-two tile >= 512, and S * pitch < 2^32");
    if (a.in == a.out) return fail(fn, "in == out: the image is not computed in place");
    if (a.n > 0 && sym_overlap(a.in, sym_extent(a.n, a.pitch_in, a.sh_in, T::S), a.out, sym_extent(a.n, a.pitch_out, a.sh_out, T::S)))
        return fail(fn, "in and out overlap");
    return 0;
}

template <class T, int MODE>
int sym_launch_cubes(const SymArgs &a, hipStream_t st) {
    const int64_t blocks = ceil_div(a.n, kSymSpan);
    RC_GRID(blocks);
    const dim3 g((unsigned)blocks), b(kSymThreads);
    const int pol = mall_policy(a.n * T::S, a.out ? a.n * T::S : 0);
    if (pol == 0) hipLaunchKernelGGL((k_sym_cubes<T, MODE, 0>), g, b, 0, st, a);
    else if (pol == 1) hipLaunchKernelGGL((k_sym_cubes<T, MODE, 1>), g, b, 0, st, a);
    else hipLaunchKernelGGL((k_sym_cubes<T, MODE, 2>), g, b, 0, st, a);
    RC_HIP(-2, hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int rcs_sym_count(int cube_size) { return cube_size == 3 ? Sym3::K : cube_size == 2 ? Sym2::K : -1; }

int rcs_sym_tables(int cube_size, uint8_t *perm, uint8_t *relabel, uint8_t *amap, uint8_t *inverse, uint8_t *compose) {
    return by_size(cube_size, [&](auto t) { return sym_host_tables<decltype(t)>(perm, relabel, amap, inverse, compose); });
}

int rcs_sym_apply(const uint8_t *in, uint8_t *out, int64_t n, int64_t pitch_in, int64_t pitch_out, int cube_size, const uint8_t *sym,
                  int sym_uniform, uint8_t *bad, void *stream) {
    static const char fn[] = "rcs_sym_apply";
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        using Y = typename SymOf<T>::type;
        SymArgs a{in, out, sym, nullptr, bad, n, pitch_in, pitch_out, 63, 63};
        if (int rc = sym_check<T>(fn, a, true)) return rc;
        if (sym && !aligned16(sym)) return fail(fn, "sym is not 16-byte aligned");
        if (!sym && (sym_uniform < 0 || sym_uniform >= Y::K)) return fail(fn, "sym_uniform is outside 0..K-1");
        if (n == 0) return 0;
        if (sym) return sym_launch_cubes<T, 0>(a, S(stream));
        SymRow<T> row;
        memcpy(row.perm, Y::perm_dw[sym_uniform], sizeof row.perm);
        memcpy(row.rel, Y::relabel_dw[sym_uniform], sizeof row.rel);
        const int64_t blocks = ceil_div(n, kSymSpan);
        RC_GRID(blocks);
        const dim3 g((unsigned)blocks), b(kWave);
        const int pol = mall_policy(n * T::S, n * T::S);
        if (pol == 0) hipLaunchKernelGGL((k_sym_uniform<T, 0>), g, b, 0, S(stream), a, row);
        else if (pol == 1) hipLaunchKernelGGL((k_sym_uniform<T, 1>), g, b, 0, S(stream), a, row);
        else hipLaunchKernelGGL((k_sym_uniform<T, 2>), g, b, 0, S(stream), a, row);
        RC_HIP(-2, hipGetLastError());
        return 0;
    });
}

int rcs_sym_canonical(const uint8_t *in, int64_t n, int64_t pitch_in, int cube_size, uint8_t *sym_out, uint8_t *out, int64_t pitch_out,
                      void *stream) {
    static const char fn[] = "rcs_sym_canonical";
    return by_size(cube_size, [&](auto t) {
        using T = decltype(t);
        SymArgs a{in, out, nullptr, sym_out, nullptr, n, pitch_in, pitch_out, 63, 63};
        if (int rc = sym_check<T>(fn, a, false)) return rc;
        if (!sym_out || !aligned16(sym_out)) return fail(fn, "sym_out is NULL or not 16-byte aligned");
        if (n == 0) return 0;
        return sym_launch_cubes<T, 1>(a, S(stream));
    });
}

}  // extern "C"
