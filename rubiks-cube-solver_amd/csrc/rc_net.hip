// rc_net.hip -- kernel and C ABI of librubiknet.so (include/rubiknet.h): the value net's first layer as a sum of table rows picked
// by the compact code (DESIGN.md "Net front").  gfx950 only, wave64.
//
//   k_first_layer  grid = column slabs x state ranges.  A workgroup copies its slab of the transposed weight -- all R * C rows x
//                  64 columns, widened to fp32 (256 bytes per row) -- into LDS once and keeps it while it walks its range of states
//                  in passes of 1024.  Per pass the workgroup fetches the code bytes once (one state per thread, coalesced rows) and
//                  stages them in LDS; then 16 lanes own one state and 4 columns each: SLOTS ds_read_b128 (a wave reads four
//                  256-byte rows, every 16-lane group its row's consecutive columns: conflict-free) and SLOTS fp32 additions per
//                  column IN SLOT ORDER, the activation, one rounding, one 16- or 8-byte store.  There is no multiplication.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/rubiknet.h"
#include "rc_host.h"

namespace {

constexpr int kThreads = 1024;                   // 16 waves, four per SIMD: one workgroup per CU at 3x3x3 (LDS), at most 128 VGPRs
constexpr int kPass = 1024;                      // states per pass = one per thread when the codes are fetched
constexpr int kRowBytes = 256;                   // one table row of a slab in LDS: every LDS bank once
constexpr int kLanes = 16;                       // lanes per state, 16 bytes of the row each
constexpr int kV = 4;                            // columns per lane
constexpr int kCols = kLanes * kV;               // columns per slab
constexpr int kGroup = 64 / kLanes * (kThreads / 64);   // states the workgroup sums at a time (4 per wave)

// Per cube size: the one-hot's geometry and how a code byte is staged.  The staged byte v and the slot's base give the row
// k = base(s) + v (include/rubiknet.h); out-of-range codes are clamped so that k stays below ROWS.
struct Net3 {
    static constexpr int SIZE = 3, SLOTS = 20, ROWS = 480, WORDS = 5, STAGE = 32;    // STAGE: bytes per state in LDS (16-byte multiple)
    static __device__ __forceinline__ uint32_t stage(int, uint32_t c) { return c < 24u ? c : 23u; }
    static constexpr int base(int s) { return s * 24; }
};
struct Net2 {
    static constexpr int SIZE = 2, SLOTS = 7, ROWS = 147, WORDS = 2, STAGE = 8;
    static __device__ __forceinline__ uint32_t stage(int s, uint32_t c) {
        c = c < 21u ? c : 20u;
        const uint32_t piece = c / 3u;
        return piece * 21u + (uint32_t)s * 3u + (c - piece * 3u);
    }
    static constexpr int base(int) { return 0; }
};

struct bf16_t { uint16_t bits; };

__device__ __forceinline__ uint32_t f32_to_bf16(float f) {               // round to nearest even; NaN -> quiet NaN of the same sign
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x0040u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// 4 consecutive elements of the weight or the bias as fp32 (bf16 widens exactly)
__device__ __forceinline__ uint4 load4(const float *p) { return *reinterpret_cast<const uint4 *>(p); }
__device__ __forceinline__ uint4 load4(const bf16_t *p) {
    const uint2 q = *reinterpret_cast<const uint2 *>(p);
    return make_uint4(q.x << 16, q.x & 0xffff0000u, q.y << 16, q.y & 0xffff0000u);
}
__device__ __forceinline__ void store4(float *p, const float *a) { *reinterpret_cast<float4 *>(p) = make_float4(a[0], a[1], a[2], a[3]); }
__device__ __forceinline__ void store4(bf16_t *p, const float *a) {
    *reinterpret_cast<uint2 *>(p) = make_uint2(f32_to_bf16(a[0]) | f32_to_bf16(a[1]) << 16, f32_to_bf16(a[2]) | f32_to_bf16(a[3]) << 16);
}

struct Args {
    const uint8_t *code;
    const void *wt, *bias;
    void *out;
    int64_t n, pitch, out_stride, passes, passes_per_block;
    int shift, hidden, act;                      // shift 63: one tile
};

template <class T>
__device__ __forceinline__ void fetch_codes(const Args &a, int64_t g, uint32_t (&c)[T::SLOTS]) {
    if (g < a.n) {
        const uint8_t *p = a.code + (a.shift >= 63 ? g : (g >> a.shift) * T::SLOTS * a.pitch + (g & (a.pitch - 1)));
#pragma unroll
        for (int s = 0; s < T::SLOTS; ++s) c[s] = p[(int64_t)s * a.pitch];
    } else {
#pragma unroll
        for (int s = 0; s < T::SLOTS; ++s) c[s] = 0;
    }
}

template <class T>
__device__ __forceinline__ void read_staged(const uint32_t *staged, int st, uint32_t (&w)[T::WORDS]) {
    const uint32_t *src = staged + st * (T::STAGE / 4);
    if (T::SIZE == 3) {
        const uint4 q = *reinterpret_cast<const uint4 *>(src);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        w[T::WORDS - 1] = src[T::WORDS - 1];
    } else {
        const uint2 q = *reinterpret_cast<const uint2 *>(src);
        w[0] = q.x; w[1] = q.y;
    }
}

template <class T, class W, class O>
__global__ void __launch_bounds__(kThreads) k_first_layer(Args a) {
    __shared__ __attribute__((aligned(16))) uint8_t slab[T::ROWS * kRowBytes];
    __shared__ __attribute__((aligned(16))) uint32_t staged[kPass * T::STAGE / 4];
    const int tid = threadIdx.x;
    const int64_t h0 = (int64_t)blockIdx.x * kCols;

    // the slab: row r of LDS = float(wt[r][h0 .. h0 + 64)); columns past `hidden` (the last slab) are zeros and are never stored
    for (int i = tid; i < T::ROWS * kLanes; i += kThreads) {
        const int64_t col = h0 + (i & (kLanes - 1)) * kV;
        uint4 q = make_uint4(0, 0, 0, 0);
        if (col < a.hidden) q = load4(static_cast<const W *>(a.wt) + (int64_t)(i >> 4) * a.hidden + col);
        reinterpret_cast<uint4 *>(slab)[i] = q;
    }

    const int lane = tid & 63, cl = lane & (kLanes - 1);
    const int first = (tid >> 6) * (64 / kLanes) + (lane >> 4);          // this lane's state within a group of kGroup
    const int64_t col = h0 + cl * kV;
    const bool col_ok = col < a.hidden;
    uint4 acc0 = make_uint4(0, 0, 0, 0);
    if (a.bias && col_ok) acc0 = load4(static_cast<const W *>(a.bias) + col);
    const uint8_t *my_rows = slab + cl * 16;

    const int64_t p0 = (int64_t)blockIdx.y * a.passes_per_block;
    const int64_t p1 = p0 + a.passes_per_block < a.passes ? p0 + a.passes_per_block : a.passes;
    uint32_t c[T::SLOTS];
    fetch_codes<T>(a, p0 * kPass + tid, c);
    for (int64_t p = p0; p < p1; ++p) {
        __syncthreads();                                       // the slab is filled / the previous pass has been read
        {
            uint32_t w[T::STAGE / 4];
#pragma unroll
            for (int k = 0; k < T::STAGE / 4; ++k) w[k] = 0;
#pragma unroll
            for (int s = 0; s < T::SLOTS; ++s) w[s >> 2] |= T::stage(s, c[s]) << (8 * (s & 3));
            uint32_t *dst = staged + tid * (T::STAGE / 4);
            if (T::SIZE == 3) {
                *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
                dst[4] = w[4];
            } else {
                *reinterpret_cast<uint2 *>(dst) = make_uint2(w[0], w[1]);
            }
        }
        __syncthreads();
        if (p + 1 < p1) fetch_codes<T>(a, (p + 1) * kPass + tid, c);   // in flight while this pass is summed

        const int64_t g0 = p * kPass;
        uint32_t w[T::WORDS], wn[T::WORDS] = {};
        read_staged<T>(staged, first, w);
#pragma unroll 1                                               // unrolled, the 2x2x2 body keeps 16 groups live and spills
        for (int it = 0; it < kPass / kGroup; ++it) {
            const int st = it * kGroup + first;
            if (g0 + (st & ~3) >= a.n) break;                  // wave-uniform: the wave's four states are st & ~3 .. + 3
            if (it + 1 < kPass / kGroup) read_staged<T>(staged, st + kGroup, wn);   // the next group's rows, one LDS latency ahead
            float acc[kV] = {__uint_as_float(acc0.x), __uint_as_float(acc0.y), __uint_as_float(acc0.z), __uint_as_float(acc0.w)};
#pragma unroll
            for (int s = 0; s < T::SLOTS; ++s) {               // slot order is part of the contract: one fp32 addition per slot
                const uint32_t k = T::base(s) + ((w[s >> 2] >> (8 * (s & 3))) & 0xffu);
                const float4 f = *reinterpret_cast<const float4 *>(my_rows + k * kRowBytes);
                acc[0] = acc[0] + f.x; acc[1] = acc[1] + f.y; acc[2] = acc[2] + f.z; acc[3] = acc[3] + f.w;
            }
            if (a.act == RC_NET_ACT_ELU) {
                // acc > 0 ? acc : expm1f(acc) of the header, where expm1f(-0) is -0.  The device's expm1f answers +0 there, so zeros of
                // both signs take the identity branch (>=, not >); a NaN fails the comparison and stays a NaN through expm1f.
#pragma unroll
                for (int j = 0; j < kV; ++j) acc[j] = acc[j] >= 0.0f ? acc[j] : expm1f(acc[j]);
            }
            const int64_t g = g0 + st;
            if (g < a.n && col_ok) store4(static_cast<O *>(a.out) + g * a.out_stride + col, acc);
#pragma unroll
            for (int k = 0; k < T::WORDS; ++k) w[k] = wn[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------- host side
// -1: bad argument, -2: a HIP call failed (include/rubiknet.h)
inline int fail(const char *msg) { return fail(-1, "%s", msg); }

constexpr int kTargetBlocks = 256;               // one workgroup per CU of an MI355X at 3x3x3

template <class T, class W, class O>
int launch(Args a, void *stream) {
    const int slabs = (a.hidden + kCols - 1) / kCols;
    // workgroups per CU: 1 at 3x3x3 (152 KiB of the 160 KiB of LDS), 2 at 2x2x2 (32 waves) -- state ranges to fill the chip once
    constexpr int per_cu = T::SIZE == 3 ? 1 : 2;
    int64_t ranges = (kTargetBlocks * per_cu + slabs - 1) / slabs;
    if (ranges > a.passes) ranges = a.passes;
    if (ranges > 65535) ranges = 65535;
    a.passes_per_block = (a.passes + ranges - 1) / ranges;
    ranges = (a.passes + a.passes_per_block - 1) / a.passes_per_block;
    hipLaunchKernelGGL((k_first_layer<T, W, O>), dim3((unsigned)slabs, (unsigned)ranges), dim3(kThreads), 0, S(stream), a);
    RC_HIP(-2, hipGetLastError());
    return 0;
}

template <class T>
int by_format(const Args &a, int wfmt, int ofmt, void *stream) {
    if (wfmt == RC_FMT_F32) return ofmt == RC_FMT_F32 ? launch<T, float, float>(a, stream) : launch<T, float, bf16_t>(a, stream);
    return ofmt == RC_FMT_F32 ? launch<T, bf16_t, float>(a, stream) : launch<T, bf16_t, bf16_t>(a, stream);
}

}  // namespace

RC_BUILD_ID(rc_net_build_id)

const char *rc_net_last_error(void) { return t_err; }

int rc_net_first_layer(const uint8_t *code, int64_t n, int64_t code_pitch, int cube_size, const void *wt, const void *bias, int hidden,
                       int wfmt, int act, void *out, int ofmt, int64_t out_stride, void *stream) {
    if (cube_size != 2 && cube_size != 3) return fail("rc_net_first_layer: cube_size must be 2 or 3");
    if (!code || !wt || !out) return fail("rc_net_first_layer: null code, wt or out");
    if (n < 0) return fail("rc_net_first_layer: n < 0");
    if (hidden < 8 || hidden > 4096 || hidden % 8 != 0) return fail("rc_net_first_layer: hidden must be a multiple of 8 in 8..4096");
    if ((wfmt != RC_FMT_F32 && wfmt != RC_FMT_BF16) || (ofmt != RC_FMT_F32 && ofmt != RC_FMT_BF16))
        return fail("rc_net_first_layer: wfmt and ofmt must be RC_FMT_F32 (4) or RC_FMT_BF16 (5)");
    if (act != RC_NET_ACT_NONE && act != RC_NET_ACT_ELU) return fail("rc_net_first_layer: act must be 0 (none) or 1 (ELU)");
    if (out_stride < hidden) return fail("rc_net_first_layer: out_stride < hidden");
    const int64_t osz = ofmt == RC_FMT_F32 ? 4 : 2;
    if (!aligned16(code) || !aligned16(wt) || !aligned16(bias) || !aligned16(out) || (out_stride * osz) % 16 != 0)
        return fail("rc_net_first_layer: code, wt, bias, out and every row of out must be 16-byte aligned");
    const int slots = cube_size == 3 ? 20 : 7;
    const int shift = tile_shift(code_pitch, n, slots);
    if (shift == -1) return fail("rc_net_first_layer: code_pitch must be a positive multiple of 16 with SLOTS * code_pitch < 2^32");
    if (shift < 0) return fail("rc_net_first_layer: several tiles need a power-of-two code_pitch >= 512");
    if (n == 0) return 0;
    Args a{code, wt, bias, out, n, code_pitch, out_stride, (n + kPass - 1) / kPass, 0, shift, hidden, act};
    return cube_size == 3 ? by_format<Net3>(a, wfmt, ofmt, stream) : by_format<Net2>(a, wfmt, ofmt, stream);
}
