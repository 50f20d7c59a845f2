// rc_host.h -- host plumbing every translation unit of csrc/ shares: the build id, the thread-local error text, the HIP-call macro,
// pointer / size helpers, the one host statement of the tiled state layout and the Infinity Cache policy pick.
// rc_tree.cpp is built by the host compiler and takes the build id only; the rest needs hipcc.
#pragma once

#include <cstdint>
#include <cstdio>

// ---------------------------------------------------------------------------------------------------- build id
// The hash of the sources a library was compiled from (__graft_entry__.build passes -DRC_SRC_HASH=<16 hex digits>), stored in the
// binary as "rc-build-id:<id>" (_build.MARKER) and returned by the library's `fn`.  A plain compile without the define still works
// and reports "unhashed", which the Python binding refuses as stale.
#ifndef RC_SRC_HASH
#define RC_SRC_HASH unhashed
#endif
#define RC_STR2(x) #x
#define RC_STR(x) RC_STR2(x)
#define RC_BUILD_ID(fn)                                                       \
    static const char k_build_id[] = "rc-build-id:" RC_STR(RC_SRC_HASH);      \
    const char *fn(void) { return k_build_id + 12; }

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace rc {
struct Cube3;   // rc_tables.h: complete where by_size is called
struct Cube2;
}

namespace {

// ------------------------------------------------------------------------------------------ errors and HIP calls
// Every library returns a negative code and keeps the text of its thread's last refusal.  The codes and the wording stay each
// library's own: `code` and `fmt` (one or two %s) are the caller's.
thread_local char t_err[256] = "";

inline int fail(int code, const char *fmt, const char *a = "", const char *b = "") {
    snprintf(t_err, sizeof t_err, fmt, a, b);
    return code;
}
#define RC_HIP(code, call)                                                                      \
    do {                                                                                        \
        const hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) return fail(code, "%s: %s", #call, hipGetErrorString(e_));        \
    } while (0)

// The code of the helpers below that refuse by themselves (by_size, RC_GRID): bad argument, -1 in every library (RC_EINVAL).
constexpr int kEinval = -1;

// ------------------------------------------------------------------------------------------------- small helpers
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
template <class... P>
bool any_null(P... p) { return (... || (p == nullptr)); }
template <class... P>
bool all_aligned16(P... p) { return (... && aligned16(p)); }
inline int log2_exact(int64_t v) {
    int s = 0;
    while (((int64_t)1 << s) < v) ++s;
    return s;
}
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline hipStream_t S(void *s) { return static_cast<hipStream_t>(s); }

template <class F, class C3 = rc::Cube3, class C2 = rc::Cube2>
int by_size(int cube_size, F &&f) {
    if (cube_size == 3) return f(C3{});
    if (cube_size == 2) return f(C2{});
    return fail(kEinval, "cube_size must be 2 or 3");  // NotImplementedError, cube_env.py:44
}

// the x dimension of a grid is a positive int
inline bool grid_ok(int64_t blocks) { return blocks > 0 && blocks <= 0x7fffffff; }
#define RC_GRID(blocks) \
    do { if (!grid_ok(blocks)) return fail(kEinval, "too many cubes for one launch"); } while (0)

// -------------------------------------------------------------------------------------------------- state layout
// include/rubikhip.h "State layout", the one host statement of the rule.  A buffer of `rows` rows for n cubes is one tile
// (pitch >= n, pitch % 16 == 0) or several (pitch a power of two >= kMinTile = 512, the widest wave span); tiles follow each
// other, [tile][row][pitch].  Row offsets inside a tile are 32-bit scalar offsets of buffer instructions: rows * pitch < 2^32 (a
// single tile of more than 79 M 3x3x3 cubes has to be split into tiles).
// Returns the shift for tile_off / tiled (rc_device.h): log2(pitch) with several tiles, 63 with one; or -1: the pitch is not a
// positive multiple of 16 with rows * pitch < 2^32, -2: several tiles, and the pitch is no power of two >= 512.  Each caller has
// its own message for a refusal.  n = INT64_MAX asks for the tiled form whatever fits (the beams and pools of rc_search.hip).
constexpr int64_t kMinTile = 512;
inline int tile_shift(int64_t pitch, int64_t n, int rows = 54) {
    if (pitch <= 0 || (pitch & 15) != 0 || pitch * rows >= ((int64_t)1 << 32)) return -1;
    if (n <= pitch) return 63;
    if (pitch < kMinTile || (pitch & (pitch - 1)) != 0) return -2;
    return log2_exact(pitch);
}
inline int64_t tiles_of(int64_t n, int64_t pitch) { return n <= pitch ? 1 : ceil_div(n, pitch); }

// ---------------------------------------------------------------------------------------------------- cache policy
// Row-traffic policy (rc_device.h RowPolicy) of a launch that reads in_bytes and writes out_bytes, by what of it the Infinity
// Cache holds: 0 both fit: default-cached; 1 the output alone fits: stream the input, keep the output for the next launch;
// 2 beyond that: stream both.
constexpr int64_t kMallBytes = (int64_t)240 << 20;   // what we count on of the 256 MiB Infinity Cache
inline int mall_policy(int64_t in_bytes, int64_t out_bytes) {
    return in_bytes + out_bytes <= kMallBytes ? 0 : out_bytes <= kMallBytes ? 1 : 2;
}

}  // namespace
#endif  // __HIPCC__
