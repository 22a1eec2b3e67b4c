// What the kernels and entries that work on uint8 [L][H][W][3] frames share: the scene detector's luma, the group of four pixels as
// three dwords, the clip to a byte, and on the host the size checks, the overlap tests and the launch of L frames in slabs of the
// grid's y axis.  Internal linkage: no object exports anything from here.  include/e2fgvi_hip.h has the definitions.
#pragma once
#include "common.h"

namespace {

constexpr int FB_PX = 4;                  // pixels per group: 12 bytes, three dwords
constexpr int FB_FRAMES_MAX = 65535;      // frames per launch (the grid's y axis); more are launched in slabs
constexpr long long FB_N_MAX = 1LL << 26; // pixels per frame

// Y = (77 R + 150 G + 29 B + 128) >> 8
__device__ __forceinline__ int fb_luma(unsigned r, unsigned g, unsigned b) { return (int)((77u * r + 150u * g + 29u * b + 128u) >> 8); }

// three dwords of a group that is whole and on a dword
__device__ __forceinline__ void fb_load_dwords(const uint8_t* p, unsigned (&w)[3]) {
    const unsigned* q = reinterpret_cast<const unsigned*>(p);
    w[0] = q[0];
    w[1] = q[1];
    w[2] = q[2];
}

// the n <= 4 pixels at p as three words (the bytes behind the n-th pixel are 0): dwords when the group is whole and on a dword
__device__ __forceinline__ void fb_load(const uint8_t* p, int n, unsigned (&w)[3]) {
    if (n == FB_PX && ((uintptr_t)p & 3) == 0) {
        fb_load_dwords(p, w);
    } else {
        w[0] = w[1] = w[2] = 0;
#pragma unroll
        for (int i = 0; i < 3 * FB_PX; ++i)
            if (i < 3 * n) w[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
    }
}

// the same way out: only the bytes of the n pixels are written
__device__ __forceinline__ void fb_store(uint8_t* p, int n, const unsigned (&w)[3]) {
    if (n == FB_PX && ((uintptr_t)p & 3) == 0) {
        unsigned* q = reinterpret_cast<unsigned*>(p);
        q[0] = w[0];
        q[1] = w[1];
        q[2] = w[2];
    } else {
#pragma unroll
        for (int i = 0; i < 3 * FB_PX; ++i)
            if (i < 3 * n) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// byte i of a group: channel i % 3 of pixel i / 3
__device__ __forceinline__ int fb_get(const unsigned (&w)[3], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }

// the luma of the four pixels of a group: a pixel's three bytes are moved to the bottom (or left at the top) of a word and
// multiplied by the three weights in one v_dot4_u32_u8, the fourth weight being 0: 10 instructions where shifts and masks take 32
__device__ __forceinline__ void fb_luma4(const unsigned (&w)[3], int (&y)[FB_PX]) {
    constexpr unsigned K = 77u | (150u << 8) | (29u << 16);
    y[0] = (int)(__builtin_amdgcn_udot4(w[0], K, 128u, false) >> 8);
    y[1] = (int)(__builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w[1], w[0], 3), K, 128u, false) >> 8);
    y[2] = (int)(__builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w[2], w[1], 2), K, 128u, false) >> 8);
    y[3] = (int)(__builtin_amdgcn_udot4(w[2], K << 8, 128u, false) >> 8);
}

// The same four lumas with shifts and masks, the 32 instructions.  flicker.hip keeps this coding: when the two were timed side by side
// (profiles/frame_bytes_isa.txt) its apply pass on the flat video came out above the slowest repetition of this one with fb_luma4
__device__ __forceinline__ void fb_luma4_shifts(const unsigned (&w)[3], int (&y)[FB_PX]) {
    y[0] = fb_luma(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u);
    y[1] = fb_luma(w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
    y[2] = fb_luma((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u);
    y[3] = fb_luma((w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
}

// A value clipped to [0, 255] on its way into a word of packed bytes.  Two clipped shifts side by side in a word are what hipcc
// turns into one v_ashr_pk_u8_i32 (new on gfx950: shift two int32, clamp each to a byte, pack them into the low half of the
// destination), and it ORs the word's other two bytes on top of the result as if the upper half were zero.  On the chip exactly
// those two bytes came out wrong (bits set that neither operand has) while the packed pair was right, in the 8-byte instantiation
// of yuv.hip's decoder, the only code of the library that had the instruction; its byte-wise instantiation and a host build of the
// same body were right.  The empty asm ends the pattern: the clip stays a v_med3_i32 and the bytes are packed with shifts and ORs.
// build.verify_no_pk_u8 fails the build if the instruction comes back in any unit.
__device__ __forceinline__ unsigned fb_byte(int v) {
    v = min(max(v, 0), 255);
    asm volatile("" : "+v"(v));
    return (unsigned)v;
}

// ------------------------------------------------------------------------------------------------ the host side
// what every entry asks of its frames first; a unit's own checks come behind it
inline int fb_check_sizes(const char* who, int32_t L, int32_t H, int32_t W) {
    E2_REQUIRE(L >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "%s: negative size (L = %d, H = %d, W = %d)", who, L, H, W);
    E2_REQUIRE((int64_t)H * W <= FB_N_MAX, E2FGVI_EINVAL, "%s: needs H * W <= 2^26, got %d x %d", who, H, W);
    return 0;
}

// pn bytes at p and qn bytes at q share no byte
inline bool fb_disjoint(const void* p, uint64_t pn, const void* q, uint64_t qn) {
    const uint64_t a = (uint64_t)(uintptr_t)p, b = (uint64_t)(uintptr_t)q;
    return a + pn <= b || b + qn <= a;
}

// two buffers of n bytes each are one buffer or share no byte: what a kernel that writes each byte where it read it may be given
inline bool fb_same_or_disjoint(const void* p, const void* q, uint64_t n) { return p == q || fb_disjoint(p, n, q, n); }

// launch(t0, n) for every slab of L frames, n <= FB_FRAMES_MAX frames from frame t0 on, with the launch check behind each:
//   return fb_slabs("who", L, [&](int t0, unsigned n) { hipLaunchKernelGGL(kernel, dim3(nblk, n), ..., t0, ...); });
template <class Launch>
inline int fb_slabs(const char* who, int L, Launch&& launch) {
    for (int t0 = 0; t0 < L; t0 += FB_FRAMES_MAX) {
        launch(t0, (unsigned)(L - t0 < FB_FRAMES_MAX ? L - t0 : FB_FRAMES_MAX));
        E2_LAUNCH_CHECK(who);
    }
    return 0;
}

}  // namespace
