// Deflicker (video.deflicker): per frame a tone curve that moves its luma quantiles onto their mean over the frames around it.
// Pure integers; include/e2fgvi_hip.h has the definition, tests/flicker_cases.py restates it in numpy, word for word and byte for
// byte.
//   frames uint8 [L][H][W][3], read as N = H W pixels per frame;  Y = (77 R + 150 G + 29 B + 128) >> 8 (the scene detector's luma)
//
// The histogram pass.  hist[t][v] = the pixels of frame t with Y == v, int32 [L][256].  A workgroup owns FL_HPX = 8192 consecutive
// pixels of one frame; a thread takes FL_HIT = 8 groups of four pixels, 1024 pixels apart -- three dwords each when the frame starts
// on a dword (a group is 12 bytes, so every group of the frame is aligned when the first is), twelve bytes otherwise; the last
// group of a frame may be short and is read by bytes.  All the dwords of a thread are asked for before the first is used.  Every
// frame byte is read once.  Counts go to LDS with integer atomics, FL_HC = 8 copies of the 256 bins side by side (word 8 v + tid % 8:
// eight lanes that hit one bin hit eight banks); four equal lumas in a group -- the flat frame, where every lane of every wave
// hits one bin -- are one atomic of 4.  After the barrier thread v adds its bin's copies and, if the sum is not zero, adds it to
// hist[t][v] with one integer global atomic.  The entry clears all L 256 words on the stream first, so every word is written.
// Integer atomics: exact, the same in every run.  A bin holds up to N <= 2^26.
//
// The curves pass is ONE launch: workgroup t, thread v.  The nodes of the other frames of the window are not read from Q (that
// would need a launch of its own in front): the workgroup recomputes them from hist, frame by frame over its window of at most 2
// FL_SPAN_MAX + 1 = 17 frames -- a 256-wide inclusive scan of the row (wave shuffles, the four wave totals through LDS) into LDS,
// then thread k < 32 finds the smallest level with C > r_k by bisection and adds its node to a register.  256 words and three
// barriers per frame of the window; recomputing costs L (2 span + 1) KB of L2 reads in all.  The frame's own scan, row and nodes
// stay in LDS for the 256 shifts.  64-bit where the definition says so (and in r_k: 63 N passes 2^31).
//
// The apply pass.  A workgroup stages the frame's 256 shifts in LDS and owns FL_APX = 4096 consecutive pixels; a thread takes four
// groups of four pixels, loaded as in the histogram pass when both the frame and its output start on a dword.  The shift is looked
// up once per pixel and added to its three bytes, clipped to [0, 255]; twelve bytes go out as three dwords (or byte by byte): each
// output byte is written once, by the thread that read the input byte, so out == frames is in order.
#include "flicker_common.h"          // the scan, the nodes and the curves of one row: shared with flicker_local.hip

namespace {

constexpr int FL_HIT = 8;                 // groups per thread of the histogram kernel
constexpr int FL_HPX = FL_NTH * FB_PX * FL_HIT;
// A/B switches (build.build_variant("tag", "-DFL_COPIES=1")); profiles/flicker.txt has what they measured
#ifndef FL_COPIES
#define FL_COPIES 8
#endif
#ifndef FL_MERGE4
#define FL_MERGE4 1
#endif
constexpr int FL_HC = FL_COPIES;          // copies of the histogram in LDS: a power of two
constexpr int FL_AIT = 4;                 // groups per thread of the apply kernel
constexpr int FL_APX = FL_NTH * FB_PX * FL_AIT;

__global__ void __launch_bounds__(FL_NTH)
flicker_hist_kernel(const uint8_t* __restrict__ frames, int t0, int N, int* __restrict__ hist) {
    __shared__ int s_h[256 * FL_HC];
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < 256 * FL_HC; i += FL_NTH) s_h[i] = 0;
    __syncthreads();
    const uint8_t* fr = frames + (long long)t * N * 3;
    const int p0 = (int)blockIdx.x * FL_HPX + tid * FB_PX;        // < 2^26 + 8192: blockIdx.x < ceil(N / FL_HPX)
    int* mine = s_h + (tid & (FL_HC - 1));
    // the same for every thread of the frame: a group is 12 bytes
    if (((uintptr_t)fr & 3) == 0) {
        unsigned w[FL_HIT][3];
#pragma unroll
        for (int k = 0; k < FL_HIT; ++k) {
            const int p = p0 + k * FL_NTH * FB_PX;
            w[k][0] = w[k][1] = w[k][2] = 0;
            if (p + FB_PX <= N) fb_load_dwords(fr + (long long)p * 3, w[k]);       // the twelve bytes lie in frame t
        }
#pragma unroll
        for (int k = 0; k < FL_HIT; ++k) {
            const int p = p0 + k * FL_NTH * FB_PX;
            if (p + FB_PX <= N) {
                int y[FB_PX];
                fb_luma4_shifts(w[k], y);       // not fb_luma4: frame_bytes.h says why
                if (FL_MERGE4 && y[0] == y[1] && y[1] == y[2] && y[2] == y[3]) {
                    atomicAdd(mine + y[0] * FL_HC, FB_PX);
                } else {
#pragma unroll
                    for (int j = 0; j < FB_PX; ++j) atomicAdd(mine + y[j] * FL_HC, 1);
                }
            } else {
                for (int j = 0; p + j < N; ++j) {                  // the short group at the end of the frame
                    const uint8_t* q = fr + (long long)(p + j) * 3;
                    atomicAdd(mine + fb_luma(q[0], q[1], q[2]) * FL_HC, 1);
                }
            }
        }
    } else {
        for (int k = 0; k < FL_HIT; ++k) {
            const int p = p0 + k * FL_NTH * FB_PX;
            for (int j = 0; j < FB_PX && p + j < N; ++j) {
                const uint8_t* q = fr + (long long)(p + j) * 3;
                atomicAdd(mine + fb_luma(q[0], q[1], q[2]) * FL_HC, 1);
            }
        }
    }
    __syncthreads();
    int sum = 0;
#pragma unroll
    for (int c = 0; c < FL_HC; ++c) sum += s_h[tid * FL_HC + ((c + tid) & (FL_HC - 1))];
    if (sum) atomicAdd(hist + (long long)t * 256 + tid, sum);
}

__global__ void __launch_bounds__(FL_NTH)
flicker_curves_kernel(const int* __restrict__ hist, const int* __restrict__ scene, int L, int N, int span, int max_shift,
                      int* __restrict__ Q, short* __restrict__ d) {
    fl_curves_row<true>(hist, scene, (int)blockIdx.x, L, 1, 0, N, span, max_shift, Q, d);
}

__global__ void __launch_bounds__(FL_NTH)
flicker_apply_kernel(const uint8_t* frames, const short* __restrict__ d, int t0, int N, uint8_t* out) {
    __shared__ int s_d[256];
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    s_d[tid] = d[(long long)t * 256 + tid];
    __syncthreads();
    const uint8_t* fr = frames + (long long)t * N * 3;
    uint8_t* fo = out + (long long)t * N * 3;
    const int p0 = (int)blockIdx.x * FL_APX + tid * FB_PX;
    const bool aligned = (((uintptr_t)fr | (uintptr_t)fo) & 3) == 0;       // the same for every thread of the frame
    unsigned w[FL_AIT][3];
    // frames and out may be the same buffer (no __restrict__): a thread reads the bytes of its groups before it writes any of them
    if (aligned) {
#pragma unroll
        for (int k = 0; k < FL_AIT; ++k) {
            const int p = p0 + k * FL_NTH * FB_PX;
            w[k][0] = w[k][1] = w[k][2] = 0;
            if (p + FB_PX <= N) fb_load_dwords(fr + (long long)p * 3, w[k]);       // the twelve bytes lie in frame t
        }
    }
#pragma unroll
    for (int k = 0; k < FL_AIT; ++k) {
        const int p = p0 + k * FL_NTH * FB_PX;
        if (aligned && p + FB_PX <= N) {
            int y[FB_PX];
            fb_luma4_shifts(w[k], y);       // not fb_luma4: frame_bytes.h says why
            unsigned b[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) b[i] = fb_byte(fb_get(w[k], i) + s_d[y[i / 3]]);
            unsigned* o = reinterpret_cast<unsigned*>(fo + (long long)p * 3);
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
        } else {
            for (int j = 0; j < FB_PX && p + j < N; ++j) {
                const uint8_t* q = fr + (long long)(p + j) * 3;
                const int r = q[0], g = q[1], bl = q[2];
                const int s = s_d[fb_luma(r, g, bl)];
                uint8_t* o = fo + (long long)(p + j) * 3;
                o[0] = (uint8_t)min(max(r + s, 0), 255);
                o[1] = (uint8_t)min(max(g + s, 0), 255);
                o[2] = (uint8_t)min(max(bl + s, 0), 255);
            }
        }
    }
}

}  // namespace

extern "C" int e2fgvi_flicker_hist(const uint8_t* frames, int32_t* hist, int32_t L, int32_t H, int32_t W, void* stream) {
    if (int rc = fb_check_sizes("flicker_hist", L, H, W)) return rc;
    const int N = H * W;
    if (L == 0 || N == 0) return 0;                                // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && hist, E2FGVI_EINVAL, "flicker_hist: null pointer");
    E2_REQUIRE(((uintptr_t)hist & 3) == 0, E2FGVI_EINVAL, "flicker_hist: hist must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(hist, 0, sizeof(int32_t) * 256 * (size_t)L, st);
    E2_REQUIRE(e == hipSuccess, (int)e, "flicker_hist: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const unsigned nblk = (unsigned)((N + FL_HPX - 1) / FL_HPX);
    return fb_slabs("flicker_hist", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(flicker_hist_kernel, dim3(nblk, n), dim3(FL_NTH), 0, st, frames, t0, N, hist);
    });
}

extern "C" int e2fgvi_flicker_curves(const int32_t* hist, const int32_t* scene, int32_t* Q, int16_t* d, int32_t L, int32_t N,
                                     int32_t span, int32_t max_shift, void* stream) {
    E2_REQUIRE(L >= 0 && N >= 0, E2FGVI_EINVAL, "flicker_curves: negative size (L = %d, N = %d)", L, N);
    E2_REQUIRE(N <= FB_N_MAX, E2FGVI_EINVAL, "flicker_curves: needs N <= 2^26, got %d", N);
    E2_REQUIRE(span >= 0 && span <= FL_SPAN_MAX, E2FGVI_EINVAL, "flicker_curves: span must be in [0, %d], got %d", FL_SPAN_MAX, span);
    E2_REQUIRE(max_shift >= 1 && max_shift <= FL_SHIFT_MAX, E2FGVI_EINVAL, "flicker_curves: max_shift must be in [1, %d], got %d",
               FL_SHIFT_MAX, max_shift);
    if (L == 0 || N == 0) return 0;                                // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(hist && scene && Q && d, E2FGVI_EINVAL, "flicker_curves: null pointer");
    E2_REQUIRE((((uintptr_t)hist | (uintptr_t)scene | (uintptr_t)Q) & 3) == 0 && ((uintptr_t)d & 1) == 0, E2FGVI_EINVAL,
               "flicker_curves: hist, scene and Q must be 4-byte aligned, d 2-byte aligned");
    hipLaunchKernelGGL(flicker_curves_kernel, dim3((unsigned)L), dim3(FL_NTH), 0, (hipStream_t)stream, hist, scene, L, N, span,
                       max_shift, Q, d);
    E2_LAUNCH_CHECK("flicker_curves");
    return 0;
}

extern "C" int e2fgvi_flicker_apply(const uint8_t* frames, const int16_t* d, uint8_t* out, int32_t L, int32_t H, int32_t W,
                                    void* stream) {
    if (int rc = fb_check_sizes("flicker_apply", L, H, W)) return rc;
    const int N = H * W;
    if (L == 0 || N == 0) return 0;                                // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && d && out, E2FGVI_EINVAL, "flicker_apply: null pointer");
    E2_REQUIRE(((uintptr_t)d & 1) == 0, E2FGVI_EINVAL, "flicker_apply: d must be 2-byte aligned");
    E2_REQUIRE(fb_same_or_disjoint(frames, out, (uint64_t)L * (uint64_t)N * 3), E2FGVI_EINVAL,
               "flicker_apply: out must be frames itself or not overlap it");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = (unsigned)((N + FL_APX - 1) / FL_APX);
    return fb_slabs("flicker_apply", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(flicker_apply_kernel, dim3(nblk, n), dim3(FL_NTH), 0, st, frames, d, t0, N, out);
    });
}
