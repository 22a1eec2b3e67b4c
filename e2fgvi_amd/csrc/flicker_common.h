// What the deflicker (flicker.hip) and the local deflicker (flicker_local.hip) share beyond frame_bytes.h: the curves of one
// histogram row -- scan, nodes by bisection, the window's mean, the shift per level.  Device code only, internal linkage: neither
// object exports anything from here.  include/e2fgvi_hip.h has the definition.
#pragma once
#include "frame_bytes.h"

namespace {

constexpr int FL_NTH = 256;
constexpr int FL_K = 32;                  // quantile nodes per frame
constexpr int FL_SPAN_MAX = 8, FL_SHIFT_MAX = 64;

// the inclusive scan of one value per thread over the workgroup's 256 threads; s_w holds the four wave totals.  Two barriers; the
// caller puts one more between two calls (s_w is read here after the first and written again in the next call).
__device__ __forceinline__ int fl_scan256(int v, int* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(v, s, 64);
        if (lane >= s) v += o;
    }
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < FL_NTH / 64 - 1; ++w)
        if (w < wave) base += s_w[w];
    return v + base;
}

// Q of one frame's node k from its scan in LDS (s_c[v] = C[v]) : the smallest v with C[v] > r by bisection; a row that does not sum
// to N (the contract) still ends at some v <= 255, and an empty bin there divides by 1
__device__ __forceinline__ int fl_node(const int* s_c, int k, int N) {
    const long long r = ((long long)(2 * k + 1) * N) / (2 * FL_K);
    int lo = 0, hi = 255;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)s_c[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    const int below = lo ? s_c[lo - 1] : 0;
    const int h = s_c[lo] - below;
    long long frac = (16 * (r - below)) / (h > 0 ? h : 1);
    frac = frac < 0 ? 0 : (frac > 15 ? 15 : frac);                 // in 0 .. 15 already when the row sums to N
    return 16 * lo + (int)frac;
}

// The curves of one histogram row, by a workgroup of 256 threads, thread y: the row of frame u is hist + (u stride + row) 256, its
// pixels are N; Q and d are the outputs of row (t stride + row).  The nodes of the other frames of the window are not read from Q
// (that would need a launch of its own in front): the workgroup recomputes them from hist, frame by frame over its window of at most
// 2 FL_SPAN_MAX + 1 = 17 frames -- a 256-wide inclusive scan of the row (wave shuffles, the four wave totals through LDS) into LDS,
// then thread k < 32 finds the smallest level with C > r_k by bisection and adds its node to a register.  256 words and three
// barriers per frame of the window.  The frame's own scan, row and nodes stay in LDS for the 256 shifts.  64-bit where the
// definition says so (and in r_k: 63 N passes 2^31).  WHOLE: d is rounded to whole levels, (d16 + 8) >> 4; otherwise it stays d16.
template <bool WHOLE>
__device__ __forceinline__ void fl_curves_row(const int* __restrict__ hist, const int* __restrict__ scene, int t, int L, int stride,
                                              int row, int N, int span, int max_shift, int* __restrict__ Q, short* __restrict__ d) {
    __shared__ int s_c[2][256];            // [0]: the scan of the window's frame at hand, [1]: the scan of frame t
    __shared__ int s_w[FL_NTH / 64];
    __shared__ int s_s[FL_K];              // the node shifts of frame t
    const int y = (int)threadIdx.x;
    const int sc = scene[t];
    const int u0 = max(t - span, 0), u1 = min(t + span, L - 1);
    int qsum = 0, n = 0, qt = 0, ht = 0;
    for (int u = u0; u <= u1; ++u) {
        if (scene[u] != sc) continue;                              // the same for the whole workgroup
        const int h = hist[((long long)u * stride + row) * 256 + y];
        const int c = fl_scan256(h, s_w);
        const int which = u == t ? 1 : 0;
        s_c[which][y] = c;
        if (which) ht = h;
        __syncthreads();
        if (y < FL_K) {
            const int q = fl_node(s_c[which], y, N);
            qsum += q;
            if (which) qt = q;
        }
        ++n;
        __syncthreads();                                           // s_c[0] and s_w are written again in the next trip
    }
    const long long mine = (long long)t * stride + row;
    if (y < FL_K) {
        const int T = (2 * qsum + n) / (2 * n);                    // n >= 1: frame t is in its own window
        s_s[y] = min(max(T - qt, -16 * max_shift), 16 * max_shift);
        Q[mine * FL_K + y] = qt;
    }
    __syncthreads();
    const int below = y ? s_c[1][y - 1] : 0;
    const long long c2 = 2LL * below + ht;
    long long phi = (c2 * (FL_K * 128)) / N - 128;
    phi = phi < 0 ? 0 : (phi > (FL_K - 1) * 256 ? (FL_K - 1) * 256 : phi);
    const int k0 = (int)phi >> 8, f = (int)phi & 255, k1 = min(k0 + 1, FL_K - 1);
    const int d16 = (s_s[k0] * (256 - f) + s_s[k1] * f + 128) >> 8;
    d[mine * 256 + y] = (short)(WHOLE ? (d16 + 8) >> 4 : d16);
}

}  // namespace
