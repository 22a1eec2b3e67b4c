// Colour restoration (video.restore_color, video.apply_color): per scene and channel one monotone byte table, from channel
// histograms pooled over a set of frames and their quantile nodes.  Pure integers; include/e2fgvi_hip.h has the definition,
// tests/color_cases.py restates it in numpy, word for word and byte for byte.
//   frames uint8 [L][H][W][3], read as N = H W pixels per frame; byte i of a group of four pixels (twelve bytes) is channel i mod 3
//
// The histogram pass.  hist[t][c][v] = the pixels of frame t whose channel c equals v, int32 [L][3][256].  A workgroup owns
// COL_HPX = 8192 consecutive pixels of one frame; a thread takes COL_HIT = 8 groups of four pixels, 1024 pixels apart, read as the
// deflicker reads them: three dwords each when the frame starts on a dword, bytes otherwise and for the short last group; all the
// dwords of a thread are asked for before the first is used.  Every frame byte is read once.  Counts go to LDS with integer
// atomics, three histograms of COL_HC = 8 copies of the 256 bins side by side (word 8 (256 c + v) + tid % 8); the equal bytes of one
// channel in a group are one atomic of their number -- on a flat frame every lane of every wave hits one bin per channel, one
// atomic of 4 where there would be four.  After the barrier thread v adds the copies of its three bins and adds every sum that is
// not zero to hist with one integer global atomic.  The entry clears all L 768 words on the stream first.
//
// The nodes pass.  One workgroup per (group, channel), thread v: its bin summed in 64 bits over the group's ids (an id outside
// [0, L) is skipped, starts are read clamped to [0, M]), a 256-wide inclusive scan in 64 bits (wave shuffles, the four wave totals
// through LDS) into LDS, then thread k < 34 finds the smallest level with C > r_k by bisection: 32 quantiles, the black and the
// white point.  A pool reaches 2^50 pixels, so the products and the one division per node are 64-bit.
//
// The table pass.  One workgroup per group, thread v; the black and white points of the three channels are read first (the
// automatic target of the levels mode is their smallest and largest over the usable channels), then the level's three entries.
//
// The apply pass.  A workgroup stages its frame's group's 768 table bytes in LDS -- the identity for a frame whose group is outside
// [0, G), which copies it -- and owns COL_APX = 4096 consecutive pixels; a thread takes four groups of four pixels.  Twelve LDS
// lookups per group where the deflicker makes four: the table is 256 dwords with R, G and B packed (one ds_read_b32, the byte
// picked by a shift) or, with -DCOL_PACKED=0, three byte tables (ds_read_u8); profiles/color.txt has what both measured.  Bytes
// are put together into dwords in registers; each output byte is written once, by the thread that read the input byte, so
// out == frames is in order.
#include "frame_bytes.h"

namespace {

constexpr int COL_NTH = 256;
constexpr int COL_K = 32;                 // quantile nodes per group and channel, as the deflicker's
constexpr int COL_HIT = 8;                // groups per thread of the histogram kernel
constexpr int COL_HPX = COL_NTH * FB_PX * COL_HIT;
// A/B switches (build.build_variant("tag", "-DCOL_COPIES=1")); profiles/color.txt has what they measured
#ifndef COL_COPIES
#define COL_COPIES 8
#endif
#ifndef COL_MERGE
#define COL_MERGE 1
#endif
#ifndef COL_PACKED
#define COL_PACKED 1
#endif
constexpr int COL_HC = COL_COPIES;        // copies of each histogram in LDS: a power of two
constexpr int COL_AIT = 4;                // groups per thread of the apply kernel
constexpr int COL_APX = COL_NTH * FB_PX * COL_AIT;
constexpr int COL_Q = COL_K + 2;          // nodes per group and channel: 32 quantiles, the black and the white point
constexpr int COL_CLIP_MAX = 250;         // per mille
constexpr int COL_GAIN_MIN = 256, COL_GAIN_MAX = 4096;

__global__ void __launch_bounds__(COL_NTH)
color_hist_kernel(const uint8_t* __restrict__ frames, int t0, int N, int* __restrict__ hist) {
    __shared__ int s_h[3 * 256 * COL_HC];
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < 3 * 256 * COL_HC; i += COL_NTH) s_h[i] = 0;
    __syncthreads();
    const uint8_t* fr = frames + (long long)t * N * 3;
    const int p0 = (int)blockIdx.x * COL_HPX + tid * FB_PX;       // < 2^26 + 8192: blockIdx.x < ceil(N / COL_HPX)
    int* mine = s_h + (tid & (COL_HC - 1));
    // the same for every thread of the frame: a group is 12 bytes
    if (((uintptr_t)fr & 3) == 0) {
        unsigned w[COL_HIT][3];
#pragma unroll
        for (int k = 0; k < COL_HIT; ++k) {
            const int p = p0 + k * COL_NTH * FB_PX;
            w[k][0] = w[k][1] = w[k][2] = 0;
            if (p + FB_PX <= N) fb_load_dwords(fr + (long long)p * 3, w[k]);       // the twelve bytes lie in frame t
        }
#pragma unroll
        for (int k = 0; k < COL_HIT; ++k) {
            const int p = p0 + k * COL_NTH * FB_PX;
            if (p + FB_PX <= N) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    int v[FB_PX];
#pragma unroll
                    for (int j = 0; j < FB_PX; ++j) v[j] = fb_get(w[k], 3 * j + c);
#pragma unroll
                    for (int j = 0; j < FB_PX; ++j) {
                        if (COL_MERGE) {
                            // the first of the equal bytes counts for all of them
                            bool seen = false;
                            int n = 1;
#pragma unroll
                            for (int i = 0; i < FB_PX; ++i) {
                                if (i < j) seen = seen || v[i] == v[j];
                                if (i > j) n += v[i] == v[j] ? 1 : 0;
                            }
                            if (!seen) atomicAdd(mine + (c * 256 + v[j]) * COL_HC, n);
                        } else {
                            atomicAdd(mine + (c * 256 + v[j]) * COL_HC, 1);
                        }
                    }
                }
            } else {
                for (int j = 0; p + j < N; ++j) {                  // the short group at the end of the frame
                    const uint8_t* q = fr + (long long)(p + j) * 3;
                    for (int c = 0; c < 3; ++c) atomicAdd(mine + (c * 256 + q[c]) * COL_HC, 1);
                }
            }
        }
    } else {
        for (int k = 0; k < COL_HIT; ++k) {
            const int p = p0 + k * COL_NTH * FB_PX;
            for (int j = 0; j < FB_PX && p + j < N; ++j) {
                const uint8_t* q = fr + (long long)(p + j) * 3;
                for (int c = 0; c < 3; ++c) atomicAdd(mine + (c * 256 + q[c]) * COL_HC, 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < COL_HC; ++k) sum += s_h[(c * 256 + tid) * COL_HC + ((k + tid) & (COL_HC - 1))];
        if (sum) atomicAdd(hist + ((long long)t * 3 + c) * 256 + tid, sum);
    }
}

// fl_scan256 in 64 bits
__device__ __forceinline__ long long col_scan256(long long v, long long* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const long long o = __shfl_up(v, s, 64);
        if (lane >= s) v += o;
    }
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    long long base = 0;
#pragma unroll
    for (int w = 0; w < COL_NTH / 64 - 1; ++w)
        if (w < wave) base += s_w[w];
    return v + base;
}

// fl_node in 64 bits: the smallest v with C[v] > r, 0 <= r < C[255]
__device__ __forceinline__ int col_node(const long long* s_c, long long r) {
    int lo = 0, hi = 255;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_c[mid] > r) hi = mid;
        else lo = mid + 1;
    }
    const long long below = lo ? s_c[lo - 1] : 0;
    const long long h = s_c[lo] - below;
    long long frac = (16 * (r - below)) / (h > 0 ? h : 1);
    frac = frac < 0 ? 0 : (frac > 15 ? 15 : frac);                 // in 0 .. 15 already: below <= r < below + h
    return 16 * lo + (int)frac;
}

__global__ void __launch_bounds__(COL_NTH)
color_nodes_kernel(const int* __restrict__ hist, const int* __restrict__ starts, const int* __restrict__ ids, int L, int M, int lo,
                   int hi, int* __restrict__ Q) {
    __shared__ long long s_c[256];
    __shared__ long long s_w[COL_NTH / 64];
    const int g = (int)(blockIdx.x / 3), c = (int)(blockIdx.x % 3);
    const int v = (int)threadIdx.x;
    const int i0 = min(max(starts[g], 0), M), i1 = min(max(starts[g + 1], 0), M);
    long long p = 0;
    for (int i = i0; i < i1; ++i) {                                // the same trips for the whole workgroup
        const int t = ids[i];
        if (t >= 0 && t < L) p += hist[((long long)t * 3 + c) * 256 + v];
    }
    s_c[v] = col_scan256(p, s_w);
    __syncthreads();
    if (v < COL_Q) {
        const long long n = s_c[255];
        int q = 0;
        if (n > 0) {
            const long long r = v < COL_K ? ((long long)(2 * v + 1) * n) / (2 * COL_K)
                              : v == COL_K ? ((long long)lo * n) / 1000 : n - 1 - ((long long)hi * n) / 1000;
            q = col_node(s_c, r);
        }
        Q[((long long)g * 3 + c) * COL_Q + v] = q;
    }
}

// the floor of a / b, b > 0, for either sign of a
__device__ __forceinline__ long long col_floor_div(long long a, long long b) {
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

__global__ void __launch_bounds__(COL_NTH)
color_lut_kernel(const int* __restrict__ Q, const int* __restrict__ T, const int* __restrict__ mode, int lo_t, int hi_t, int min_range,
                 int max_gain, int strength, uint8_t* __restrict__ lut) {
    const int g = (int)blockIdx.x, v = (int)threadIdx.x;
    const int* Qg = Q + (long long)g * 3 * COL_Q;
    const int* Tg = T + (long long)g * 3 * COL_Q;
    const int md = mode[g];
    // the end points of the three channels first: the automatic target is taken over the usable ones
    long long b[3], w[3], B = 0, Wt = 0;
    bool usable[3], any = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        b[c] = Qg[c * COL_Q + COL_K];
        w[c] = Qg[c * COL_Q + COL_K + 1];
        usable[c] = w[c] - b[c] >= 16LL * min_range;
        if (usable[c]) {
            B = any ? (b[c] < B ? b[c] : B) : b[c];
            Wt = any ? (w[c] > Wt ? w[c] : Wt) : w[c];
            any = true;
        }
    }
    if (lo_t >= 0) {
        B = 16 * lo_t;
        Wt = 16 * hi_t;
    }
    const long long x = 16 * v;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        long long o = x;
        if (md == 1) {
            if (usable[c]) {
                const long long den = w[c] - b[c];
                const long long cut = ((long long)max_gain * den) >> 8;
                const long long num = Wt - B < cut ? Wt - B : cut;
                o = col_floor_div((B + Wt) * den + (2 * x - b[c] - w[c]) * num + den, 2 * den);
            }
        } else if (md == 2) {
            const int* q = Qg + c * COL_Q;
            const int* tt = Tg + c * COL_Q;
            const long long q0 = q[0], q31 = q[COL_K - 1];
            if (x <= q0) {
                o = x + min(max(tt[0], 0), 4095) - q0;
            } else if (x >= q31) {
                o = x + min(max(tt[COL_K - 1], 0), 4095) - q31;
            } else {
                int k = COL_K - 2;                                  // the largest index with q[k] <= x: q[0] < x, so there is one
                while (k > 0 && (long long)q[k] > x) --k;
                int k1 = k + 1;                                    // and q[k + 1] > x by the choice of k
                const long long den = (long long)q[k1] - q[k];
                const long long tk = min(max(tt[k], 0), 4095), tk1 = min(max(tt[k1], 0), 4095);
                o = tk + col_floor_div(2 * (x - q[k]) * (tk1 - tk) + den, 2 * den);
            }
        }
        const long long o2 = x + (((o - x) * strength + 128) >> 8);
        const long long e = (o2 + 8) >> 4;
        lut[((long long)g * 3 + c) * 256 + v] = (uint8_t)(e < 0 ? 0 : (e > 255 ? 255 : e));
    }
}

// the table entry of byte value v of channel c
#if COL_PACKED
__device__ __forceinline__ unsigned col_look(const unsigned* s_t, int c, int v) { return (s_t[v] >> (8 * c)) & 255u; }
#else
__device__ __forceinline__ unsigned col_look(const uint8_t* s_t, int c, int v) { return s_t[c * 256 + v]; }
#endif

__global__ void __launch_bounds__(COL_NTH)
color_apply_kernel(const uint8_t* frames, const uint8_t* __restrict__ lut, const int* __restrict__ group, int t0, int N, int G,
                   uint8_t* out) {
#if COL_PACKED
    __shared__ unsigned s_t[256];
#else
    __shared__ uint8_t s_t[3 * 256];
#endif
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    const int g = group[t];
    {
        // a frame whose group is outside [0, G) gets the identity: it is copied
        unsigned e[3] = {(unsigned)tid, (unsigned)tid, (unsigned)tid};
        if (g >= 0 && g < G) {
#pragma unroll
            for (int c = 0; c < 3; ++c) e[c] = lut[((long long)g * 3 + c) * 256 + tid];
        }
#if COL_PACKED
        s_t[tid] = e[0] | (e[1] << 8) | (e[2] << 16);
#else
#pragma unroll
        for (int c = 0; c < 3; ++c) s_t[c * 256 + tid] = (uint8_t)e[c];
#endif
    }
    __syncthreads();
    const uint8_t* fr = frames + (long long)t * N * 3;
    uint8_t* fo = out + (long long)t * N * 3;
    const int p0 = (int)blockIdx.x * COL_APX + tid * FB_PX;
    const bool aligned = (((uintptr_t)fr | (uintptr_t)fo) & 3) == 0;       // the same for every thread of the frame
    unsigned w[COL_AIT][3];
    // frames and out may be the same buffer (no __restrict__): a thread reads the bytes of its groups before it writes any of them
    if (aligned) {
#pragma unroll
        for (int k = 0; k < COL_AIT; ++k) {
            const int p = p0 + k * COL_NTH * FB_PX;
            w[k][0] = w[k][1] = w[k][2] = 0;
            if (p + FB_PX <= N) fb_load_dwords(fr + (long long)p * 3, w[k]);       // the twelve bytes lie in frame t
        }
    }
#pragma unroll
    for (int k = 0; k < COL_AIT; ++k) {
        const int p = p0 + k * COL_NTH * FB_PX;
        if (aligned && p + FB_PX <= N) {
            unsigned b[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) b[i] = col_look(s_t, i % 3, fb_get(w[k], i));
            unsigned* o = reinterpret_cast<unsigned*>(fo + (long long)p * 3);
#pragma unroll
            for (int i = 0; i < 3; ++i) o[i] = b[4 * i] | (b[4 * i + 1] << 8) | (b[4 * i + 2] << 16) | (b[4 * i + 3] << 24);
        } else {
            for (int j = 0; j < FB_PX && p + j < N; ++j) {
                const uint8_t* q = fr + (long long)(p + j) * 3;
                const int r = q[0], gr = q[1], bl = q[2];
                uint8_t* o = fo + (long long)(p + j) * 3;
                o[0] = (uint8_t)col_look(s_t, 0, r);
                o[1] = (uint8_t)col_look(s_t, 1, gr);
                o[2] = (uint8_t)col_look(s_t, 2, bl);
            }
        }
    }
}

}  // namespace

extern "C" int e2fgvi_color_hist(const uint8_t* frames, int32_t* hist, int32_t L, int32_t H, int32_t W, void* stream) {
    if (int rc = fb_check_sizes("color_hist", L, H, W)) return rc;
    const int N = H * W;
    if (L == 0 || N == 0) return 0;                                // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && hist, E2FGVI_EINVAL, "color_hist: null pointer");
    E2_REQUIRE(((uintptr_t)hist & 3) == 0, E2FGVI_EINVAL, "color_hist: hist must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(hist, 0, sizeof(int32_t) * 3 * 256 * (size_t)L, st);
    E2_REQUIRE(e == hipSuccess, (int)e, "color_hist: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const unsigned nblk = (unsigned)((N + COL_HPX - 1) / COL_HPX);
    return fb_slabs("color_hist", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(color_hist_kernel, dim3(nblk, n), dim3(COL_NTH), 0, st, frames, t0, N, hist);
    });
}

extern "C" int e2fgvi_color_nodes(const int32_t* hist, const int32_t* starts, const int32_t* ids, int32_t* Q, int32_t L, int32_t G,
                                  int32_t M, int32_t lo, int32_t hi, void* stream) {
    E2_REQUIRE(L >= 0 && G >= 0 && M >= 0, E2FGVI_EINVAL, "color_nodes: negative size (L = %d, G = %d, M = %d)", L, G, M);
    E2_REQUIRE((int64_t)G * 3 <= 0x7fffffffLL, E2FGVI_EINVAL, "color_nodes: needs 3 G < 2^31, got G = %d", G);
    E2_REQUIRE(lo >= 0 && lo <= COL_CLIP_MAX, E2FGVI_EINVAL, "color_nodes: lo must be in [0, %d], got %d", COL_CLIP_MAX, lo);
    E2_REQUIRE(hi >= 0 && hi <= COL_CLIP_MAX, E2FGVI_EINVAL, "color_nodes: hi must be in [0, %d], got %d", COL_CLIP_MAX, hi);
    if (G == 0) return 0;                                          // no group: no launch, and the pointers are not looked at
    // without a frame or an id every pool is empty: the launch writes zeros and reads neither hist nor ids
    E2_REQUIRE(starts && Q && (hist || L == 0 || M == 0) && (ids || M == 0), E2FGVI_EINVAL, "color_nodes: null pointer");
    E2_REQUIRE((((uintptr_t)hist | (uintptr_t)starts | (uintptr_t)ids | (uintptr_t)Q) & 3) == 0, E2FGVI_EINVAL,
               "color_nodes: hist, starts, ids and Q must be 4-byte aligned");
    hipLaunchKernelGGL(color_nodes_kernel, dim3((unsigned)G * 3u), dim3(COL_NTH), 0, (hipStream_t)stream, hist, starts, ids, L, M, lo, hi,
                       Q);
    E2_LAUNCH_CHECK("color_nodes");
    return 0;
}

extern "C" int e2fgvi_color_lut(const int32_t* Q, const int32_t* T, const int32_t* mode, uint8_t* lut, int32_t G, int32_t lo_t,
                                int32_t hi_t, int32_t min_range, int32_t max_gain, int32_t strength, void* stream) {
    E2_REQUIRE(G >= 0, E2FGVI_EINVAL, "color_lut: negative size (G = %d)", G);
    E2_REQUIRE((lo_t == -1 && hi_t == -1) || (lo_t >= 0 && lo_t < hi_t && hi_t <= 255), E2FGVI_EINVAL,
               "color_lut: the target must be lo_t = hi_t = -1 or 0 <= lo_t < hi_t <= 255, got %d, %d", lo_t, hi_t);
    E2_REQUIRE(min_range >= 1 && min_range <= 255, E2FGVI_EINVAL, "color_lut: min_range must be in [1, 255], got %d", min_range);
    E2_REQUIRE(max_gain >= COL_GAIN_MIN && max_gain <= COL_GAIN_MAX, E2FGVI_EINVAL, "color_lut: max_gain must be in [%d, %d], got %d",
               COL_GAIN_MIN, COL_GAIN_MAX, max_gain);
    E2_REQUIRE(strength >= 0 && strength <= 256, E2FGVI_EINVAL, "color_lut: strength must be in [0, 256], got %d", strength);
    if (G == 0) return 0;                                          // no group: no launch, and the pointers are not looked at
    E2_REQUIRE(Q && T && mode && lut, E2FGVI_EINVAL, "color_lut: null pointer");
    E2_REQUIRE((((uintptr_t)Q | (uintptr_t)T | (uintptr_t)mode) & 3) == 0, E2FGVI_EINVAL,
               "color_lut: Q, T and mode must be 4-byte aligned");
    hipLaunchKernelGGL(color_lut_kernel, dim3((unsigned)G), dim3(COL_NTH), 0, (hipStream_t)stream, Q, T, mode, lo_t, hi_t, min_range,
                       max_gain, strength, lut);
    E2_LAUNCH_CHECK("color_lut");
    return 0;
}

extern "C" int e2fgvi_color_apply(const uint8_t* frames, const uint8_t* lut, const int32_t* group, uint8_t* out, int32_t L, int32_t H,
                                  int32_t W, int32_t G, void* stream) {
    if (int rc = fb_check_sizes("color_apply", L, H, W)) return rc;
    E2_REQUIRE(G >= 0, E2FGVI_EINVAL, "color_apply: negative size (G = %d)", G);
    const int N = H * W;
    if (L == 0 || N == 0) return 0;                                // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && group && out && (lut || G == 0), E2FGVI_EINVAL, "color_apply: null pointer");
    E2_REQUIRE(((uintptr_t)group & 3) == 0, E2FGVI_EINVAL, "color_apply: group must be 4-byte aligned");
    E2_REQUIRE(fb_same_or_disjoint(frames, out, (uint64_t)L * (uint64_t)N * 3), E2FGVI_EINVAL,
               "color_apply: out must be frames itself or not overlap it");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = (unsigned)((N + COL_APX - 1) / COL_APX);
    return fb_slabs("color_apply", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(color_apply_kernel, dim3(nblk, n), dim3(COL_NTH), 0, st, frames, lut, group, t0, N, G, out);
    });
}
