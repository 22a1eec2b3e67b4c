// PSNR / SSIM of evaluate.py (core/metrics.py:20-56) on the device, fp64 like the reference (img.astype(np.float64)):
//   psnr = 20 log10(255 / sqrt(mean((a-b)^2)))                                   (inf when identical)
//   ssim = skimage compare_ssim(a, b, data_range=255, multichannel=True, win_size=65): per channel, uniform 65x65 window,
//          sample covariance (NP/(NP-1)), K1 = 0.01, K2 = 0.03, S averaged over the image cropped by 32 pixels per side
//          (there every window lies inside the image, so the filter's border mode never matters), then over channels.
// Box sums come from fp64 summed-area tables: frames are uint8-valued (or k/2^j after the 0.5/0.5 blends), so every
// partial sum is exact in fp64 -- the only rounding is in the final SSIM arithmetic.  Reductions are two-stage with a
// fixed order (deterministic).
// E_warp, the flow-warping temporal error of the same result table, follows below them (warp_error_partial_kernel).
#include "common.h"

namespace {

constexpr int NTH = 256;
inline unsigned blocks_for(long long n) { return (unsigned)((n + NTH - 1) / NTH); }

// table layout: T[n][q][c][(H+1)][(W+1)], q = 0..4 for a, b, a*a, b*b, a*b; row 0 and column 0 are zero
__global__ void sat_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ T, int N, int H, int W) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // (n, c, y)
    if (idx >= (long long)N * 3 * (H + 1)) return;
    const int y = (int)(idx % (H + 1));
    const int c = (int)((idx / (H + 1)) % 3);
    const int n = (int)(idx / ((long long)3 * (H + 1)));
    const long long plane = (long long)(H + 1) * (W + 1);
    double* t0 = T + (((long long)n * 5) * 3 + c) * plane + (long long)y * (W + 1);
    const long long qs = 3 * plane;
    for (int q = 0; q < 5; ++q) t0[q * qs] = 0.0;
    if (y == 0) {
        for (int x = 1; x <= W; ++x)
            for (int q = 0; q < 5; ++q) t0[q * qs + x] = 0.0;
        return;
    }
    const float* pa = a + (((long long)n * H + (y - 1)) * W) * 3 + c;
    const float* pb = b + (((long long)n * H + (y - 1)) * W) * 3 + c;
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
    for (int x = 0; x < W; ++x) {
        const double va = (double)pa[(long long)x * 3], vb = (double)pb[(long long)x * 3];
        s0 += va; s1 += vb; s2 += va * va; s3 += vb * vb; s4 += va * vb;
        t0[x + 1] = s0; t0[qs + x + 1] = s1; t0[2 * qs + x + 1] = s2; t0[3 * qs + x + 1] = s3; t0[4 * qs + x + 1] = s4;
    }
}

__global__ void sat_cols_kernel(double* __restrict__ T, int N, int H, int W) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // (n, q, c, x)
    if (idx >= (long long)N * 15 * (W + 1)) return;
    const int x = (int)(idx % (W + 1));
    const long long pl = idx / (W + 1);
    double* t = T + pl * (long long)(H + 1) * (W + 1) + x;
    double s = 0.0;
    for (int y = 1; y <= H; ++y) {
        s += t[(long long)y * (W + 1)];
        t[(long long)y * (W + 1)] = s;
    }
}

__device__ __forceinline__ double block_sum(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < NTH / 64; ++i) s += red[i];
    __syncthreads();
    return s;          // valid in thread 0
}

// per-block partial sums: part[n][0][block] = sum of S over the block's cropped pixels (all channels), part[n][1][block] = sum (a-b)^2
__global__ void ssim_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, const double* __restrict__ T,
                                    double* __restrict__ part, int H, int W, int win, int nblk) {
    __shared__ double red[NTH / 64];
    const int n = blockIdx.y;
    const int pad = (win - 1) / 2;
    const int Hc = H - 2 * pad, Wc = W - 2 * pad;
    const long long ncrop = (long long)3 * Hc * Wc, nall = (long long)3 * H * W;
    const long long plane = (long long)(H + 1) * (W + 1);
    const double NP = (double)win * win, cov_norm = NP / (NP - 1.0);
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double ssum = 0.0, dsum = 0.0;
    for (long long i = (long long)blockIdx.x * NTH + threadIdx.x; i < nall; i += (long long)nblk * NTH) {
        const double d = (double)a[(long long)n * nall + i] - (double)b[(long long)n * nall + i];
        dsum += d * d;
        if (i < ncrop) {
            const int c = (int)(i % 3);
            const int x = (int)((i / 3) % Wc);
            const int y = (int)(i / ((long long)3 * Wc));
            // window rows [y, y + win), columns [x, x + win) of the image (centre (y + pad, x + pad))
            double m[5];
            for (int q = 0; q < 5; ++q) {
                const double* t = T + (((long long)n * 5 + q) * 3 + c) * plane;
                const double s = t[(long long)(y + win) * (W + 1) + x + win] - t[(long long)y * (W + 1) + x + win] -
                                 t[(long long)(y + win) * (W + 1) + x] + t[(long long)y * (W + 1) + x];
                m[q] = s / NP;
            }
            const double ux = m[0], uy = m[1];
            const double vx = cov_norm * (m[2] - ux * ux), vy = cov_norm * (m[3] - uy * uy), vxy = cov_norm * (m[4] - ux * uy);
            const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
            ssum += (A1 * A2) / (B1 * B2);
        }
    }
    const double s = block_sum(ssum, red);
    const double d = block_sum(dsum, red);
    if (threadIdx.x == 0) {
        part[((long long)n * 2 + 0) * nblk + blockIdx.x] = s;
        part[((long long)n * 2 + 1) * nblk + blockIdx.x] = d;
    }
}

__global__ void metrics_final_kernel(const double* __restrict__ part, double* __restrict__ out, int N, int H, int W, int win, int nblk) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double s = 0.0, d = 0.0;
    for (int i = 0; i < nblk; ++i) { s += part[((long long)n * 2 + 0) * nblk + i]; d += part[((long long)n * 2 + 1) * nblk + i]; }
    const int pad = (win - 1) / 2;
    const double mse = d / ((double)3 * H * W);
    out[2 * n + 0] = mse == 0.0 ? (double)INFINITY : 20.0 * log10(255.0 / sqrt(mse));
    out[2 * n + 1] = s / ((double)3 * (H - 2 * pad) * (W - 2 * pad));
}

constexpr int PART_BLOCKS = 256;

// ------------------------------------------------------------------------------------------------ E_warp
// The flow-warping temporal error (Lai et al., ECCV 2018; occlusion test of Ruder et al. 2016), fp64 on fp32 / uint8 inputs.
// Pair t: A = frames[t], B = frames[t+1], f = fwd[t] (t -> t+1 on frame t's grid, pixels, channel 0 = x), g = bwd[t] (t+1 -> t
// on frame t+1's grid).  For pixel p = (x, y):
//   q = (x + f_x(p), y + f_y(p));  inside = 0 <= q_x <= W-1 and 0 <= q_y <= H-1, decided in floating point BEFORE any conversion
//       to an integer (a flow of 1e30, inf or nan is simply outside);
//   bil(T, q) = 4-corner bilinear sample, corners outside the image contribute 0 (flow_warp(padding_mode='zeros'), i.e.
//       grid_sample(align_corners=True));  g_w = bil(g, q), B_w = bil(B, q);
//   occluded        |f + g_w|^2 > 0.01 (|f|^2 + |g_w|^2) + 0.5;
//   motion boundary |dx f|^2 + |dy f|^2 > 0.01 |f|^2 + 0.002, dx f = f(x+1,y) - f(x,y), dy f = f(x,y+1) - f(x,y), 0 on the last
//       column / row;
//   M(p) = inside, not occluded, no motion boundary, valid[t](p) != 0 (if given), and f(p), the neighbours of f used above and g_w
//       finite.  Exclusion is a select: an excluded pixel's terms are never formed and multiplied by 0 (that is how the deformable
//       conv once produced NaN).
//   n_t = sum M;  e_t = sum_p M(p) sum_c ((A_c - B_w,c) / 255)^2 / n_t, 0 when n_t = 0.
// One thread per pixel, the pair on the grid's y axis; wave reduction by shuffles, block reduction through LDS, one (sum, count)
// partial per block; a second kernel adds each pair's partials in a fixed order.  No atomics: the same bits every run.  The count
// is an integer until the last step (a double holds it exactly: H W < 2^31).
__device__ __forceinline__ double we_load(const float* p) { return (double)*p; }
__device__ __forceinline__ double we_load(const uint8_t* p) { return (double)*p; }

__device__ __forceinline__ unsigned block_count(unsigned v, unsigned* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) red[w] = v;
    __syncthreads();
    unsigned s = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < NTH / 64; ++i) s += red[i];
    __syncthreads();
    return s;          // valid in thread 0
}

template <typename T>
__global__ void __launch_bounds__(NTH)
warp_error_partial_kernel(const T* __restrict__ frames, const float* __restrict__ fwd, const float* __restrict__ bwd,
                          const uint8_t* __restrict__ valid, double* __restrict__ part, int H, int W, int nblk) {
    __shared__ double red[NTH / 64];
    __shared__ unsigned redn[NTH / 64];
    const int t = blockIdx.y;
    const long long HW = (long long)H * W;
    const long long idx = (long long)blockIdx.x * NTH + threadIdx.x;
    double err = 0.0;
    unsigned keep = 0;
    if (idx < HW) {
        const int x = (int)(idx % W), y = (int)(idx / W);
        const float* f = fwd + ((long long)t * HW + idx) * 2;
        const double fx = (double)f[0], fy = (double)f[1];
        bool ok = isfinite(fx) && isfinite(fy);
        double grad = 0.0;
        if (x + 1 < W) {
            const double rx = (double)f[2], ry = (double)f[3];
            ok = ok && isfinite(rx) && isfinite(ry);
            grad += (rx - fx) * (rx - fx) + (ry - fy) * (ry - fy);
        }
        if (y + 1 < H) {
            const double lx = (double)f[2 * (long long)W], ly = (double)f[2 * (long long)W + 1];
            ok = ok && isfinite(lx) && isfinite(ly);
            grad += (lx - fx) * (lx - fx) + (ly - fy) * (ly - fy);
        }
        const double ff = fx * fx + fy * fy;
        const double qx = (double)x + fx, qy = (double)y + fy;
        // comparisons with a NaN are false: a non-finite q is outside
        const bool inside = qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
        ok = ok && inside && !(grad > 0.01 * ff + 0.002);
        if (valid) ok = ok && valid[(long long)t * HW + idx] != 0;
        if (ok) {
            // 0 <= q <= size - 1 holds here, so the conversions are in range; x0 + 1 can be W (q_x = W - 1): that corner is outside
            const int x0 = (int)floor(qx), y0 = (int)floor(qy);
            const double wx1 = qx - (double)x0, wy1 = qy - (double)y0;
            const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
            const bool hx = x0 + 1 < W, hy = y0 + 1 < H;
            const double w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
            const long long o00 = (long long)y0 * W + x0, o01 = o00 + 1, o10 = o00 + W, o11 = o10 + 1;
            const float* g = bwd + (long long)t * HW * 2;
            double gx = w00 * (double)g[o00 * 2], gy = w00 * (double)g[o00 * 2 + 1];
            if (hx) { gx += w01 * (double)g[o01 * 2]; gy += w01 * (double)g[o01 * 2 + 1]; }
            if (hy) { gx += w10 * (double)g[o10 * 2]; gy += w10 * (double)g[o10 * 2 + 1]; }
            if (hx && hy) { gx += w11 * (double)g[o11 * 2]; gy += w11 * (double)g[o11 * 2 + 1]; }
            const double sx = fx + gx, sy = fy + gy;
            ok = isfinite(gx) && isfinite(gy) && !(sx * sx + sy * sy > 0.01 * (ff + gx * gx + gy * gy) + 0.5);
            if (ok) {
                const T* A = frames + ((long long)t * HW + idx) * 3;
                const T* B = frames + (long long)(t + 1) * HW * 3;
                double e = 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double b = w00 * we_load(B + o00 * 3 + c);
                    if (hx) b += w01 * we_load(B + o01 * 3 + c);
                    if (hy) b += w10 * we_load(B + o10 * 3 + c);
                    if (hx && hy) b += w11 * we_load(B + o11 * 3 + c);
                    const double d = (we_load(A + c) - b) / 255.0;
                    e += d * d;
                }
                err = e;
                keep = 1;
            }
        }
    }
    const double s = block_sum(err, red);
    const unsigned n = block_count(keep, redn);
    if (threadIdx.x == 0) {
        part[((long long)t * 2 + 0) * nblk + blockIdx.x] = s;
        part[((long long)t * 2 + 1) * nblk + blockIdx.x] = (double)n;
    }
}

// one block per pair: thread i adds partials i, i + NTH, ... in order, the block adds its threads in order
__global__ void __launch_bounds__(NTH) warp_error_final_kernel(const double* __restrict__ part, double* __restrict__ out, int nblk) {
    __shared__ double red[NTH / 64];
    const int t = blockIdx.x;
    double s = 0.0, n = 0.0;
    for (int i = threadIdx.x; i < nblk; i += NTH) {
        s += part[((long long)t * 2 + 0) * nblk + i];
        n += part[((long long)t * 2 + 1) * nblk + i];          // integers below 2^31: exact in any order
    }
    s = block_sum(s, red);
    n = block_sum(n, red);
    if (threadIdx.x == 0) {
        out[2 * t + 0] = n > 0.0 ? s / n : 0.0;
        out[2 * t + 1] = n;
    }
}

}  // namespace

extern "C" int64_t e2fgvi_warp_error_workspace(int32_t L, int32_t H, int32_t W) {
    if (L < 2 || H <= 0 || W <= 0 || (int64_t)H * W >= 2147483647LL - NTH) {
        e2fgvi_set_error("warp_error_workspace: bad sizes");
        return E2FGVI_EINVAL;
    }
    return (int64_t)(L - 1) * 2 * (int64_t)blocks_for((long long)H * W) * 8;
}

extern "C" int e2fgvi_warp_error(const void* frames, int32_t frame_dtype, const float* fwd, const float* bwd, const uint8_t* valid,
                                 int32_t L, int32_t H, int32_t W, void* workspace, double* out, void* stream) {
    E2_REQUIRE(frames && fwd && bwd && workspace && out, E2FGVI_EINVAL, "warp_error: null pointer");
    E2_REQUIRE(L >= 2 && L <= 65536, E2FGVI_EINVAL, "warp_error: needs 2 <= L <= 65536 frames, got %d", L);
    E2_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < 2147483647LL - NTH, E2FGVI_EINVAL, "warp_error: bad sizes %d x %d", H, W);
    E2_REQUIRE(frame_dtype == E2FGVI_F32 || frame_dtype == E2FGVI_U8, E2FGVI_EINVAL, "warp_error: frames must be E2FGVI_F32 or E2FGVI_U8");
    E2_REQUIRE(((uintptr_t)workspace & 7) == 0, E2FGVI_EINVAL, "warp_error: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)blocks_for((long long)H * W);
    double* part = (double*)workspace;
    if (frame_dtype == E2FGVI_U8)
        hipLaunchKernelGGL(warp_error_partial_kernel<uint8_t>, dim3(nblk, L - 1, 1), dim3(NTH), 0, st, (const uint8_t*)frames, fwd, bwd,
                           valid, part, H, W, nblk);
    else
        hipLaunchKernelGGL(warp_error_partial_kernel<float>, dim3(nblk, L - 1, 1), dim3(NTH), 0, st, (const float*)frames, fwd, bwd,
                           valid, part, H, W, nblk);
    hipLaunchKernelGGL(warp_error_final_kernel, dim3(L - 1), dim3(NTH), 0, st, part, out, nblk);
    E2_LAUNCH_CHECK("warp_error");
    return 0;
}

extern "C" int64_t e2fgvi_psnr_ssim_workspace(int32_t N, int32_t H, int32_t W) {
    if (N <= 0 || H <= 0 || W <= 0) { e2fgvi_set_error("psnr_ssim_workspace: bad sizes"); return E2FGVI_EINVAL; }
    return ((int64_t)N * 15 * (H + 1) * (W + 1) + (int64_t)N * 2 * PART_BLOCKS) * 8;
}

extern "C" int e2fgvi_psnr_ssim(const float* img1, const float* img2, int32_t N, int32_t H, int32_t W, int32_t win_size,
                                void* workspace, double* out, void* stream) {
    E2_REQUIRE(img1 && img2 && workspace && out && N > 0 && H > 0 && W > 0, E2FGVI_EINVAL, "psnr_ssim: bad arguments");
    E2_REQUIRE(N <= 65535, E2FGVI_EINVAL, "psnr_ssim: at most 65535 image pairs per call (the grid's y axis), got %d", N);
    E2_REQUIRE(win_size >= 3 && (win_size & 1) && win_size <= H && win_size <= W, E2FGVI_EINVAL,
               "psnr_ssim: win_size must be odd, >= 3 and <= min(H, W)");
    E2_REQUIRE(((uintptr_t)workspace & 7) == 0, E2FGVI_EINVAL, "psnr_ssim: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double* T = (double*)workspace;
    double* part = T + (long long)N * 15 * (H + 1) * (W + 1);
    hipLaunchKernelGGL(sat_rows_kernel, dim3(blocks_for((long long)N * 3 * (H + 1))), dim3(NTH), 0, st, img1, img2, T, N, H, W);
    hipLaunchKernelGGL(sat_cols_kernel, dim3(blocks_for((long long)N * 15 * (W + 1))), dim3(NTH), 0, st, T, N, H, W);
    hipLaunchKernelGGL(ssim_partial_kernel, dim3(PART_BLOCKS, N, 1), dim3(NTH), 0, st, img1, img2, T, part, H, W, win_size, PART_BLOCKS);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(blocks_for(N)), dim3(NTH), 0, st, part, out, N, H, W, win_size, PART_BLOCKS);
    E2_LAUNCH_CHECK("psnr_ssim");
    return 0;
}
