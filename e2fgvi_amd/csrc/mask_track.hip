// Masks from keyframes (video.propagate_masks, inpaint_video(mask_keys=)): one step of pulling a binary mask along the flows of
// metrics.video_flows, fp64 on the fp32 / uint8 inputs like E_warp (metrics.hip), in the order written and without FMA contraction
// (this unit is built with -ffp-contract=off: the numpy restatement of tests/mask_key_cases.py matches it bit for bit).
//   planes uint8 [2][L][H][W] of 0 / 1: plane 0 is carried forward in time, plane 1 backward
//   fwd, bwd [L-1][H][W][2] fp32 in warp_error's convention (fwd[t]: t -> t+1 on t's grid, bwd[t]: t+1 -> t on t+1's grid, pixels,
//       channel 0 = x)
//   jobs int32 [n][2] = (pair t, dir) on the device
// dir 0 reads plane 0 frame t and writes plane 0 frame t+1 with the pull flow g = bwd[t] and the check flow c = fwd[t];
// dir 1 reads plane 1 frame t+1 and writes plane 1 frame t with g = fwd[t] and c = bwd[t].  For a destination pixel p = (x, y) and
// the source mask M:
//   q = (x + g_x(p), y + g_y(p));  inside = g(p) finite, 0 <= q_x <= W-1 and 0 <= q_y <= H-1, decided in floating point before any
//       conversion to an integer;
//   bil(T, q) = the 4-corner bilinear sample of e2fgvi_warp_error, corners outside the image contribute 0, corners added in the
//       order (y0,x0), (y0,x0+1), (y0+1,x0), (y0+1,x0+1);  s = bil(M, q), c_w = bil(c, q);
//   inconsistent = c_w not finite, or  sx sx + sy sy > 0.01 ((g_x g_x + g_y g_y) + (c_wx c_wx + c_wy c_wy)) + 0.5  with
//       sx = g_x + c_wx, sy = g_y + c_wy;
//   dst(p) = 1 iff inside and s >= 0.5 and (check == 0 or not inconsistent).
// Excluded pixels are dropped by select: nothing of them is formed and multiplied by 0.  The 32-byte gather of c is done only for
// pixels that passed `inside` and s >= 0.5 -- most pixels lie outside the mask, and the result is the same.
// A thread owns four consecutive pixels of a row and stores them as one dword when the address allows, bytes otherwise (W % 4 != 0,
// rows that are not dword-aligned).  The job is the grid's y axis; a job outside [0, L-1) x {0, 1} writes nothing.  No atomics: the
// same inputs give the same bits.  Within a launch no job may write a frame of a plane that another job reads or writes
// (video.plan_mask_chains guarantees it).
#include "frame_bytes.h"          // the launch in slabs

namespace {

constexpr int MT_NTH = 256;
constexpr int MT_PX = 4;              // pixels per thread

__device__ __forceinline__ unsigned mt_pixel(const uint8_t* M, const float* __restrict__ g, const float* __restrict__ c,
                                             int x, int y, int H, int W, int check) {
    const long long p = (long long)y * W + x;
    const float2 gv = *reinterpret_cast<const float2*>(g + p * 2);
    const double gx = (double)gv.x, gy = (double)gv.y;
    const double qx = (double)x + gx, qy = (double)y + gy;
    // comparisons with a NaN are false and x + inf is inf: a non-finite g is outside either way; the test says so itself
    const bool inside = isfinite(gx) && isfinite(gy) && qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
    if (!inside) return 0u;
    // 0 <= q <= size - 1 holds here, so the conversions are in range; x0 + 1 can be W (q_x = W - 1): that corner is outside
    const int x0 = (int)floor(qx), y0 = (int)floor(qy);
    const double wx1 = qx - (double)x0, wy1 = qy - (double)y0;
    const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
    const bool hx = x0 + 1 < W, hy = y0 + 1 < H;
    const double w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
    const long long o00 = (long long)y0 * W + x0, o01 = o00 + 1, o10 = o00 + W, o11 = o10 + 1;
    double s = w00 * (double)M[o00];
    if (hx) s += w01 * (double)M[o01];
    if (hy) s += w10 * (double)M[o10];
    if (hx && hy) s += w11 * (double)M[o11];
    if (!(s >= 0.5)) return 0u;
    if (!check) return 1u;
    double cx = w00 * (double)c[o00 * 2], cy = w00 * (double)c[o00 * 2 + 1];
    if (hx) { cx += w01 * (double)c[o01 * 2]; cy += w01 * (double)c[o01 * 2 + 1]; }
    if (hy) { cx += w10 * (double)c[o10 * 2]; cy += w10 * (double)c[o10 * 2 + 1]; }
    if (hx && hy) { cx += w11 * (double)c[o11 * 2]; cy += w11 * (double)c[o11 * 2 + 1]; }
    if (!(isfinite(cx) && isfinite(cy))) return 0u;
    const double sx = gx + cx, sy = gy + cy;
    const double lhs = sx * sx + sy * sy;
    const double rhs = 0.01 * ((gx * gx + gy * gy) + (cx * cx + cy * cy)) + 0.5;
    return lhs > rhs ? 0u : 1u;
}

__global__ void __launch_bounds__(MT_NTH)
mask_track_step_kernel(uint8_t* planes, const float* __restrict__ fwd, const float* __restrict__ bwd,
                       const int* __restrict__ jobs, int L, int H, int W, int wq, int check) {
    const int t = jobs[2 * blockIdx.y], dir = jobs[2 * blockIdx.y + 1];
    if (t < 0 || t >= L - 1 || (dir != 0 && dir != 1)) return;          // a table entry outside the video: nothing is written
    const long long idx = (long long)blockIdx.x * MT_NTH + threadIdx.x;  // (y, four-pixel group)
    if (idx >= (long long)H * wq) return;
    const int y = (int)(idx / wq), xb = (int)(idx % wq) * MT_PX;
    const long long HW = (long long)H * W;
    const long long src_f = dir ? t + 1 : t, dst_f = dir ? t : t + 1;
    const uint8_t* M = planes + ((long long)dir * L + src_f) * HW;
    uint8_t* D = planes + ((long long)dir * L + dst_f) * HW + (long long)y * W + xb;
    const float* g = (dir ? fwd : bwd) + (long long)t * HW * 2;
    const float* c = (dir ? bwd : fwd) + (long long)t * HW * 2;
    const int nx = W - xb < MT_PX ? W - xb : MT_PX;
    unsigned bits[MT_PX];
#pragma unroll
    for (int j = 0; j < MT_PX; ++j) bits[j] = j < nx ? mt_pixel(M, g, c, xb + j, y, H, W, check) : 0u;
    if (nx == MT_PX && ((uintptr_t)D & 3) == 0) {
        *reinterpret_cast<unsigned*>(D) = bits[0] | (bits[1] << 8) | (bits[2] << 16) | (bits[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < MT_PX; ++j)
            if (j < nx) D[j] = (uint8_t)bits[j];
    }
}

}  // namespace

extern "C" int e2fgvi_mask_track_step(uint8_t* planes, const float* fwd, const float* bwd, const int32_t* jobs, int32_t n, int32_t L,
                                      int32_t H, int32_t W, int32_t check, void* stream) {
    E2_REQUIRE(n >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "mask_track_step: negative size (n = %d, H = %d, W = %d)", n, H, W);
    E2_REQUIRE(L >= 2, E2FGVI_EINVAL, "mask_track_step: needs L >= 2 frames, got %d", L);
    E2_REQUIRE(check == 0 || check == 1, E2FGVI_EINVAL, "mask_track_step: check must be 0 or 1, got %d", check);
    E2_REQUIRE((int64_t)H * W < 2147483647LL - 256, E2FGVI_EINVAL, "mask_track_step: needs H * W < 2^31 - 256, got %d x %d", H, W);
    if (n == 0 || (int64_t)H * W == 0) return 0;        // no work: no launch, and the pointers are not looked at
    E2_REQUIRE(planes && fwd && bwd && jobs, E2FGVI_EINVAL, "mask_track_step: null pointer");
    E2_REQUIRE(((uintptr_t)fwd & 7) == 0 && ((uintptr_t)bwd & 7) == 0 && ((uintptr_t)jobs & 3) == 0, E2FGVI_EINVAL,
               "mask_track_step: fwd and bwd must be 8-byte aligned, jobs 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int wq = (W + MT_PX - 1) / MT_PX;
    const unsigned nblk = (unsigned)(((long long)H * wq + MT_NTH - 1) / MT_NTH);
    return fb_slabs("mask_track_step", n, [&](int j0, unsigned nj) {
        hipLaunchKernelGGL(mask_track_step_kernel, dim3(nblk, nj), dim3(MT_NTH), 0, st, planes, fwd, bwd, jobs + 2LL * j0, L, H, W, wq,
                           check);
    });
}
