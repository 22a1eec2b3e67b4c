// Real pixels for restored holes (video.propagate_pixels): for every hole pixel, WHERE IN WHICH FRAME its colour can be seen, carried
// along the flows of metrics.video_flows, and one bilinear read of that colour at the end.  Coordinates travel, not colours: a pixel
// reached after 20 steps has been sampled once, not 20 times.  fp64 on the fp32 / uint8 inputs like mask_track.hip, in the order
// written and without FMA contraction (this unit is built with -ffp-contract=off: the numpy restatement of
// tests/pixel_track_cases.py matches it bit for bit).
//   hole   uint8 [L][H][W] of 0 / 1
//   fwd, bwd [L-1][H][W][2] fp32 in warp_error's convention (fwd[t]: t -> t+1 on t's grid, bwd[t]: t+1 -> t on t+1's grid, pixels,
//       channel 0 = x)
//   age    uint8 [2][L][H][W]: 255 = not reached, 0 = a known pixel, a = reached after a steps; the caller sets both planes to
//       255 * hole.  Plane 0 travels forward in time, plane 1 backward.
//   origin fp32 [2][L][H][W][2] = (x, y), meaningful only where 1 <= age <= 254 (a pixel of age 0 is its own origin): the origin of
//       a reached pixel of frame d lies in frame d - age (plane 0) or d + age (plane 1)
//   jobs   int32 [n][2] = (pair t, dir) on the device
// The step: dir 0 reads frame s = t and writes frame d = t+1 of plane 0 with the pull flow g = bwd[t] and the check flow
// c = fwd[t]; dir 1 reads frame s = t+1 and writes frame d = t of plane 1 with g = fwd[t] and c = bwd[t].  For a destination pixel
// p = (x, y) with hole[d](p) == 1 (no other pixel is touched):
//   q = (x + g_x(p), y + g_y(p));  inside = g(p) finite, 0 <= q_x <= W-1 and 0 <= q_y <= H-1, decided in floating point before any
//       conversion to an integer;
//   c* = (floor(q_x + 0.5), floor(q_y + 0.5)), the nearest pixel, a half goes up;  a = age[dir][s](c*);
//   c_w = bil(c, q) and `inconsistent` exactly as in mask_track.hip;
//   reached = inside and a != 255 and a + 1 <= reach and (check == 0 or not inconsistent);
//   reached:  age[dir][d](p) = a + 1,  origin[dir][d](p) = O_c + (q - c*) per component -- the difference first, then the sum, the
//       sum rounded to fp32 by the store -- with O_c = c* when a == 0 and origin[dir][s](c*) widened to fp64 otherwise;
//   otherwise age[dir][d](p) = 255 (the origin keeps what it held).
// The nearest REACHED pixel, not an interpolation of the four origins around q: they may lie in different frames.
// A thread owns four consecutive pixels of a row.  It reads their hole bytes (one dword when the address allows) and is done when
// none is set: the common case, and what makes a step over a large frame with a small hole cheap.  The job is the grid's y axis; a
// job outside [0, L-1) x {0, 1} writes nothing.  No atomics: the same inputs give the same bits.  Within a launch no job may write
// a frame of a plane that another job reads or writes (video.plan_pixel_chains guarantees it).
// The fill: one launch over all frames, see pixel_fill_kernel.
#include "frame_bytes.h"          // the launch in slabs

namespace {

constexpr int PT_NTH = 256;
constexpr int PT_PX = 4;              // pixels per thread

// the hole bytes of a thread's nx pixels at h, one per byte of the result
__device__ __forceinline__ unsigned pt_hole_bytes(const uint8_t* h, int nx) {
    if (nx == PT_PX && ((uintptr_t)h & 3) == 0) return *reinterpret_cast<const unsigned*>(h);
    unsigned v = 0u;
#pragma unroll
    for (int j = 0; j < PT_PX; ++j)
        if (j < nx) v |= (unsigned)h[j] << (8 * j);
    return v;
}

// one destination pixel of a step: writes its age byte and, when it is reached, its origin
__device__ __forceinline__ void pt_pixel(const uint8_t* A, const float* O, uint8_t* dA, float* dO, const float* __restrict__ g,
                                         const float* __restrict__ c, int x, int y, int H, int W, int reach, int check) {
    const long long p = (long long)y * W + x;
    const float2 gv = *reinterpret_cast<const float2*>(g + p * 2);
    const double gx = (double)gv.x, gy = (double)gv.y;
    const double qx = (double)x + gx, qy = (double)y + gy;
    // comparisons with a NaN are false and x + inf is inf: a non-finite g is outside either way; the test says so itself
    const bool inside = isfinite(gx) && isfinite(gy) && qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
    dA[p] = 255;
    if (!inside) return;
    // 0 <= q <= size - 1 holds here, so every conversion is in range and so is the nearest pixel: q + 0.5 <= size - 0.5
    const double nx_ = floor(qx + 0.5), ny_ = floor(qy + 0.5);
    const long long on = (long long)(int)ny_ * W + (int)nx_;
    const int a = (int)A[on];
    if (a == 255 || a + 1 > reach) return;
    if (check) {
        // x0 + 1 can be W (q_x = W - 1): that corner is outside
        const int x0 = (int)floor(qx), y0 = (int)floor(qy);
        const double wx1 = qx - (double)x0, wy1 = qy - (double)y0;
        const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
        const bool hx = x0 + 1 < W, hy = y0 + 1 < H;
        const double w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
        const long long o00 = (long long)y0 * W + x0, o01 = o00 + 1, o10 = o00 + W, o11 = o10 + 1;
        double cx = w00 * (double)c[o00 * 2], cy = w00 * (double)c[o00 * 2 + 1];
        if (hx) { cx += w01 * (double)c[o01 * 2]; cy += w01 * (double)c[o01 * 2 + 1]; }
        if (hy) { cx += w10 * (double)c[o10 * 2]; cy += w10 * (double)c[o10 * 2 + 1]; }
        if (hx && hy) { cx += w11 * (double)c[o11 * 2]; cy += w11 * (double)c[o11 * 2 + 1]; }
        if (!(isfinite(cx) && isfinite(cy))) return;
        const double sx = gx + cx, sy = gy + cy;
        const double lhs = sx * sx + sy * sy;
        const double rhs = 0.01 * ((gx * gx + gy * gy) + (cx * cx + cy * cy)) + 0.5;
        if (lhs > rhs) return;
    }
    double ox = nx_, oy = ny_;
    if (a != 0) {
        const float2 ov = *reinterpret_cast<const float2*>(O + on * 2);
        ox = (double)ov.x;
        oy = (double)ov.y;
    }
    const double dx = qx - nx_, dy = qy - ny_;
    float2 out;
    out.x = (float)(ox + dx);
    out.y = (float)(oy + dy);
    *reinterpret_cast<float2*>(dO + p * 2) = out;
    dA[p] = (uint8_t)(a + 1);
}

__global__ void __launch_bounds__(PT_NTH)
pixel_track_step_kernel(const uint8_t* __restrict__ hole, uint8_t* age, float* origin, const float* __restrict__ fwd,
                        const float* __restrict__ bwd, const int* __restrict__ jobs, int L, int H, int W, int wq, int reach, int check) {
    const int t = jobs[2 * blockIdx.y], dir = jobs[2 * blockIdx.y + 1];
    if (t < 0 || t >= L - 1 || (dir != 0 && dir != 1)) return;          // a table entry outside the video: nothing is written
    const long long idx = (long long)blockIdx.x * PT_NTH + threadIdx.x;  // (y, four-pixel group)
    if (idx >= (long long)H * wq) return;
    const int y = (int)(idx / wq), xb = (int)(idx % wq) * PT_PX;
    const long long HW = (long long)H * W;
    const long long src_f = dir ? t + 1 : t, dst_f = dir ? t : t + 1;
    const int nx = W - xb < PT_PX ? W - xb : PT_PX;
    const unsigned hb = pt_hole_bytes(hole + dst_f * HW + (long long)y * W + xb, nx);
    if (hb == 0u) return;                                                // no hole pixel among the four: one dword read
    const uint8_t* A = age + ((long long)dir * L + src_f) * HW;
    const float* O = origin + ((long long)dir * L + src_f) * HW * 2;
    uint8_t* dA = age + ((long long)dir * L + dst_f) * HW;
    float* dO = origin + ((long long)dir * L + dst_f) * HW * 2;
    const float* g = (dir ? fwd : bwd) + (long long)t * HW * 2;
    const float* c = (dir ? bwd : fwd) + (long long)t * HW * 2;
#pragma unroll
    for (int j = 0; j < PT_PX; ++j)
        if (j < nx && ((hb >> (8 * j)) & 0xffu) == 1u) pt_pixel(A, O, dA, dO, g, c, xb + j, y, H, W, reach, check);
}

// One candidate of the fill: the plane's age a and origin at the pixel (x, y) of frame t.  Holds iff its frame f = t -+ a is in the
// video, the origin is finite and in the image, and every one of the four bilinear corners with non-zero weight lies in the image
// and is no hole pixel of f; then rgb gets the rounded sample.
__device__ __forceinline__ bool pt_candidate(const uint8_t* __restrict__ src, const uint8_t* __restrict__ hole, const float* O, int pl,
                                             int a, int t, int x, int y, int L, int H, int W, unsigned rgb[3]) {
    const int f = pl ? t + a : t - a;
    if (f < 0 || f >= L) return false;
    double ox = (double)x, oy = (double)y;
    if (a != 0) {
        const float2 ov = *reinterpret_cast<const float2*>(O);
        ox = (double)ov.x;
        oy = (double)ov.y;
    }
    if (!(isfinite(ox) && isfinite(oy) && ox >= 0.0 && ox <= (double)(W - 1) && oy >= 0.0 && oy <= (double)(H - 1))) return false;
    const int x0 = (int)floor(ox), y0 = (int)floor(oy);
    const double wx1 = ox - (double)x0, wy1 = oy - (double)y0;
    const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
    const bool hx = x0 + 1 < W, hy = y0 + 1 < H;
    const double w[4] = {wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1};
    const bool in[4] = {true, hx, hy, hx && hy};
    const long long o00 = (long long)y0 * W + x0;
    const long long off[4] = {o00, o00 + 1, o00 + W, o00 + W + 1};
    const uint8_t* Hf = hole + (long long)f * H * W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (w[k] != 0.0 && (!in[k] || Hf[off[k]] != 0)) return false;
    }
    const uint8_t* S = src + (long long)f * H * W * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double s = w[0] * (double)S[off[0] * 3 + ch];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (in[k]) s += w[k] * (double)S[off[k] * 3 + ch];
        const double r = floor(s + 0.5);
        rgb[ch] = r >= 255.0 ? 255u : (unsigned)r;
    }
    return true;
}

// out[t](p) for every hole pixel p: the candidates are the two planes in the order of their ages (a tie goes to plane 0; age 255 is
// no candidate), the first that holds wins, and when none holds out keeps its byte.  source (or NULL): 0 = no hole pixel, 1 = plane
// 0, 2 = plane 1, 3 = a hole pixel left as it was.
__global__ void __launch_bounds__(PT_NTH)
pixel_fill_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ hole, const uint8_t* __restrict__ age,
                  const float* __restrict__ origin, uint8_t* out, uint8_t* source, int t0, int L, int H, int W, int wq) {
    const int t = t0 + (int)blockIdx.y;
    const long long idx = (long long)blockIdx.x * PT_NTH + threadIdx.x;
    if (idx >= (long long)H * wq) return;
    const int y = (int)(idx / wq), xb = (int)(idx % wq) * PT_PX;
    const long long HW = (long long)H * W;
    const long long row = (long long)t * HW + (long long)y * W + xb;
    const int nx = W - xb < PT_PX ? W - xb : PT_PX;
    const unsigned hb = pt_hole_bytes(hole + row, nx);
    unsigned sb = 0u;
    if (hb != 0u) {
#pragma unroll
        for (int j = 0; j < PT_PX; ++j) {
            if (j >= nx || ((hb >> (8 * j)) & 0xffu) != 1u) continue;
            const long long p = row + j;
            const int a0 = (int)age[p], a1 = (int)age[(long long)L * HW + p];
            const int first = a0 <= a1 ? 0 : 1;
            unsigned rgb[3], from = 3u;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int pl = k == 0 ? first : 1 - first;
                const int a = pl ? a1 : a0;
                if (from != 3u || a == 255) continue;
                if (pt_candidate(src, hole, origin + ((long long)pl * L * HW + p) * 2, pl, a, t, xb + j, y, L, H, W, rgb))
                    from = (unsigned)pl + 1u;
            }
            if (from != 3u) {
                out[p * 3] = (uint8_t)rgb[0];
                out[p * 3 + 1] = (uint8_t)rgb[1];
                out[p * 3 + 2] = (uint8_t)rgb[2];
            }
            sb |= from << (8 * j);
        }
    }
    if (source) {
        uint8_t* S = source + row;
        if (nx == PT_PX && ((uintptr_t)S & 3) == 0) {
            *reinterpret_cast<unsigned*>(S) = sb;
        } else {
#pragma unroll
            for (int j = 0; j < PT_PX; ++j)
                if (j < nx) S[j] = (uint8_t)(sb >> (8 * j));
        }
    }
}

}  // namespace

extern "C" int e2fgvi_pixel_track_step(const uint8_t* hole, uint8_t* age, float* origin, const float* fwd, const float* bwd,
                                       const int32_t* jobs, int32_t n, int32_t L, int32_t H, int32_t W, int32_t reach, int32_t check,
                                       void* stream) {
    E2_REQUIRE(n >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "pixel_track_step: negative size (n = %d, H = %d, W = %d)", n, H, W);
    E2_REQUIRE(L >= 2, E2FGVI_EINVAL, "pixel_track_step: needs L >= 2 frames, got %d", L);
    E2_REQUIRE(reach >= 1 && reach <= 254, E2FGVI_EINVAL, "pixel_track_step: reach must be in [1, 254], got %d", reach);
    E2_REQUIRE(check == 0 || check == 1, E2FGVI_EINVAL, "pixel_track_step: check must be 0 or 1, got %d", check);
    E2_REQUIRE((int64_t)H * W < 2147483647LL - 256, E2FGVI_EINVAL, "pixel_track_step: needs H * W < 2^31 - 256, got %d x %d", H, W);
    if (n == 0 || (int64_t)H * W == 0) return 0;        // no work: no launch, and the pointers are not looked at
    E2_REQUIRE(hole && age && origin && fwd && bwd && jobs, E2FGVI_EINVAL, "pixel_track_step: null pointer");
    E2_REQUIRE(((uintptr_t)fwd & 7) == 0 && ((uintptr_t)bwd & 7) == 0 && ((uintptr_t)origin & 7) == 0 && ((uintptr_t)jobs & 3) == 0,
               E2FGVI_EINVAL, "pixel_track_step: fwd, bwd and origin must be 8-byte aligned, jobs 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int wq = (W + PT_PX - 1) / PT_PX;
    const unsigned nblk = (unsigned)(((long long)H * wq + PT_NTH - 1) / PT_NTH);
    return fb_slabs("pixel_track_step", n, [&](int j0, unsigned nj) {
        hipLaunchKernelGGL(pixel_track_step_kernel, dim3(nblk, nj), dim3(PT_NTH), 0, st, hole, age, origin, fwd, bwd, jobs + 2LL * j0, L,
                           H, W, wq, reach, check);
    });
}

extern "C" int e2fgvi_pixel_fill(const uint8_t* src, const uint8_t* hole, const uint8_t* age, const float* origin, uint8_t* out,
                                 uint8_t* source, int32_t L, int32_t H, int32_t W, void* stream) {
    E2_REQUIRE(L >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "pixel_fill: negative size (L = %d, H = %d, W = %d)", L, H, W);
    E2_REQUIRE((int64_t)H * W < 2147483647LL - 256, E2FGVI_EINVAL, "pixel_fill: needs H * W < 2^31 - 256, got %d x %d", H, W);
    if (L == 0 || (int64_t)H * W == 0) return 0;        // no work: no launch, and the pointers are not looked at
    E2_REQUIRE(src && hole && age && origin && out, E2FGVI_EINVAL, "pixel_fill: null pointer");
    E2_REQUIRE(((uintptr_t)origin & 7) == 0, E2FGVI_EINVAL, "pixel_fill: origin must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int wq = (W + PT_PX - 1) / PT_PX;
    const unsigned nblk = (unsigned)(((long long)H * wq + PT_NTH - 1) / PT_NTH);
    return fb_slabs("pixel_fill", L, [&](int t0, unsigned nt) {
        hipLaunchKernelGGL(pixel_fill_kernel, dim3(nblk, nt), dim3(PT_NTH), 0, st, src, hole, age, origin, out, source, t0, L, H, W, wq);
    });
}
