// Frames between frames (video.retime, video.replace_frames): the picture at a fractional time k / d between two frames A and B,
// gathered along the two flows between them.  include/e2fgvi_hip.h has the definition, tests/interpolate_cases.py restates it in
// numpy, byte for byte.
//   frames uint8 [L][H][W][3];  fwd, bwd fp32 [P][H][W][2] in warp_error's convention (pixels, channel 0 = x)
//   jobs   int32 [n][5] = (ia, ib, fi, k, d) on the device: A = frames[ia], B = frames[ib], fwd[fi]: A -> B on A's grid, bwd[fi]: B -> A
//          on B's grid
//   out    uint8 [n][H][W][3];  source uint8 [n][H][W] or NULL
// Every output pixel p asks both frames which of their pixels passes through p at the time of the output: from A along fwd with
// lambda = k / d, from B along bwd with lambda = (d - k) / d.  A side solves q + lambda h(q) = p for its start q by the fixed point
// q <- p - lambda h(q) from q = p - lambda h(p), `iterations` times, and has `landed` when the residual is within the tolerance;
// it is `two_ended` when the far end q + h(q) lies in the other frame, and `matched` when the colours of the two ends agree.  A
// gather and not a splat: no atomics, so the same inputs give the same bytes.  Coordinates are fp64 on the fp32 inputs like
// mask_track.hip and pixel_track.hip, in the order written and without FMA contraction (this unit is built with
// -ffp-contract=off); the colours are integers on a 1/16 px grid like weave.hip's taps.
// lambda = (double)k / (double)d: a division's expansion is made of fused multiply-adds, which this unit may not hold, so the
// quotients come from a table the compiler fills (IP_LAMBDA), one correctly rounded division each.
// A thread owns four pixels: in a job with k == 0 or k == d four adjacent ones, whose twelve bytes it copies as dwords where the
// addresses allow; in a new frame every 64th of its wave's 256, so that a wave's loads and stores are runs of adjacent pixels.
// The job is the grid's y axis; a job outside its ranges writes nothing.  What binds the kernel is in profiles/interpolate.txt.
#include "frame_bytes.h"          // the launch in slabs and the overlap test

namespace {

constexpr int IP_NTH = 256;
constexpr int IP_PX = 4;              // pixels per thread
constexpr int IP_D_MAX = 64;
constexpr int IP_ITER_MAX = 8;

struct IpLambda { double v[IP_D_MAX + 1][IP_D_MAX + 1]; };
constexpr IpLambda ip_lambda() {
    IpLambda t{};
    for (int d = 1; d <= IP_D_MAX; ++d)
        for (int k = 0; k <= d; ++k) t.v[d][k] = (double)k / (double)d;
    return t;
}
__device__ const IpLambda IP_LAMBDA = ip_lambda();       // v[d][k] = (double)k / (double)d, rounded once, by the compiler

struct IpSide {
    bool landed, two_ended;
    double qx, qy, ex, ey;            // the start in S; the end in E (meaningful when two_ended)
};

__device__ __forceinline__ bool ip_inside(double qx, double qy, int H, int W) {
    // comparisons with a NaN are false and an infinity fails its bound: the test says so itself
    return isfinite(qx) && isfinite(qy) && qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
}

// the four-corner sample of a flow at q, inside(q): corners outside the image contribute nothing, by select
__device__ __forceinline__ void ip_bil(const float* __restrict__ h, double qx, double qy, int H, int W, double& cx, double& cy) {
    // x0 + 1 can be W (q_x = W - 1): that corner is outside
    const int x0 = (int)floor(qx), y0 = (int)floor(qy);
    const double wx1 = qx - (double)x0, wy1 = qy - (double)y0;
    const double wx0 = 1.0 - wx1, wy0 = 1.0 - wy1;
    const bool hx = x0 + 1 < W, hy = y0 + 1 < H;
    const double w00 = wy0 * wx0, w01 = wy0 * wx1, w10 = wy1 * wx0, w11 = wy1 * wx1;
    const long long o00 = (long long)y0 * W + x0, o01 = o00 + 1, o10 = o00 + W, o11 = o10 + 1;
    const float2 v00 = *reinterpret_cast<const float2*>(h + o00 * 2);
    cx = w00 * (double)v00.x;
    cy = w00 * (double)v00.y;
    if (hx) {
        const float2 v = *reinterpret_cast<const float2*>(h + o01 * 2);
        cx += w01 * (double)v.x;
        cy += w01 * (double)v.y;
    }
    if (hy) {
        const float2 v = *reinterpret_cast<const float2*>(h + o10 * 2);
        cx += w10 * (double)v.x;
        cy += w10 * (double)v.y;
    }
    if (hx && hy) {
        const float2 v = *reinterpret_cast<const float2*>(h + o11 * 2);
        cx += w11 * (double)v.x;
        cy += w11 * (double)v.y;
    }
}

// one side's trajectory through the pixel (x, y): h the flow from S to E on S's grid, lam the share of it that lies in front of p
__device__ __forceinline__ IpSide ip_side(const float* __restrict__ h, double lam, int x, int y, int H, int W, int iterations,
                                          double bound) {
    IpSide s;
    s.landed = s.two_ended = false;
    s.qx = s.qy = s.ex = s.ey = 0.0;
    const double px = (double)x, py = (double)y;
    const float2 h0 = *reinterpret_cast<const float2*>(h + ((long long)y * W + x) * 2);
    double qx = px - lam * (double)h0.x, qy = py - lam * (double)h0.y;
    double cx, cy;
    for (int it = 0; it < iterations; ++it) {
        if (!ip_inside(qx, qy, H, W)) return s;
        ip_bil(h, qx, qy, H, W, cx, cy);
        if (!(isfinite(cx) && isfinite(cy))) return s;
        qx = px - lam * cx;
        qy = py - lam * cy;
    }
    if (!ip_inside(qx, qy, H, W)) return s;
    ip_bil(h, qx, qy, H, W, cx, cy);
    if (!(isfinite(cx) && isfinite(cy))) return s;
    const double rx = (qx + lam * cx) - px, ry = (qy + lam * cy) - py;
    if (!(rx * rx + ry * ry <= bound)) return s;
    s.landed = true;
    s.qx = qx;
    s.qy = qy;
    s.ex = qx + cx;
    s.ey = qy + cy;
    s.two_ended = ip_inside(s.ex, s.ey, H, W);
    return s;
}

// the colour of T at q, inside(q), on the 1/16 px grid: 0 <= Q <= 16 (size - 1), so the conversions are in range, the left and upper
// corners lie in the image, and a right or lower corner that does not has weight 0 and is read from the last column or row
__device__ __forceinline__ void ip_tap16(const uint8_t* __restrict__ T, double qx, double qy, int H, int W, int (&c)[3]) {
    // Q can pass 2^31 (16 W) and a conversion of a double to 64 bits is made of fused multiply-adds: Q >> 4 and Q & 15 are taken in
    // fp64, where both are exact, and converted one by one
    const double Qx = floor(qx * 16.0 + 0.5), Qy = floor(qy * 16.0 + 0.5);
    const double Xi = floor(Qx * 0.0625), Yi = floor(Qy * 0.0625);
    const int xi = (int)Xi, fx = (int)(Qx - Xi * 16.0), yi = (int)Yi, fy = (int)(Qy - Yi * 16.0);
    const int x1 = min(xi + 1, W - 1), y1 = min(yi + 1, H - 1);
    const uint8_t* r0 = T + (long long)yi * W * 3;
    const uint8_t* r1 = T + (long long)y1 * W * 3;
    const uint8_t *p00 = r0 + 3 * xi, *p01 = r0 + 3 * x1, *p10 = r1 + 3 * xi, *p11 = r1 + 3 * x1;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
        c[ch] = ((16 - fy) * ((16 - fx) * (int)p00[ch] + fx * (int)p01[ch]) + fy * ((16 - fx) * (int)p10[ch] + fx * (int)p11[ch]) + 128) >> 8;
}

// floor(n / d) for 0 <= n < 2^24 and 1 <= d <= 64, rd = 1 / d to within an ulp: the estimate is off by one at the most
__device__ __forceinline__ int ip_div(int n, int d, float rd) {
    int q = (int)((float)n * rd);
    const int r = n - q * d;
    q += r >= d ? 1 : 0;
    q -= r < 0 ? 1 : 0;
    return q;
}

// one output pixel: its three bytes in the low 24 bits, its source code above them
__device__ __forceinline__ unsigned ip_pixel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B, const float* __restrict__ f,
                                             const float* __restrict__ g, int x, int y, int H, int W, int k, int d, double tau,
                                             double sigma, float rd, int iterations, double bound, int match) {
    const IpSide a = ip_side(f, tau, x, y, H, W, iterations, bound);
    const IpSide b = ip_side(g, sigma, x, y, H, W, iterations, bound);
    int sa[3] = {0, 0, 0}, ta[3] = {0, 0, 0}, sb[3] = {0, 0, 0}, tb[3] = {0, 0, 0};
    int cost_a = 0, cost_b = 0;
    if (a.landed) ip_tap16(A, a.qx, a.qy, H, W, sa);
    if (a.two_ended) {
        ip_tap16(B, a.ex, a.ey, H, W, ta);
        cost_a = abs(sa[0] - ta[0]) + abs(sa[1] - ta[1]) + abs(sa[2] - ta[2]);
    }
    if (b.landed) ip_tap16(B, b.qx, b.qy, H, W, sb);
    if (b.two_ended) {
        ip_tap16(A, b.ex, b.ey, H, W, tb);
        cost_b = abs(sb[0] - tb[0]) + abs(sb[1] - tb[1]) + abs(sb[2] - tb[2]);
    }
    const bool ma = a.two_ended && cost_a <= match, mb = b.two_ended && cost_b <= match;
    const int half = d >> 1, ka = d - k;
    int c[3];
    unsigned code;
    if (ma && (!mb || cost_a <= cost_b)) {
        code = 1u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = ip_div(ka * sa[ch] + k * ta[ch] + half, d, rd);
    } else if (mb) {
        code = 2u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = ip_div(ka * tb[ch] + k * sb[ch] + half, d, rd);
    } else if (a.landed && (!b.landed || 2 * k <= d)) {
        code = 3u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = sa[ch];
    } else if (b.landed) {
        code = 4u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = sb[ch];
    } else {
        code = 0u;
        const long long o = ((long long)y * W + x) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = ip_div(ka * (int)A[o + ch] + k * (int)B[o + ch] + half, d, rd);
    }
    return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16) | (code << 24);
}

__global__ void __launch_bounds__(IP_NTH)
interpolate_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ fwd, const float* __restrict__ bwd,
                   const int* __restrict__ jobs, uint8_t* __restrict__ out, uint8_t* __restrict__ source, int j0, int L, int P, int H,
                   int W, int iterations, double bound, int match) {
    const long long job = (long long)j0 + blockIdx.y;
    const int* jb = jobs + job * 5;
    const int ia = jb[0], ib = jb[1], fi = jb[2], k = jb[3], d = jb[4];
    // a table entry outside its ranges: nothing is written
    if (ia < 0 || ia >= L || ib < 0 || ib >= L || fi < 0 || fi >= P || d < 1 || d > IP_D_MAX || k < 0 || k > d) return;
    const long long HW = (long long)H * W;
    const long long t = (long long)blockIdx.x * IP_NTH + threadIdx.x;    // pixels are numbered along the rows, 0 .. H W - 1
    uint8_t* O = out + job * HW * 3;
    uint8_t* S = source ? source + job * HW : nullptr;
    if (k == 0 || k == d) {
        // a copy of A or of B (the same for the whole workgroup): a thread moves the twelve bytes of four adjacent pixels
        const long long p0 = t * IP_PX;
        if (p0 >= HW) return;
        const int nx = HW - p0 < IP_PX ? (int)(HW - p0) : IP_PX;
        const uint8_t* C = frames + ((long long)(k == 0 ? ia : ib) * HW + p0) * 3;
        uint8_t* o = O + p0 * 3;
        if (nx == IP_PX && (((uintptr_t)C | (uintptr_t)o) & 3) == 0) {
            const unsigned* c4 = reinterpret_cast<const unsigned*>(C);
            unsigned* o4 = reinterpret_cast<unsigned*>(o);
            const unsigned w0 = c4[0], w1 = c4[1], w2 = c4[2];
            o4[0] = w0;
            o4[1] = w1;
            o4[2] = w2;
        } else {
            for (int j = 0; j < 3 * nx; ++j) o[j] = C[j];
        }
        if (S) {
            if (nx == IP_PX && ((uintptr_t)(S + p0) & 3) == 0) {
                *reinterpret_cast<unsigned*>(S + p0) = 0x05050505u;
            } else {
                for (int j = 0; j < nx; ++j) S[p0 + j] = 5;
            }
        }
        return;
    }
    // a new frame: a wave owns 256 adjacent pixels and a lane every 64th of them, so that the 64 pixels a wave works on at a time
    // are adjacent -- their flows are one run of 512 bytes and their bytes one of 192.  (Four ADJACENT pixels a lane, the first
    // version, put a lane's loads 32 bytes apart: every flow line was fetched four times, 33 GB from beyond the L2 where 3 GB
    // are read -- profiles/interpolate.txt.)
    const uint8_t* A = frames + (long long)ia * HW * 3;
    const uint8_t* B = frames + (long long)ib * HW * 3;
    const float* f = fwd + (long long)fi * HW * 2;
    const float* g = bwd + (long long)fi * HW * 2;
    const double tau = IP_LAMBDA.v[d][k], sigma = IP_LAMBDA.v[d][d - k];
    const float rd = __builtin_amdgcn_rcpf((float)d);
    const long long first = (t & ~63LL) * IP_PX + (t & 63);
    for (int j = 0; j < IP_PX; ++j) {
        const long long p = first + 64 * j;
        if (p >= HW) return;
        // p < H W < 2^31: a 32-bit division, a fraction of the 64-bit one's expansion
        const unsigned y_ = (unsigned)p / (unsigned)W;
        const int y = (int)y_, x = (int)((unsigned)p - y_ * (unsigned)W);
        const unsigned px = ip_pixel(A, B, f, g, x, y, H, W, k, d, tau, sigma, rd, iterations, bound, match);
        O[p * 3] = (uint8_t)px;
        O[p * 3 + 1] = (uint8_t)(px >> 8);
        O[p * 3 + 2] = (uint8_t)(px >> 16);
        if (S) S[p] = (uint8_t)(px >> 24);
    }
}

}  // namespace

extern "C" int e2fgvi_interpolate(const uint8_t* frames, const float* fwd, const float* bwd, const int32_t* jobs, uint8_t* out,
                                  uint8_t* source, int32_t n, int32_t L, int32_t P, int32_t H, int32_t W, int32_t iterations,
                                  int32_t tolerance, int32_t match, void* stream) {
    E2_REQUIRE(n >= 0 && L >= 0 && P >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL,
               "interpolate: negative size (n = %d, L = %d, P = %d, H = %d, W = %d)", n, L, P, H, W);
    E2_REQUIRE((int64_t)H * W < 2147483647LL - 256, E2FGVI_EINVAL, "interpolate: needs H * W < 2^31 - 256, got %d x %d", H, W);
    E2_REQUIRE(iterations >= 0 && iterations <= IP_ITER_MAX, E2FGVI_EINVAL, "interpolate: iterations must be in [0, %d], got %d",
               IP_ITER_MAX, iterations);
    E2_REQUIRE(tolerance >= 0 && tolerance <= 255, E2FGVI_EINVAL, "interpolate: tolerance must be in [0, 255], got %d", tolerance);
    E2_REQUIRE(match >= 0 && match <= 765, E2FGVI_EINVAL, "interpolate: match must be in [0, 765], got %d", match);
    if (n == 0 || (int64_t)H * W == 0) return 0;        // no work: no launch, and the pointers are not looked at
    E2_REQUIRE(jobs && out, E2FGVI_EINVAL, "interpolate: null pointer");
    E2_REQUIRE(((uintptr_t)jobs & 3) == 0, E2FGVI_EINVAL, "interpolate: jobs must be 4-byte aligned");
    // without a frame or without a pair every job is outside its ranges and writes nothing: those pointers are not looked at
    E2_REQUIRE(L == 0 || frames, E2FGVI_EINVAL, "interpolate: null pointer");
    E2_REQUIRE(P == 0 || (fwd && bwd), E2FGVI_EINVAL, "interpolate: null pointer");
    E2_REQUIRE(((uintptr_t)fwd & 7) == 0 && ((uintptr_t)bwd & 7) == 0, E2FGVI_EINVAL, "interpolate: fwd and bwd must be 8-byte aligned");
    const uint64_t px = (uint64_t)H * (uint64_t)W;
    E2_REQUIRE(fb_disjoint(frames, 3ull * px * (uint64_t)L, out, 3ull * px * (uint64_t)n), E2FGVI_EINVAL,
               "interpolate: out must not overlap frames (a pixel reads two frames)");
    // nothing that is written may lie on anything that is read, or on the other output: threads of other pixels and jobs read on
    const uint64_t ob = 3ull * px * (uint64_t)n, sb = px * (uint64_t)n, hb = 8ull * px * (uint64_t)P, jn = 20ull * (uint64_t)n;
    E2_REQUIRE(fb_disjoint(fwd, hb, out, ob) && fb_disjoint(bwd, hb, out, ob) && fb_disjoint(jobs, jn, out, ob), E2FGVI_EINVAL,
               "interpolate: out must not overlap fwd, bwd or jobs");
    if (source) {
        E2_REQUIRE(fb_disjoint(frames, 3ull * px * (uint64_t)L, source, sb) && fb_disjoint(out, ob, source, sb) &&
                       fb_disjoint(fwd, hb, source, sb) && fb_disjoint(bwd, hb, source, sb) && fb_disjoint(jobs, jn, source, sb),
                   E2FGVI_EINVAL, "interpolate: source must not overlap frames, fwd, bwd, jobs or out");
    }
    hipStream_t st = (hipStream_t)stream;
    // a workgroup's 256 threads own 1024 adjacent pixels: H W < 2^31, so the grid's x axis is below 2^21
    const unsigned nblk = (unsigned)(((long long)H * W + (long long)IP_NTH * IP_PX - 1) / ((long long)IP_NTH * IP_PX));
    const double bound = (double)(tolerance * tolerance) / 256.0;
    return fb_slabs("interpolate", n, [&](int j0, unsigned nj) {
        hipLaunchKernelGGL(interpolate_kernel, dim3(nblk, nj), dim3(IP_NTH), 0, st, frames, fwd, bwd, jobs, out, source, j0, L, P, H, W,
                           iterations, bound, match);
    });
}
