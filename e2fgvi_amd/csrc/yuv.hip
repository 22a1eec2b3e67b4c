// Pixel formats of the video driver (video.yuv420_to_rgb / rgb_to_yuv420, inpaint_video(pixel_format=)): 8-bit 4:2:0 YUV frames,
// NV12 or I420, to and from the uint8 [L,H,W,3] RGB frames every other byte kernel works on.  Integers only, the definitions of
// include/e2fgvi_hip.h restated in numpy by tests/yuv_cases.py, every byte equal.  HBM-bound: a thread owns a strip of two luma
// rows by YUV_PX pixels (the decoder: YUV_ROWS such strips below one another), so a chroma sample is read once per 2x2 block and
// the loads and stores are 8 bytes wide.  W is only even and a tensor may be a view, so the wide instantiation runs only where the
// host finds W % 8 == 0 and 8-byte aligned bases (then every row, plane and frame starts on a multiple of 4, every strip's luma
// and RGB bytes on a multiple of 8); everything else takes the byte-wise instantiation of the same body.
#include "frame_bytes.h"

namespace {

constexpr int NTH = 256;
constexpr int YUV_PX = 8;        // pixels of a strip: 8 luma bytes, 24 RGB bytes, 4 chroma samples per row
constexpr int YUV_ROWS = 4;      // chroma rows a decoder thread walks down, the rows above and below carried in registers

struct YuvDec { int cy, crv, cgu, cgv, cbu, yo; };
struct YuvEnc { int yr, yg, yb, ur, ug, ub, vr, vg, vb, yo; };

__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// n <= N valid bytes at p -> v[0 .. n) (the rest 0); AL: n == N and p is 8-byte aligned (N = 4: 4-byte aligned)
template <bool AL, int N>
__device__ __forceinline__ void load_bytes(const unsigned char* __restrict__ p, int n, int (&v)[N]) {
    if constexpr (AL && N == 4) {
        const unsigned w = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (int)((w >> (8 * k)) & 255u);
    } else if constexpr (AL) {
        static_assert(N % 8 == 0, "whole 8-byte words");
#pragma unroll
        for (int q = 0; q < N / 8; ++q) {
            const uint2 w = reinterpret_cast<const uint2*>(p)[q];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[8 * q + k] = (int)((w.x >> (8 * k)) & 255u);
                v[8 * q + 4 + k] = (int)((w.y >> (8 * k)) & 255u);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = k < n ? (int)p[k] : 0;
    }
}

// v[0 .. n) (values in [0, 255]) -> n bytes at p, same conditions; the bytes of a word go through fb_byte (frame_bytes.h has why)
template <bool AL, int N>
__device__ __forceinline__ void store_bytes(unsigned char* __restrict__ p, int n, const int (&u)[N]) {
    unsigned v[N];
    if constexpr (AL) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = fb_byte(u[k]);
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = (unsigned)u[k];
    }
    if constexpr (AL && N == 4) {
        *reinterpret_cast<unsigned*>(p) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
    } else if constexpr (AL) {
        static_assert(N % 8 == 0, "whole 8-byte words");
#pragma unroll
        for (int q = 0; q < N / 8; ++q) {
            uint2 w;
            w.x = (unsigned)v[8 * q] | ((unsigned)v[8 * q + 1] << 8) | ((unsigned)v[8 * q + 2] << 16) | ((unsigned)v[8 * q + 3] << 24);
            w.y = (unsigned)v[8 * q + 4] | ((unsigned)v[8 * q + 5] << 8) | ((unsigned)v[8 * q + 6] << 16) | ((unsigned)v[8 * q + 7] << 24);
            reinterpret_cast<uint2*>(p)[q] = w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (k < n) p[k] = (unsigned char)v[k];
    }
}

// Chroma row j of a frame (fc: the first byte behind its luma), columns i0 ... i0 + 4 clamped to the plane: C[0] = U, C[1] = V.
// The fifth column is the right-hand tap of "left" siting at the strip's last odd pixel; where it is not used the load goes away.
template <bool AL>
__device__ __forceinline__ void load_chroma(const unsigned char* __restrict__ fc, int i420, int Hc, int Wc, int j, int i0,
                                            int (&C)[2][5]) {
    const int ie = min(i0 + 4, Wc - 1);
    if (i420) {
        const unsigned char* pu = fc + (long long)j * Wc;
        const unsigned char* pv = pu + (long long)Hc * Wc;
        if constexpr (AL) {
            int u[4], v[4];
            load_bytes<true, 4>(pu + i0, 4, u);
            load_bytes<true, 4>(pv + i0, 4, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) { C[0][k] = u[k]; C[1][k] = v[k]; }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ii = min(i0 + k, Wc - 1);
                C[0][k] = pu[ii];
                C[1][k] = pv[ii];
            }
        }
        C[0][4] = pu[ie];
        C[1][4] = pv[ie];
    } else {
        const unsigned char* p = fc + (long long)j * Wc * 2;
        if constexpr (AL) {
            int b[8];
            load_bytes<true, 8>(p + 2 * i0, 8, b);
#pragma unroll
            for (int k = 0; k < 4; ++k) { C[0][k] = b[2 * k]; C[1][k] = b[2 * k + 1]; }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int ii = min(i0 + k, Wc - 1);
                C[0][k] = p[2 * ii];
                C[1][k] = p[2 * ii + 1];
            }
        }
        C[0][4] = p[2 * ie];
        C[1][4] = p[2 * ie + 1];
    }
}

// nc <= 4 chroma samples of row j from column i0 on: U[k], V[k] -> the frame
template <bool AL>
__device__ __forceinline__ void store_chroma(unsigned char* __restrict__ fc, int i420, int Hc, int Wc, int j, int i0, int nc,
                                             const int (&U)[4], const int (&V)[4]) {
    if (i420) {
        unsigned char* pu = fc + (long long)j * Wc + i0;
        store_bytes<AL, 4>(pu, nc, U);
        store_bytes<AL, 4>(pu + (long long)Hc * Wc, nc, V);
    } else {
        int b[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) { b[2 * k] = U[k]; b[2 * k + 1] = V[k]; }
        store_bytes<AL, 8>(fc + (long long)j * Wc * 2 + 2 * i0, 2 * nc, b);
    }
}

// YUV -> RGB.  Thread idx: strip column sx (fastest: neighbouring lanes read and write neighbouring bytes), group g of YUV_ROWS
// chroma rows, frame l.  LEFT: the chroma rows above and below (clamped) are carried down the group in registers, so a group reads
// YUV_ROWS + 2 chroma rows for YUV_ROWS; otherwise ("nearest") a row is read once.
template <bool AL, bool LEFT>
__global__ __launch_bounds__(NTH) void yuv420_to_rgb_kernel(const unsigned char* __restrict__ yuv, unsigned char* __restrict__ rgb,
                                                            int H, int W, int i420, YuvDec c, int nsx, int ngr, long long total) {
    const long long idx = (long long)blockIdx.x * NTH + threadIdx.x;
    if (idx >= total) return;
    const int sx = (int)(idx % nsx);
    const long long t = idx / nsx;
    const int g = (int)(t % ngr);
    const long long l = t / ngr;
    const int Hc = H >> 1, Wc = W >> 1;
    const unsigned char* fy = yuv + l * 3LL * Hc * W;
    const unsigned char* fc = fy + (long long)H * W;
    unsigned char* fo = rgb + l * 3LL * H * W;
    const int x0 = sx * YUV_PX, i0 = sx * (YUV_PX / 2);
    const int n = min(YUV_PX, W - x0);
    const int j0 = g * YUV_ROWS, j1 = min(j0 + YUV_ROWS, Hc);
    int up[2][5], cur[2][5], dn[2][5];
    if constexpr (LEFT) {
        load_chroma<AL>(fc, i420, Hc, Wc, max(j0 - 1, 0), i0, up);
        load_chroma<AL>(fc, i420, Hc, Wc, j0, i0, cur);
    }
    for (int j = j0; j < j1; ++j) {
        if constexpr (LEFT) load_chroma<AL>(fc, i420, Hc, Wc, min(j + 1, Hc - 1), i0, dn);
        else load_chroma<AL>(fc, i420, Hc, Wc, j, i0, cur);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long long row = (long long)(2 * j + r) * W + x0;
            int Y[YUV_PX], out[3 * YUV_PX];
            load_bytes<AL, YUV_PX>(fy + row, n, Y);
#pragma unroll
            for (int k = 0; k < YUV_PX; ++k) {
                const int i = k >> 1;
                int uv[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    if constexpr (LEFT) {
                        // horizontal taps {i: 2} at even and {i: 1, i + 1: 1} at odd pixels; vertical {j - 1: 1, j: 3} / {j: 3, j + 1: 1}
                        const int hc = (k & 1) ? cur[p][i] + cur[p][i + 1] : 2 * cur[p][i];
                        const int ho = r ? ((k & 1) ? dn[p][i] + dn[p][i + 1] : 2 * dn[p][i])
                                         : ((k & 1) ? up[p][i] + up[p][i + 1] : 2 * up[p][i]);
                        uv[p] = (3 * hc + ho + 4) >> 3;
                    } else {
                        uv[p] = cur[p][i];
                    }
                }
                const int yy = c.cy * (Y[k] - c.yo), u = uv[0] - 128, v = uv[1] - 128;
                out[3 * k] = clip255((yy + c.crv * v + 8192) >> 14);
                out[3 * k + 1] = clip255((yy - c.cgu * u - c.cgv * v + 8192) >> 14);
                out[3 * k + 2] = clip255((yy + c.cbu * u + 8192) >> 14);
            }
            store_bytes<AL, 3 * YUV_PX>(fo + 3 * row, 3 * n, out);
        }
        if constexpr (LEFT) {
#pragma unroll
            for (int p = 0; p < 2; ++p)
#pragma unroll
                for (int k = 0; k < 5; ++k) { up[p][k] = cur[p][k]; cur[p][k] = dn[p][k]; }
        }
    }
}

// RGB -> YUV, one 2 x YUV_PX strip per thread: strip column sx (fastest), chroma row j, frame l.  PASTE: a pixel whose three bytes
// equal like_rgb's keeps like's luma byte, a block of four such pixels keeps like's chroma pair; every output byte is written once.
template <bool AL, bool PASTE>
__global__ __launch_bounds__(NTH) void rgb_to_yuv420_kernel(const unsigned char* __restrict__ rgb, const unsigned char* __restrict__ like_rgb,
                                                            const unsigned char* __restrict__ like, unsigned char* __restrict__ yuv,
                                                            int H, int W, int i420, YuvEnc c, int nsx, long long total) {
    const long long idx = (long long)blockIdx.x * NTH + threadIdx.x;
    if (idx >= total) return;
    const int sx = (int)(idx % nsx);
    const long long t = idx / nsx;
    const int Hc = H >> 1, Wc = W >> 1;
    const int j = (int)(t % Hc);
    const long long l = t / Hc;
    const long long fyuv = l * 3LL * Hc * W, frgb = l * 3LL * H * W;
    const int x0 = sx * YUV_PX, i0 = sx * (YUV_PX / 2);
    const int n = min(YUV_PX, W - x0);
    int sr[4] = {0, 0, 0, 0}, sg[4] = {0, 0, 0, 0}, sb[4] = {0, 0, 0, 0}, keep[4] = {1, 1, 1, 1};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const long long row = (long long)(2 * j + r) * W + x0;
        int p[3 * YUV_PX], Y[YUV_PX];
        load_bytes<AL, 3 * YUV_PX>(rgb + frgb + 3 * row, 3 * n, p);
#pragma unroll
        for (int k = 0; k < YUV_PX; ++k) {
            const int R = p[3 * k], G = p[3 * k + 1], B = p[3 * k + 2];
            sr[k >> 1] += R; sg[k >> 1] += G; sb[k >> 1] += B;
            Y[k] = clip255(c.yo + ((c.yr * R + c.yg * G + c.yb * B + 8192) >> 14));
        }
        if constexpr (PASTE) {
            int q[3 * YUV_PX], ly[YUV_PX];
            load_bytes<AL, 3 * YUV_PX>(like_rgb + frgb + 3 * row, 3 * n, q);
            load_bytes<AL, YUV_PX>(like + fyuv + row, n, ly);
#pragma unroll
            for (int k = 0; k < YUV_PX; ++k) {
                const int same = (p[3 * k] == q[3 * k]) & (p[3 * k + 1] == q[3 * k + 1]) & (p[3 * k + 2] == q[3 * k + 2]);
                keep[k >> 1] &= same;
                Y[k] = same ? ly[k] : Y[k];
            }
        }
        store_bytes<AL, YUV_PX>(yuv + fyuv + row, n, Y);
    }
    int U[4], V[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        U[k] = clip255(128 + ((c.ur * sr[k] + c.ug * sg[k] + c.ub * sb[k] + 32768) >> 16));
        V[k] = clip255(128 + ((c.vr * sr[k] + c.vg * sg[k] + c.vb * sb[k] + 32768) >> 16));
    }
    const long long fc = fyuv + (long long)H * W;
    if constexpr (PASTE) {
        int lc[2][5];
        load_chroma<AL>(like + fc, i420, Hc, Wc, j, i0, lc);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            U[k] = keep[k] ? lc[0][k] : U[k];
            V[k] = keep[k] ? lc[1][k] : V[k];
        }
    }
    store_chroma<AL>(yuv + fc, i420, Hc, Wc, j, i0, n >> 1, U, V);
}

// the checks both entries share; 1 = nothing to do, 0 = launch, else the error code
int yuv_geometry(const char* what, int32_t L, int32_t H, int32_t W, int32_t layout) {
    E2_REQUIRE(L >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "%s: negative size %d x %d x %d", what, L, H, W);
    E2_REQUIRE((H & 1) == 0 && (W & 1) == 0, E2FGVI_EINVAL, "%s: 4:2:0 frames need even H and W, got %d x %d", what, H, W);
    E2_REQUIRE(layout == E2FGVI_YUV_NV12 || layout == E2FGVI_YUV_I420, E2FGVI_EINVAL,
               "%s: layout must be E2FGVI_YUV_NV12 (0) or E2FGVI_YUV_I420 (1), got %d", what, layout);
    if ((int64_t)L * H * W == 0) return 1;
    E2_REQUIRE((int64_t)H * W < (1LL << 31), E2FGVI_EINVAL, "%s: frames must have H * W < 2^31, got %d x %d", what, H, W);
    return 0;
}

inline bool yuv_wide(int32_t W, const void* a, const void* b, const void* c2 = nullptr, const void* d = nullptr) {
    return W % YUV_PX == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c2 | (uintptr_t)d) & 7) == 0;
}

}  // namespace

extern "C" int e2fgvi_yuv420_to_rgb(const uint8_t* yuv, uint8_t* rgb, int32_t L, int32_t H, int32_t W, int32_t layout, int32_t chroma,
                                    const int32_t* coef, void* stream) {
    const int g = yuv_geometry("yuv420_to_rgb", L, H, W, layout);
    if (g < 0) return g;
    E2_REQUIRE(chroma == E2FGVI_CHROMA_LEFT || chroma == E2FGVI_CHROMA_NEAREST, E2FGVI_EINVAL,
               "yuv420_to_rgb: chroma must be E2FGVI_CHROMA_LEFT (0) or E2FGVI_CHROMA_NEAREST (1), got %d", chroma);
    if (g == 1) return 0;
    E2_REQUIRE(yuv && rgb && coef, E2FGVI_EINVAL, "yuv420_to_rgb: null pointer");
    const YuvDec c = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
    const int nsx = (W + YUV_PX - 1) / YUV_PX, ngr = (H / 2 + YUV_ROWS - 1) / YUV_ROWS;
    const long long total = (long long)L * ngr * nsx, blocks = (total + NTH - 1) / NTH;
    E2_REQUIRE(blocks < (1LL << 24), E2FGVI_EINVAL, "yuv420_to_rgb: %d frames of %d x %d are too many for one launch", L, H, W);   // < 2^32 threads
    const dim3 grid((unsigned)blocks), block(NTH);
    hipStream_t st = (hipStream_t)stream;
    const int i420 = layout == E2FGVI_YUV_I420;
    const bool wide = yuv_wide(W, yuv, rgb), left = chroma == E2FGVI_CHROMA_LEFT;
    if (wide && left) hipLaunchKernelGGL((yuv420_to_rgb_kernel<true, true>), grid, block, 0, st, yuv, rgb, H, W, i420, c, nsx, ngr, total);
    else if (wide) hipLaunchKernelGGL((yuv420_to_rgb_kernel<true, false>), grid, block, 0, st, yuv, rgb, H, W, i420, c, nsx, ngr, total);
    else if (left) hipLaunchKernelGGL((yuv420_to_rgb_kernel<false, true>), grid, block, 0, st, yuv, rgb, H, W, i420, c, nsx, ngr, total);
    else hipLaunchKernelGGL((yuv420_to_rgb_kernel<false, false>), grid, block, 0, st, yuv, rgb, H, W, i420, c, nsx, ngr, total);
    E2_LAUNCH_CHECK("yuv420_to_rgb");
    return 0;
}

extern "C" int e2fgvi_rgb_to_yuv420(const uint8_t* rgb, const uint8_t* like_rgb, const uint8_t* like, uint8_t* yuv, int32_t L, int32_t H,
                                    int32_t W, int32_t layout, const int32_t* coef, void* stream) {
    const int g = yuv_geometry("rgb_to_yuv420", L, H, W, layout);
    if (g < 0) return g;
    E2_REQUIRE((like == nullptr) == (like_rgb == nullptr), E2FGVI_EINVAL,
               "rgb_to_yuv420: like and like_rgb come together (both NULL: the plain encode)");
    if (g == 1) return 0;
    E2_REQUIRE(rgb && yuv && coef, E2FGVI_EINVAL, "rgb_to_yuv420: null pointer");
    const YuvEnc c = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]};
    const int nsx = (W + YUV_PX - 1) / YUV_PX;
    const long long total = (long long)L * (H / 2) * nsx, blocks = (total + NTH - 1) / NTH;
    E2_REQUIRE(blocks < (1LL << 24), E2FGVI_EINVAL, "rgb_to_yuv420: %d frames of %d x %d are too many for one launch", L, H, W);   // < 2^32 threads
    const dim3 grid((unsigned)blocks), block(NTH);
    hipStream_t st = (hipStream_t)stream;
    const int i420 = layout == E2FGVI_YUV_I420;
    const bool wide = yuv_wide(W, rgb, yuv, like, like_rgb);
    if (like) {
        if (wide) hipLaunchKernelGGL((rgb_to_yuv420_kernel<true, true>), grid, block, 0, st, rgb, like_rgb, like, yuv, H, W, i420, c, nsx, total);
        else hipLaunchKernelGGL((rgb_to_yuv420_kernel<false, true>), grid, block, 0, st, rgb, like_rgb, like, yuv, H, W, i420, c, nsx, total);
    } else {
        if (wide) hipLaunchKernelGGL((rgb_to_yuv420_kernel<true, false>), grid, block, 0, st, rgb, like_rgb, like, yuv, H, W, i420, c, nsx, total);
        else hipLaunchKernelGGL((rgb_to_yuv420_kernel<false, false>), grid, block, 0, st, rgb, like_rgb, like, yuv, H, W, i420, c, nsx, total);
    }
    E2_LAUNCH_CHECK("rgb_to_yuv420");
    return 0;
}
