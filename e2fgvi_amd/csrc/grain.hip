// Film grain (video.match_grain): measure the grain of the caller's frames block by block, and lay synthetic grain of the measured
// strength over the pixels a restoration filled in.  Pure integers; include/e2fgvi_hip.h has the definition, tests/grain_cases.py
// restates it in numpy, entry for entry and byte for byte.  Between the two launches ops.grain_lut turns the block sums into the
// table the second one reads (the lower quartile per scene, luma band and channel; borrowing; clamp; isqrt), on the device.
//   frames, filled, out uint8 [L][H][W][3];  hole, where uint8 [L][H][W] (non-zero = set);  Y = (77 R + 150 G + 29 B + 128) >> 8
//
// The blocks pass.  Block (by, bx) of a frame covers y in [1 + 8 by, 9 + 8 by), x in [1 + 8 bx, 9 + 8 bx); Hb = (H - 2) / 8 block
// rows, Wb likewise, so the 10 x 10 footprint of every block lies in the frame.  energy[t][by][bx][c] = the sum over the block's 64
// pixels of r^2, r = 4 p - p(x-1) - p(x+1) - p(y-1) - p(y+1) on channel c;  band[t][by][bx] = (sum Y >> 6) >> 5, or 255 when one of
// the block's 192 bytes is 0 or 255 or a pixel of its footprint has hole != 0.  A thread owns four pixels of a row, sixteen
// consecutive lanes own a block (lane = 16 block + 2 row + half), a workgroup sixteen blocks side by side: a row of the group is 384
// consecutive bytes.  The sums are reduced with four xor-shuffles inside the sixteen lanes; the first of them writes the four
// results.  Every entry is written exactly once: no atomics, nothing to clear, the same bits in every run.
//
// The apply pass.  A thread owns four pixels.  It reads their `where` bytes (one dword when the address allows) and is done when
// none is set and out is filled itself; otherwise a pixel whose byte is set gets, per channel c,
//   h = mix(mix(seed + 0x9E3779B9 t) ^ ((y W + x) 3 + c)) in uint32,  n = the sum of h's four bytes - 510,
//   out = clamp(p + ((n lut[scene_of[t]][Y(p)][c] + 32768) >> 16), 0, 255)    (n lut + 32768 fits int32: 510 (2^22 - 1) + 2^15 < 2^31)
// and every other byte is copied.  The thread reads its twelve bytes before it writes them and touches no other pixel: in place
// (out == filled) is allowed.  A frame whose scene_of[t] is outside [0, n_scenes) is copied.
#include "frame_bytes.h"

namespace {

constexpr int GR_NTH = 256;
constexpr int GR_PX = FB_PX;             // pixels per thread, both kernels
constexpr int GR_GROUP = GR_NTH / 16;    // blocks per workgroup of the blocks kernel, side by side
constexpr int GR_SCALE_MAX = (1 << 22) - 1;

// fb_luma in signed arithmetic: with the unsigned form hipcc indexes the apply kernel's table another way (785 instructions for 788),
// a change of generated code that nobody has timed
__device__ __forceinline__ int gr_luma(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }

__device__ __forceinline__ unsigned gr_mix(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__global__ void __launch_bounds__(GR_NTH)
grain_blocks_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ hole, int t0, int H, int W, int Hb, int Wb, int ngx,
                    int* __restrict__ energy, uint8_t* __restrict__ band) {
    const int t = t0 + (int)blockIdx.y;
    const int by = (int)blockIdx.x / ngx, gx = (int)blockIdx.x - by * ngx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bx = gx * GR_GROUP + wave * 4 + (lane >> 4);
    const int row = (lane >> 1) & 7, half = lane & 1;
    // a block past the last column: its sixteen lanes compute nothing and write nothing (they still take part in the shuffles,
    // which never cross a group of sixteen)
    const bool live = bx < Wb;
    int e[3] = {0, 0, 0}, ysum = 0, bad = 0;
    if (live) {
        // 1 <= y <= H - 2 and 1 <= x0, x0 + 4 <= W - 1: by < Hb = (H - 2) / 8 and bx < Wb = (W - 2) / 8
        const int y = 1 + 8 * by + row, x0 = 1 + 8 * bx + GR_PX * half;
        const long long at = (long long)t * H * W + (long long)y * W + x0;
        const uint8_t* c = frames + at * 3;
        const uint8_t* u = c - (long long)W * 3;
        const uint8_t* d = c + (long long)W * 3;
        int m[(GR_PX + 2) * 3], a[GR_PX * 3], b[GR_PX * 3];
#pragma unroll
        for (int k = 0; k < (GR_PX + 2) * 3; ++k) m[k] = c[k - 3];
#pragma unroll
        for (int k = 0; k < GR_PX * 3; ++k) {
            a[k] = u[k];
            b[k] = d[k];
        }
#pragma unroll
        for (int j = 0; j < GR_PX; ++j) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int p = m[(j + 1) * 3 + ch];
                const int r = 4 * p - m[j * 3 + ch] - m[(j + 2) * 3 + ch] - a[j * 3 + ch] - b[j * 3 + ch];
                e[ch] += r * r;
                bad |= (p == 0 || p == 255) ? 1 : 0;
            }
            ysum += gr_luma(m[(j + 1) * 3], m[(j + 1) * 3 + 1], m[(j + 1) * 3 + 2]);
        }
        if (hole) {
            // the 10 x 10 footprint: the two halves of a row cover its ten columns (six each), the first and the last row of the
            // block also look at the row outside
            const uint8_t* h = hole + at - 1;
#pragma unroll
            for (int k = 0; k < GR_PX + 2; ++k) bad |= h[k] != 0 ? 1 : 0;
            if (row == 0) {
#pragma unroll
                for (int k = 0; k < GR_PX + 2; ++k) bad |= h[k - W] != 0 ? 1 : 0;
            }
            if (row == 7) {
#pragma unroll
                for (int k = 0; k < GR_PX + 2; ++k) bad |= h[k + W] != 0 ? 1 : 0;
            }
        }
    }
    // sum Y <= 64 * 255 < 2^16: the flags are counted above it
    int yb = ysum + (bad << 16);
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {
        e[0] += __shfl_xor(e[0], s, 64);
        e[1] += __shfl_xor(e[1], s, 64);
        e[2] += __shfl_xor(e[2], s, 64);
        yb += __shfl_xor(yb, s, 64);
    }
    if (live && (lane & 15) == 0) {
        const long long o = ((long long)t * Hb + by) * Wb + bx;
        energy[o * 3] = e[0];
        energy[o * 3 + 1] = e[1];
        energy[o * 3 + 2] = e[2];
        band[o] = (yb >> 16) ? (uint8_t)255 : (uint8_t)(((yb & 0xFFFF) >> 6) >> 5);
    }
}

__global__ void __launch_bounds__(GR_NTH)
grain_apply_kernel(const uint8_t* filled, const uint8_t* __restrict__ where, const int* __restrict__ lut,
                   const int* __restrict__ scene_of, int n_scenes, unsigned seed, int t0, int H, int W, int wq, uint8_t* out) {
    const int t = t0 + (int)blockIdx.y;
    const long long idx = (long long)blockIdx.x * GR_NTH + threadIdx.x;      // (y, four-pixel group)
    if (idx >= (long long)H * wq) return;
    const int y = (int)(idx / wq), xb = (int)(idx % wq) * GR_PX;
    const int nx = W - xb < GR_PX ? W - xb : GR_PX;
    const long long at = (long long)t * H * W + (long long)y * W + xb;
    const int s = scene_of[t];
    const uint8_t* Wh = where + at;
    unsigned wbits = 0;
    if ((unsigned)s < (unsigned)n_scenes) {
        if (nx == GR_PX && ((uintptr_t)Wh & 3) == 0) {
            wbits = *reinterpret_cast<const unsigned*>(Wh);
        } else {
#pragma unroll
            for (int j = 0; j < GR_PX; ++j)
                if (j < nx) wbits |= (unsigned)Wh[j] << (8 * j);
        }
    }
    const uint8_t* F = filled + at * 3;
    uint8_t* O = out + at * 3;
    if (!wbits && O == F) return;
    int v[GR_PX * 3];
#pragma unroll
    for (int k = 0; k < GR_PX * 3; ++k) v[k] = k < nx * 3 ? (int)F[k] : 0;
    if (wbits) {
        const int* tab = lut + (long long)s * 256 * 3;
        const unsigned frame_key = gr_mix(seed + 0x9E3779B9u * (unsigned)t);
        const unsigned pix = ((unsigned)y * (unsigned)W + (unsigned)xb) * 3u;
#pragma unroll
        for (int j = 0; j < GR_PX; ++j) {
            if (!((wbits >> (8 * j)) & 0xFFu)) continue;
            const int Y = gr_luma(v[j * 3], v[j * 3 + 1], v[j * 3 + 2]);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int g = min(max(tab[Y * 3 + ch], 0), GR_SCALE_MAX);
                const unsigned h = gr_mix(frame_key ^ (pix + (unsigned)(j * 3 + ch)));
                const int n = (int)((h & 0xFFu) + ((h >> 8) & 0xFFu) + ((h >> 16) & 0xFFu) + (h >> 24)) - 510;
                v[j * 3 + ch] = min(max(v[j * 3 + ch] + ((n * g + 32768) >> 16), 0), 255);
            }
        }
    }
    // bytes, one by one: twelve of them at an address that is a multiple of three pixels, not of four bytes
#pragma unroll
    for (int k = 0; k < GR_PX * 3; ++k)
        if (k < nx * 3) O[k] = (uint8_t)v[k];
}

// (the unit's own: it takes frames of up to 2^31 - 256 pixels where fb_check_sizes stops at 2^26)
int gr_check_sizes(const char* who, int32_t L, int32_t H, int32_t W) {
    E2_REQUIRE(L >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "%s: negative size (L = %d, H = %d, W = %d)", who, L, H, W);
    E2_REQUIRE((int64_t)H * W < 2147483647LL - 256, E2FGVI_EINVAL, "%s: needs H * W < 2^31 - 256, got %d x %d", who, H, W);
    return 0;
}

}  // namespace

extern "C" int e2fgvi_grain_blocks(const uint8_t* frames, const uint8_t* hole, int32_t L, int32_t H, int32_t W, int32_t* energy,
                                   uint8_t* band, void* stream) {
    if (int rc = gr_check_sizes("grain_blocks", L, H, W)) return rc;
    const int Hb = H >= 10 ? (H - 2) / 8 : 0, Wb = W >= 10 ? (W - 2) / 8 : 0;
    if (L == 0 || Hb == 0 || Wb == 0) return 0;         // no block: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && energy && band, E2FGVI_EINVAL, "grain_blocks: null pointer");
    E2_REQUIRE(((uintptr_t)energy & 3) == 0, E2FGVI_EINVAL, "grain_blocks: energy must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int ngx = (Wb + GR_GROUP - 1) / GR_GROUP;
    return fb_slabs("grain_blocks", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(grain_blocks_kernel, dim3((unsigned)((long long)ngx * Hb), n), dim3(GR_NTH), 0, st, frames, hole, t0, H, W, Hb,
                           Wb, ngx, energy, band);
    });
}

extern "C" int e2fgvi_grain_apply(const uint8_t* filled, const uint8_t* where, const int32_t* lut, const int32_t* scene_of,
                                  int32_t n_scenes, uint32_t seed, int32_t L, int32_t H, int32_t W, uint8_t* out, void* stream) {
    if (int rc = gr_check_sizes("grain_apply", L, H, W)) return rc;
    E2_REQUIRE(n_scenes >= 0, E2FGVI_EINVAL, "grain_apply: negative n_scenes (%d)", n_scenes);
    if (L == 0 || (int64_t)H * W == 0) return 0;        // no work: no launch, and the pointers are not looked at
    E2_REQUIRE(filled && where && scene_of && out && (lut || n_scenes == 0), E2FGVI_EINVAL, "grain_apply: null pointer");
    E2_REQUIRE(((uintptr_t)lut & 3) == 0 && ((uintptr_t)scene_of & 3) == 0, E2FGVI_EINVAL,
               "grain_apply: lut and scene_of must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int wq = (W + GR_PX - 1) / GR_PX;
    const unsigned nblk = (unsigned)(((long long)H * wq + GR_NTH - 1) / GR_NTH);
    return fb_slabs("grain_apply", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(grain_apply_kernel, dim3(nblk, n), dim3(GR_NTH), 0, st, filled, where, lut, scene_of, n_scenes, (unsigned)seed,
                           t0, H, W, wq, out);
    });
}
