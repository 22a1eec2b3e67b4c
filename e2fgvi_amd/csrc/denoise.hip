// Temporal denoiser (video.denoise): a motion-compensated, patch-weighted mean of a pixel with the pixels its flows point at in the
// frame before and the frame after.  Integers after one floor; include/e2fgvi_hip.h has the definition, tests/denoise_cases.py
// restates it in numpy, byte for byte.
//   frames uint8 [L][H][W][3];  fwd, bwd fp32 [L-1][H][W][2] in e2fgvi_defect_candidates' convention;  scene int32 [L]
//   Y = (77 R + 150 G + 29 B + 128) >> 8 (the scene detector's luma)
//
// Two launches per slab of frames.  The luma pass writes Y of every frame once, as a plane of its own in the caller's workspace,
// with a ring of DN_PAD = 4 replicated pixels around the frame and rows of `stride` bytes, a multiple of four with four spare bytes:
//   plane[t][row][col] = Y_t(clamp(row - 4), clamp(col - 4)),  row in [0, H + 8), col in [0, stride)
// so that (a) a SAD tap costs one byte where the RGB frames cost three, (b) a tap that the definition clamps to the frame is a plain
// read -- a candidate's centre lies in the frame, so its taps go one pixel into the ring at the most -- and (c) any run of up to
// seven bytes that starts within three pixels of the frame can be fetched as two or three ALIGNED dwords without leaving its row.
// The filter pass gives a thread one pixel; a wave is 64 consecutive pixels of a row, a workgroup 64 x 4 pixels.  Per neighbour the
// thread fetches the (2 s + 3)^2 luma window around r as rows of dwords, shifts each row into place with v_alignbyte_b32, cuts the
// 2 s + 1 three-byte runs a row holds out of it once, and takes every candidate's SAD as three v_sad_u8 against the centre's three
// rows (the fourth byte is zero on both sides).  The RGB bytes of a candidate are read only when its weight is not zero.  The final
// division is a float reciprocal with one correction step either way: the dividend is below 2^22 and the divisor at most 13056,
// both exact as floats, so the estimate is off by one at the most and the correction makes it the floor.
// What binds the filter is the number of its gathered loads (50 a pixel at search 1), not its traffic and not its arithmetic
// (profiles/denoise.txt): a second workspace plane that held a pixel's R, G, B and luma as one word made a candidate
// one load where it is two and the filter 9 % faster, but the luma pass twice as slow and the workspace five times as large;
// it was taken out.
#include "frame_bytes.h"

namespace {

constexpr int DN_NTH = 256;
constexpr int DN_TX = 64;                 // pixels per tile row: a wave
constexpr int DN_TY = DN_NTH / DN_TX;     // rows per tile
constexpr int DN_PAD = 4;                 // the ring of the luma plane: >= DN_SEARCH_MAX + 1, and a multiple of four
constexpr int DN_SEARCH_MAX = 2;

// bytes in a row of the luma plane: the frame, the ring, up to a dword, and one more dword so that a third aligned dword of a
// seven-byte run stays in the row
__host__ __device__ inline long long dn_stride(int W) { return (((long long)W + 2 * DN_PAD + 3) & ~3LL) + 4; }

__device__ __forceinline__ int dn_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ void __launch_bounds__(DN_NTH)
denoise_luma_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ plane, int t0, int H, int W, int sq) {
    const int t = t0 + (int)blockIdx.y;
    const long long idx = (long long)blockIdx.x * DN_NTH + threadIdx.x;        // (row, dword) of the plane
    if (idx >= (long long)(H + 2 * DN_PAD) * sq) return;
    const int row = (int)(idx / sq), c4 = (int)(idx - (long long)row * sq);
    const int y = dn_clamp(row - DN_PAD, 0, H - 1);
    const uint8_t* src = frames + ((long long)t * H + y) * W * 3;
    unsigned v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint8_t* p = src + 3LL * dn_clamp(c4 * 4 + k - DN_PAD, 0, W - 1);
        v |= (unsigned)fb_luma(p[0], p[1], p[2]) << (8 * k);
    }
    reinterpret_cast<unsigned*>(plane + ((long long)t * (H + 2 * DN_PAD) + row) * (4LL * sq))[c4] = v;
}

// One neighbour frame's share of a pixel's sums.  cr: the centre's three patch rows, three bytes each.  PN, FN: the neighbour's luma
// plane and RGB frame.  g: the flow from the centre frame to the neighbour on the centre's grid.
template <int S>
__device__ __forceinline__ void dn_neighbour(const unsigned (&cr)[3], const uint8_t* __restrict__ PN, const uint8_t* __restrict__ FN,
                                             const float* __restrict__ g, long long p, int x, int y, int H, int W, long long stride,
                                             int m, int& wsum, int (&acc)[3]) {
    const float2 gv = *reinterpret_cast<const float2*>(g + p * 2);
    const double gx = (double)gv.x, gy = (double)gv.y;
    const double qx = (double)x + gx, qy = (double)y + gy;
    // comparisons with a NaN are false and x + inf is inf: a non-finite g is outside either way; the test says so itself
    const bool inside = isfinite(gx) && isfinite(gy) && qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
    if (!inside) return;
    // 0 <= q <= size - 1 holds here, so r = floor(q + 0.5) lies in the frame and the conversions are in range
    const int rx = (int)floor(qx + 0.5), ry = (int)floor(qy + 0.5);
    constexpr int R = 2 * S + 3, K = 2 * S + 1;
    // the window: plane rows ry - S - 1 .. ry + S + 1 and columns rx - S - 1 .. rx + S + 1, both + DN_PAD: row >= 1, column >= 1,
    // row <= H + 6 and the last byte of the dwords read is column <= W + 11 < stride (dn_stride)
    const int b0 = rx - S - 1 + DN_PAD, sh = b0 & 3;
    const uint8_t* w0 = PN + (long long)(ry - S - 1 + DN_PAD) * stride + (b0 & ~3);
    unsigned e[R][K];                                                   // e[row][k]: the three bytes of the row from column k on
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const unsigned* q = reinterpret_cast<const unsigned*>(w0 + r * stride);
        const unsigned d0 = q[0], d1 = q[1], d2 = S == 2 ? q[2] : 0u;
        const unsigned lo = __builtin_amdgcn_alignbyte(d1, d0, sh), hi = __builtin_amdgcn_alignbyte(d2, d1, sh);
#pragma unroll
        for (int k = 0; k < K; ++k)
            e[r][k] = k == 0 ? lo & 0xFFFFFFu : k == 1 ? lo >> 8 : k == 4 ? hi & 0xFFFFFFu : __builtin_amdgcn_alignbyte(hi, lo, k) & 0xFFFFFFu;
    }
    // a candidate's bytes lie at a constant distance from those of r: one 64-bit address, the rest immediate offsets and two row
    // steps; which columns and rows of candidates lie in the frame is decided once (an address off the frame is never read)
    const uint8_t* n0 = FN + ((long long)ry * W + rx) * 3;
    const long long rowb = 3LL * W;
    bool okx[K], oky[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        okx[i] = (unsigned)(rx + i - S) < (unsigned)W;
        oky[i] = (unsigned)(ry + i - S) < (unsigned)H;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const uint8_t* nr = n0 + (j - S) * rowb;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            unsigned sad = 0;
#pragma unroll
            for (int v = 0; v < 3; ++v) sad = __builtin_amdgcn_sad_u8(cr[v], e[j + v][i], sad);
            const int w = max(0, 256 - (int)((sad * (unsigned)m) >> 8));        // SAD m < 2^25
            if (w > 0 && okx[i] && oky[j]) {                                    // a candidate off the frame is dropped
                const uint8_t* n = nr + 3 * (i - S);
                wsum += w;
                acc[0] += w * (int)n[0];
                acc[1] += w * (int)n[1];
                acc[2] += w * (int)n[2];
            }
        }
    }
}

// floor(n / d) for 0 <= n < 2^24, 1 <= d < 2^24 and n / d < 2^8, rd = 1 / d to within an ulp: n rd is within 2^-13 of n / d
__device__ __forceinline__ int dn_div(int n, int d, float rd) {
    int q = (int)((float)n * rd);
    const int r = n - q * d;
    q += r >= d ? 1 : 0;
    q -= r < 0 ? 1 : 0;
    return q;
}

template <int S>
__global__ void __launch_bounds__(DN_NTH)
denoise_filter_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ plane, const float* __restrict__ fwd,
                      const float* __restrict__ bwd, const int* __restrict__ scene, uint8_t* __restrict__ out, int t0, int L, int H,
                      int W, int ntx, int m, int limit) {
    const int t = t0 + (int)blockIdx.y;
    const int by = (int)blockIdx.x / ntx, bx = (int)blockIdx.x - by * ntx;
    const int x = bx * DN_TX + ((int)threadIdx.x & (DN_TX - 1)), y = by * DN_TY + (int)threadIdx.x / DN_TX;
    if (x >= W || y >= H) return;
    const long long HW = (long long)H * W, p = (long long)y * W + x;
    const long long stride = dn_stride(W), PB = (long long)(H + 2 * DN_PAD) * stride;
    const uint8_t* Fc = frames + (long long)t * HW * 3;
    const uint8_t* c = Fc + p * 3;
    const int c0 = c[0], c1 = c[1], c2 = c[2];
    // a neighbour outside the video or in another scene contributes nothing (the same for the whole workgroup)
    const bool hasA = t > 0 && scene[t - 1] == scene[t], hasB = t + 1 < L && scene[t + 1] == scene[t];
    int wsum = 256, acc[3] = {256 * c0, 256 * c1, 256 * c2};
    if (hasA || hasB) {
        const uint8_t* Pc = plane + (long long)t * PB;
        unsigned cr[3];                                                 // the centre's patch: rows y - 1 .. y + 1, columns x - 1 .. x + 1
        const int b0 = x - 1 + DN_PAD, sh = b0 & 3;
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const unsigned* q = reinterpret_cast<const unsigned*>(Pc + (long long)(y - 1 + DN_PAD + v) * stride + (b0 & ~3));
            cr[v] = __builtin_amdgcn_alignbyte(q[1], q[0], sh) & 0xFFFFFFu;
        }
        if (hasA)                                                       // t -> t-1 on t's grid
            dn_neighbour<S>(cr, Pc - PB, Fc - HW * 3, bwd + (long long)(t - 1) * HW * 2, p, x, y, H, W, stride, m, wsum, acc);
        if (hasB)                                                       // t -> t+1 on t's grid
            dn_neighbour<S>(cr, Pc + PB, Fc + HW * 3, fwd + (long long)t * HW * 2, p, x, y, H, W, stride, m, wsum, acc);
    }
    // Wsum <= 256 + 50 * 256 = 13056 and acc + Wsum / 2 < 2^22: both exact as floats
    const float rd = __builtin_amdgcn_rcpf((float)wsum);                // v_rcp_f32, 1 ulp: the quotient is a byte, off by one at the most
    const int half = wsum >> 1;
    uint8_t* o = out + ((long long)t * HW + p) * 3;
    o[0] = (uint8_t)dn_clamp(dn_div(acc[0] + half, wsum, rd), c0 - limit, c0 + limit);    // a weighted mean of bytes is a byte
    o[1] = (uint8_t)dn_clamp(dn_div(acc[1] + half, wsum, rd), c1 - limit, c1 + limit);
    o[2] = (uint8_t)dn_clamp(dn_div(acc[2] + half, wsum, rd), c2 - limit, c2 + limit);
}

}  // namespace

extern "C" int e2fgvi_denoise(const uint8_t* frames, const float* fwd, const float* bwd, const int32_t* scene, uint8_t* out,
                              uint8_t* work, int64_t work_bytes, int32_t L, int32_t H, int32_t W, int32_t strength, int32_t search,
                              int32_t max_change, void* stream) {
    E2_REQUIRE(L >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "denoise: negative size (L = %d, H = %d, W = %d)", L, H, W);
    E2_REQUIRE((int64_t)H * W < 2147483647LL - 256, E2FGVI_EINVAL, "denoise: needs H * W < 2^31 - 256, got %d x %d", H, W);
    E2_REQUIRE(strength >= 1 && strength <= 64, E2FGVI_EINVAL, "denoise: strength must be in [1, 64], got %d", strength);
    E2_REQUIRE(search >= 0 && search <= DN_SEARCH_MAX, E2FGVI_EINVAL, "denoise: search must be in [0, %d], got %d", DN_SEARCH_MAX, search);
    E2_REQUIRE(max_change >= 0 && max_change <= 255, E2FGVI_EINVAL, "denoise: max_change must be in [0, 255], got %d", max_change);
    if (L == 0 || (int64_t)H * W == 0) return 0;        // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && scene && out, E2FGVI_EINVAL, "denoise: null pointer");
    E2_REQUIRE(((uintptr_t)scene & 3) == 0, E2FGVI_EINVAL, "denoise: scene must be 4-byte aligned");
    const uint64_t fb = 3ull * (uint64_t)H * (uint64_t)W * (uint64_t)L;
    E2_REQUIRE(fb_disjoint(frames, fb, out, fb), E2FGVI_EINVAL, "denoise: out must not overlap frames (a pixel reads three frames)");
    const long long stride = dn_stride(W);
    const int64_t need = (int64_t)L * (H + 2 * DN_PAD) * stride;
    if (L >= 2) {                                       // a single frame has no neighbour: no flows and no luma are read
        E2_REQUIRE(fwd && bwd && work, E2FGVI_EINVAL, "denoise: null pointer");
        E2_REQUIRE(((uintptr_t)fwd & 7) == 0 && ((uintptr_t)bwd & 7) == 0 && ((uintptr_t)work & 3) == 0, E2FGVI_EINVAL,
                   "denoise: fwd and bwd must be 8-byte aligned, work 4-byte aligned");
        E2_REQUIRE(work_bytes >= need, E2FGVI_EINVAL, "denoise: work must hold L (H + 8) ((W + 11) / 4 * 4 + 4) = %lld bytes, got %lld",
                   (long long)need, (long long)work_bytes);
        E2_REQUIRE(fb_disjoint(work, (uint64_t)need, out, fb) && fb_disjoint(work, (uint64_t)need, frames, fb), E2FGVI_EINVAL,
                   "denoise: work must not overlap frames or out");
    }
    hipStream_t st = (hipStream_t)stream;
    const int m = (65536 + (9 * strength) / 2) / (9 * strength);
    const int sq = (int)(stride / 4), ntx = cdiv(W, DN_TX);
    const unsigned nluma = (unsigned)cdiv64((int64_t)(H + 2 * DN_PAD) * sq, DN_NTH);
    const unsigned ntile = (unsigned)((int64_t)ntx * cdiv(H, DN_TY));                   // at most 2^31 / 4 + 2^31 / 64
    auto kernel = search == 0 ? denoise_filter_kernel<0> : search == 1 ? denoise_filter_kernel<1> : denoise_filter_kernel<2>;
    if (L >= 2) {
        const int rc = fb_slabs("denoise", L, [&](int t0, unsigned n) {
            hipLaunchKernelGGL(denoise_luma_kernel, dim3(nluma, n), dim3(DN_NTH), 0, st, frames, work, t0, H, W, sq);
        });
        if (rc) return rc;
    }
    return fb_slabs("denoise", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(kernel, dim3(ntile, n), dim3(DN_NTH), 0, st, frames, (const uint8_t*)work, fwd, bwd, scene, out, t0, L, H, W,
                           ntx, m, max_change);
    });
}
