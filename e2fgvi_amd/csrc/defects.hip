// Dust and dirt (video.detect_defects, inpaint_video(masks_u8="defects")): a motion-compensated temporal spike test in envelope form,
// pure integers after one floor.  include/e2fgvi_hip.h has the definition; tests/defect_cases.py restates it in numpy, byte for byte.
//   frames uint8 [L][H][W][3];  fwd, bwd [L-1][H][W][2] fp32 in warp_error's convention;  ids int32 [n]: the centre frames to do
// Centre frame t, 1 <= t <= L-2, neighbour A = frame t-1 reached with g = bwd[t-1], neighbour B = frame t+1 reached with g = fwd[t],
// both flows on frame t's grid.  Y = (77 R + 150 G + 29 B + 128) >> 8 (the scene detector's luma), formed from the RGB bytes where
// they are gathered: no luma plane is made (DESIGN.md 3p has the account of the other form).  Per neighbour and pixel p = (x, y):
//   q = (x + g_x(p), y + g_y(p)) in fp64;  inside = g(p) finite, 0 <= q_x <= W-1 and 0 <= q_y <= H-1, decided in floating point
//       before any conversion to an integer;  (x0, y0) = floor(q);
//   lo, hi = min, max of Y over the pixels (x0 + i, y0 + j), -slack <= i, j <= 1 + slack, coordinates clamped to the frame
//       (clamping repeats pixels of the envelope, which changes neither the min nor the max).
//   cand(p) = inside_A and inside_B and ((Y_t > hi_A + tau and Y_t > hi_B + tau) or (Y_t < lo_A - tau and Y_t < lo_B - tau)).
// B is gathered only for the pixels that A left standing (outside A's envelope by more than tau): few, and the result is the same.
// A thread owns four consecutive pixels of a row and stores them as one dword when the address allows, bytes otherwise (W % 4 != 0,
// rows that are not dword-aligned).  The job is the grid's y axis; an id outside [1, L-2] writes nothing.
//
// The cleaning pass: n3 = the number of candidates in the 3 x 3 box around p (clipped at the frame, p included), K = cand and
// n3 >= support, D = K dilated by the (2 radius + 1)-pixel box clipped at the frame, out = 255 D, counts[t] = sum D.  One launch:
// a workgroup owns a DF_TW x DF_TH tile of one frame, stages cand of the tile and its (radius + 1)-pixel halo in LDS (outside the
// frame: 0) -- a patch without a candidate is a tile of zeros and ends there --, forms K over the tile and its radius-pixel halo, ORs
// 2 radius + 1 neighbours along the rows, then along the columns
// (csrc/video.hip overlay_edges_kernel is the precedent); a wave counts its set pixels with a ballot and adds them once.  Integer
// atomics: the counts are exact and the same in every run.
#include "frame_bytes.h"

namespace {

constexpr int DF_NTH = 256;
constexpr int DF_PX = 4;              // pixels per thread of the candidate kernel
constexpr int DF_TW = 64, DF_TH = 32; // the clean kernel's tile
constexpr int DF_PER = DF_TH / (DF_NTH / 64);
constexpr int DF_RMAX = 16;           // largest dilation radius the LDS tiles hold
constexpr int DF_SLACK_MAX = 2;
// Bytes per pixel of `frames`.  3: the product, RGB.  1: the A/B build of tools/defects_bench.py (build.build_variant("luma",
// "-DE2_DEFECT_BPP=1")), which takes a ready-made luma plane [L][H][W] in the place of the frames -- what a luma-plane form of this
// kernel would gather (DESIGN.md 3p has the measurement).
#ifndef E2_DEFECT_BPP
#define E2_DEFECT_BPP 3
#endif
constexpr int DF_BPP = E2_DEFECT_BPP;

__device__ __forceinline__ int df_luma(const uint8_t* p) {
    if constexpr (DF_BPP == 1) return (int)p[0];
    else return fb_luma(p[0], p[1], p[2]);
}

// min / max of a neighbour's luma over the envelope of p's sample position; false: the position is outside (or the flow not finite)
template <int SLACK>
__device__ __forceinline__ bool df_envelope(const uint8_t* F, const float* __restrict__ g, long long p, int x, int y, int H, int W,
                                            int& lo, int& hi) {
    const float2 gv = *reinterpret_cast<const float2*>(g + p * 2);
    const double gx = (double)gv.x, gy = (double)gv.y;
    const double qx = (double)x + gx, qy = (double)y + gy;
    // comparisons with a NaN are false and x + inf is inf: a non-finite g is outside either way; the test says so itself
    const bool inside = isfinite(gx) && isfinite(gy) && qx >= 0.0 && qx <= (double)(W - 1) && qy >= 0.0 && qy <= (double)(H - 1);
    if (!inside) return false;
    // 0 <= q <= size - 1 holds here, so the conversions are in range and every clamped coordinate below is in the frame
    const int x0 = (int)floor(qx), y0 = (int)floor(qy);
    int l = 255, h = 0;
#pragma unroll
    for (int j = -SLACK; j <= 1 + SLACK; ++j) {
        const int yy = min(max(y0 + j, 0), H - 1);
        const uint8_t* row = F + (long long)yy * W * DF_BPP;
#pragma unroll
        for (int i = -SLACK; i <= 1 + SLACK; ++i) {
            const int xx = min(max(x0 + i, 0), W - 1);
            const int v = df_luma(row + (long long)xx * DF_BPP);
            l = min(l, v);
            h = max(h, v);
        }
    }
    lo = l;
    hi = h;
    return true;
}

template <int SLACK>
__device__ __forceinline__ unsigned df_pixel(const uint8_t* Fc, const uint8_t* FA, const uint8_t* FB, const float* __restrict__ gA,
                                             const float* __restrict__ gB, int x, int y, int H, int W, int tau) {
    const long long p = (long long)y * W + x;
    const int yc = df_luma(Fc + p * DF_BPP);
    int lo, hi;
    if (!df_envelope<SLACK>(FA, gA, p, x, y, H, W, lo, hi)) return 0u;
    const bool bright = yc > hi + tau, dark = yc < lo - tau;        // never both: lo <= hi and tau >= 0
    if (!bright && !dark) return 0u;
    if (!df_envelope<SLACK>(FB, gB, p, x, y, H, W, lo, hi)) return 0u;
    return (bright ? yc > hi + tau : yc < lo - tau) ? 1u : 0u;
}

template <int SLACK>
__global__ void __launch_bounds__(DF_NTH)
defect_candidates_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ fwd, const float* __restrict__ bwd,
                         const int* __restrict__ ids, int L, int H, int W, int wq, int tau, uint8_t* __restrict__ cand) {
    const int t = ids[blockIdx.y];
    if (t < 1 || t > L - 2) return;                                     // a table entry without both neighbours: nothing is written
    const long long idx = (long long)blockIdx.x * DF_NTH + threadIdx.x;  // (y, four-pixel group)
    if (idx >= (long long)H * wq) return;
    const int y = (int)(idx / wq), xb = (int)(idx % wq) * DF_PX;
    const long long HW = (long long)H * W;
    const uint8_t* Fc = frames + (long long)t * HW * DF_BPP;
    const uint8_t* FA = Fc - HW * DF_BPP;
    const uint8_t* FB = Fc + HW * DF_BPP;
    const float* gA = bwd + (long long)(t - 1) * HW * 2;                // t -> t-1 on t's grid
    const float* gB = fwd + (long long)t * HW * 2;                      // t -> t+1 on t's grid
    uint8_t* D = cand + (long long)t * HW + (long long)y * W + xb;
    const int nx = W - xb < DF_PX ? W - xb : DF_PX;
    unsigned bits[DF_PX];
#pragma unroll
    for (int j = 0; j < DF_PX; ++j) bits[j] = j < nx ? df_pixel<SLACK>(Fc, FA, FB, gA, gB, xb + j, y, H, W, tau) : 0u;
    if (nx == DF_PX && ((uintptr_t)D & 3) == 0) {
        *reinterpret_cast<unsigned*>(D) = bits[0] | (bits[1] << 8) | (bits[2] << 16) | (bits[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < DF_PX; ++j)
            if (j < nx) D[j] = (uint8_t)bits[j];
    }
}

__global__ void __launch_bounds__(DF_NTH)
defect_clean_kernel(const uint8_t* __restrict__ cand, const int* __restrict__ ids, int L, int H, int W, int support, int radius,
                    int ntx, uint8_t* __restrict__ out, int* __restrict__ counts) {
    __shared__ uint8_t s_c[DF_TH + 2 * DF_RMAX + 2][DF_TW + 2 * DF_RMAX + 4];   // candidates, halo radius + 1
    __shared__ uint8_t s_k[DF_TH + 2 * DF_RMAX][DF_TW + 2 * DF_RMAX];           // supported candidates, halo radius
    __shared__ uint8_t s_h[DF_TH + 2 * DF_RMAX][DF_TW];                         // ORed along the rows
    const int t = ids[blockIdx.y];
    if (t < 1 || t > L - 2) return;                     // the whole workgroup leaves, in front of the first barrier
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int x0 = tx * DF_TW, y0 = ty * DF_TH;
    const int kh = DF_TH + 2 * radius, kw = DF_TW + 2 * radius, win = 2 * radius + 1;
    const long long HW = (long long)H * W;
    const uint8_t* C = cand + (long long)t * HW;
    // the staging loop over the flat index of the (kh + 2) x (kw + 2) patch, four loads of a thread in flight at a time (a loop
    // over rows and columns waits for every byte before it asks for the next: 18 round trips at radius 1 where this makes 3)
    const int cw = kw + 2, npatch = (kh + 2) * cw;
    unsigned seen = 0;
    for (int i0 = threadIdx.x; i0 < npatch; i0 += 4 * DF_NTH) {
        uint8_t e[4];
        int at[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + k * DF_NTH;
            const int r = i / cw, c = i - r * cw;
            const int y = y0 - radius - 1 + r, x = x0 - radius - 1 + c;
            at[k] = i < npatch ? r * (int)sizeof(s_c[0]) + c : -1;
            e[k] = 0;
            if (i < npatch && y >= 0 && y < H && x >= 0 && x < W) e[k] = C[(long long)y * W + x] != 0;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (at[k] >= 0) (&s_c[0][0])[at[k]] = e[k];
            seen |= e[k];
        }
    }
    // most tiles of most videos hold no candidate, nor does their halo: zeros, and nothing to count (the same for every thread of
    // the workgroup, so all of them leave here or none does)
    if (!__syncthreads_or((int)seen)) {
        for (int i = 0; i < DF_PER; ++i) {
            const int ly = wave * DF_PER + i;
            if (y0 + ly < H && x0 + lane < W) out[(long long)t * HW + (long long)(y0 + ly) * W + x0 + lane] = 0;
        }
        return;
    }
    for (int r = wave; r < kh; r += DF_NTH / 64) {
        for (int c = lane; c < kw; c += 64) {
            int n = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) n += s_c[r + j][c] + s_c[r + j][c + 1] + s_c[r + j][c + 2];
            s_k[r][c] = s_c[r + 1][c + 1] && n >= support;
        }
    }
    __syncthreads();
    for (int r = wave; r < kh; r += DF_NTH / 64) {
        unsigned v = 0;
        for (int k = 0; k < win; ++k) v |= s_k[r][lane + k];
        s_h[r][lane] = (uint8_t)v;
    }
    __syncthreads();
    int n = 0;
    for (int i = 0; i < DF_PER; ++i) {
        const int ly = wave * DF_PER + i;
        unsigned v = 0;
        for (int k = 0; k < win; ++k) v |= s_h[ly + k][lane];
        const bool in = y0 + ly < H && x0 + lane < W;
        if (in) out[(long long)t * HW + (long long)(y0 + ly) * W + x0 + lane] = v ? 255 : 0;
        n += __popcll(__ballot(in && v));
    }
    if (lane == 0 && n) atomicAdd(counts + t, n);
}

// (the unit's own: its message names the jobs, and it takes frames of up to 2^31 - 256 pixels where fb_check_sizes stops at 2^26)
int df_check_sizes(const char* who, int32_t n, int32_t L, int32_t H, int32_t W) {
    E2_REQUIRE(n >= 0 && L >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "%s: negative size (n = %d, L = %d, H = %d, W = %d)", who, n, L, H, W);
    E2_REQUIRE(n == 0 || L >= 3, E2FGVI_EINVAL, "%s: a centre frame needs both neighbours: L >= 3, got %d", who, L);
    E2_REQUIRE((int64_t)H * W < 2147483647LL - 256, E2FGVI_EINVAL, "%s: needs H * W < 2^31 - 256, got %d x %d", who, H, W);
    return 0;
}

}  // namespace

extern "C" int e2fgvi_defect_candidates(const uint8_t* frames, const float* fwd, const float* bwd, const int32_t* ids, int32_t n,
                                        int32_t L, int32_t H, int32_t W, int32_t tau, int32_t slack, uint8_t* cand, void* stream) {
    if (int rc = df_check_sizes("defect_candidates", n, L, H, W)) return rc;
    E2_REQUIRE(tau >= 0 && tau <= 254, E2FGVI_EINVAL, "defect_candidates: tau must be in [0, 254], got %d", tau);
    E2_REQUIRE(slack >= 0 && slack <= DF_SLACK_MAX, E2FGVI_EINVAL, "defect_candidates: slack must be in [0, %d], got %d", DF_SLACK_MAX, slack);
    if (n == 0 || (int64_t)H * W == 0) return 0;        // no work: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && fwd && bwd && ids && cand, E2FGVI_EINVAL, "defect_candidates: null pointer");
    E2_REQUIRE(((uintptr_t)fwd & 7) == 0 && ((uintptr_t)bwd & 7) == 0 && ((uintptr_t)ids & 3) == 0, E2FGVI_EINVAL,
               "defect_candidates: fwd and bwd must be 8-byte aligned, ids 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int wq = (W + DF_PX - 1) / DF_PX;
    const unsigned nblk = (unsigned)(((long long)H * wq + DF_NTH - 1) / DF_NTH);
    auto kernel = slack == 0 ? defect_candidates_kernel<0> : slack == 1 ? defect_candidates_kernel<1> : defect_candidates_kernel<2>;
    return fb_slabs("defect_candidates", n, [&](int j0, unsigned nj) {          // slabs of jobs: the centre frames ids[j0 ...]
        hipLaunchKernelGGL(kernel, dim3(nblk, nj), dim3(DF_NTH), 0, st, frames, fwd, bwd, ids + j0, L, H, W, wq, tau, cand);
    });
}

extern "C" int e2fgvi_defect_clean(const uint8_t* cand, const int32_t* ids, int32_t n, int32_t L, int32_t H, int32_t W, int32_t support,
                                   int32_t radius, uint8_t* out, int32_t* counts, void* stream) {
    if (int rc = df_check_sizes("defect_clean", n, L, H, W)) return rc;
    E2_REQUIRE(support >= 1 && support <= 9, E2FGVI_EINVAL, "defect_clean: support must be in [1, 9], got %d", support);
    E2_REQUIRE(radius >= 0 && radius <= DF_RMAX, E2FGVI_EINVAL, "defect_clean: radius must be in [0, %d], got %d", DF_RMAX, radius);
    if (n == 0 || (int64_t)H * W == 0) return 0;        // no work: no launch, and the pointers are not looked at
    E2_REQUIRE(cand && ids && out && counts, E2FGVI_EINVAL, "defect_clean: null pointer");
    E2_REQUIRE(((uintptr_t)ids & 3) == 0 && ((uintptr_t)counts & 3) == 0, E2FGVI_EINVAL,
               "defect_clean: ids and counts must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)L, st);
    E2_REQUIRE(e == hipSuccess, (int)e, "defect_clean: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const int ntx = (W + DF_TW - 1) / DF_TW, nty = (H + DF_TH - 1) / DF_TH;
    return fb_slabs("defect_clean", n, [&](int j0, unsigned nj) {
        hipLaunchKernelGGL(defect_clean_kernel, dim3((unsigned)((long long)ntx * nty), nj), dim3(DF_NTH), 0, st, cand, ids + j0, L, H, W,
                           support, radius, ntx, out, counts);
    });
}
