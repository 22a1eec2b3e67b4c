// Local deflicker (video.deflicker_local): the deflicker of flicker.hip cell by cell on a grid of gy x gx cells, the cells' curves
// blended between the cell centres.  Pure integers; include/e2fgvi_hip.h has the definition, tests/flicker_local_cases.py restates
// it in numpy, word for word and byte for byte.  What is shared with flicker.hip comes from flicker_common.h.
//   frames uint8 [L][H][W][3];  cell (i, j) = rows [(i H) / gy, ((i + 1) H) / gy) x columns [(j W) / gx, ((j + 1) W) / gx)
//
// The rows of a cell row -- and of a band of the apply pass -- are one run of consecutive pixels of the frame, [lo, hi).  Both frame
// passes cut such a run into pieces of consecutive pixels, one workgroup each, that start on the frame's grid of groups of four
// pixels (the piece of the first workgroup starts at lo rounded down to a multiple of four): a group that lies in the run whole is
// three aligned dwords when the frame starts on a dword, as in flicker.hip; a group across an end of the run, the short group at
// the end of the frame and every group of a frame off a dword go pixel by pixel, each pixel by the workgroup of ITS run.  So every
// frame byte is read once.  The grid's x axis is gy runs x the pieces of the longest; a workgroup past the end of its run returns.
// The bounds of the rows and of the cell columns are computed by the entry and passed by value (they are the same for every thread).
//
// The histogram pass.  hist[t][i][j][v], int32 [L][gy][gx][256].  A workgroup stays inside one cell row, so it keeps gx histograms
// in LDS: word ((256 j + v) C + tid % C), C = 8 copies side by side for gx <= 4 and 4 for gx <= 8 (32 KB either way).  A thread
// takes FLL_HIT = 8 groups 1024 pixels apart, all dwords asked for before the first is used; the column of a group's first pixel is
// carried from group to group (1024 mod W further, modulo W), the cell column is the number of column bounds at or below it; a group
// that lies in one cell with four equal lumas is one atomic of 4.  After the barrier thread v adds the copies of bin v of every cell
// and issues one global integer atomic per non-zero bin.  The entry clears the words on the stream first.  Integer atomics: exact.
//
// The curves pass is ONE launch, a workgroup per (frame, cell): fl_curves_row with N = n_ij and a row stride of gy gx, d kept in
// 1/16 levels.
//
// The apply pass.  A band is the rows with the same i0 (the cell row above, in the blend): band b reaches from the centre of cell
// row b to that of b + 1, the first from row 0 and the last to row H - 1.  A workgroup owns FLL_APX = 8192 consecutive pixels of a
// band and stages the curves it can need in LDS: word 256 j + Y holds d16[t][i0][j][Y] in its low half and d16[t][i1][j][Y] in its
// high half (gx KB), so a pixel's four shifts are TWO LDS reads, at j0 and j1.  Per group three divisions -- the row and column of
// its first pixel, and its positions v and u (32-bit while (2 n - 1) 1024 < 2^31, 64-bit for longer sides); inside the group u is
// carried with its remainder, and a pixel that starts a new row takes its positions afresh.  The blend, one shift per pixel, added
// to its three bytes and clipped; twelve bytes go out as three dwords (or byte by byte).  Each output byte is written once, by the
// thread that read the input byte, and a thread reads all its dwords before it writes: out == frames is in order.
#include "flicker_common.h"

namespace {

constexpr int FLL_G_MAX = 8;               // cells per axis
constexpr int FLL_HIT = 8;                 // groups per thread of the histogram kernel
constexpr int FLL_HPX = FL_NTH * FB_PX * FLL_HIT;
constexpr int FLL_HWORDS = 8192;           // words of LDS of the histogram kernel: gx cells x 256 bins x C copies
constexpr int FLL_AIT = 8;                 // groups per thread of the apply kernel
constexpr int FLL_APX = FL_NTH * FB_PX * FLL_AIT;
constexpr int FLL_NONE = 0x7fffffff;       // a column bound that no column reaches

struct FllRows { int at[FLL_G_MAX + 1]; };     // run i is the rows [at[i], at[i + 1])
struct FllCols { int at[FLL_G_MAX - 1]; };     // cell column j + 1 starts at column at[j]; FLL_NONE from j = gx - 1 on

// the run of workgroup blockIdx.x -> its number, and the pixels [lo, hi) of the frame it covers
__device__ __forceinline__ int fll_run(const FllRows& rows, int nchunk, int W, int& lo, int& hi, int& chunk) {
    const int i = (int)blockIdx.x / nchunk;
    chunk = (int)blockIdx.x - i * nchunk;
    int r0 = 0, r1 = 0;
#pragma unroll
    for (int m = 0; m < FLL_G_MAX; ++m)
        if (m == i) {
            r0 = rows.at[m];
            r1 = rows.at[m + 1];
        }
    lo = r0 * W;
    hi = r1 * W;
    return i;
}

__device__ __forceinline__ int fll_cell(const FllCols& cols, int x) {
    int j = 0;
#pragma unroll
    for (int m = 0; m < FLL_G_MAX - 1; ++m) j += x >= cols.at[m] ? 1 : 0;
    return j;
}

__global__ void __launch_bounds__(FL_NTH)
flicker_local_hist_kernel(const uint8_t* __restrict__ frames, int t0, int N, int W, int gy, int gx, int nchunk, FllRows rows, FllCols cols,
                          int* __restrict__ hist) {
    __shared__ int s_h[FLL_HWORDS];
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    int lo, hi, chunk;
    const int i = fll_run(rows, nchunk, W, lo, hi, chunk);
    const int first = (lo & ~(FB_PX - 1)) + chunk * FLL_HPX;      // < 2^26 + 8192
    if (first >= hi) return;                                       // the same for the whole workgroup
    const int shift = gx <= 4 ? 3 : 2, copies = 1 << shift;        // gx 256 copies <= FLL_HWORDS
    for (int k = tid; k < gx * 256 * copies; k += FL_NTH) s_h[k] = 0;
    __syncthreads();
    const uint8_t* fr = frames + (long long)t * N * 3;
    const int p0 = first + tid * FB_PX;
    int* mine = s_h + (tid & (copies - 1));
    const int step = (FL_NTH * FB_PX) % W;
    int x = p0 % W;
    // one pixel, which may lie outside the run
    auto one = [&](int p, int xx) {
        if (p < lo || p >= hi) return;
        if (xx >= W) xx = p % W;
        const uint8_t* q = fr + (long long)p * 3;
        atomicAdd(mine + ((fll_cell(cols, xx) * 256 + fb_luma(q[0], q[1], q[2])) << shift), 1);
    };
    if (((uintptr_t)fr & 3) == 0) {                                // the same for every thread of the frame: a group is 12 bytes
        unsigned w[FLL_HIT][3];
#pragma unroll
        for (int k = 0; k < FLL_HIT; ++k) {
            const int p = p0 + k * FL_NTH * FB_PX;
            w[k][0] = w[k][1] = w[k][2] = 0;
            if (p >= lo && p + FB_PX <= hi) fb_load_dwords(fr + (long long)p * 3, w[k]);       // the twelve bytes lie in the run
        }
#pragma unroll
        for (int k = 0; k < FLL_HIT; ++k) {
            const int p = p0 + k * FL_NTH * FB_PX;
            if (p >= lo && p + FB_PX <= hi) {
                int y[FB_PX];
                fb_luma4(w[k], y);
                if (x + FB_PX <= W) {                              // the group lies in one row
                    const int ja = fll_cell(cols, x), jb = fll_cell(cols, x + FB_PX - 1);
                    if (ja == jb && y[0] == y[1] && y[1] == y[2] && y[2] == y[3]) {
                        atomicAdd(mine + ((ja * 256 + y[0]) << shift), FB_PX);
                    } else {
#pragma unroll
                        for (int j = 0; j < FB_PX; ++j)
                            atomicAdd(mine + (((ja == jb ? ja : fll_cell(cols, x + j)) * 256 + y[j]) << shift), 1);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < FB_PX; ++j) atomicAdd(mine + ((fll_cell(cols, (p + j) % W) * 256 + y[j]) << shift), 1);
                }
            } else {
                for (int j = 0; j < FB_PX; ++j) one(p + j, x + j);
            }
            x += step;
            x -= x >= W ? W : 0;
        }
    } else {
        for (int k = 0; k < FLL_HIT; ++k) {
            const int p = p0 + k * FL_NTH * FB_PX;
            for (int j = 0; j < FB_PX; ++j) one(p + j, x + j);
            x += step;
            x -= x >= W ? W : 0;
        }
    }
    __syncthreads();
    for (int j = 0; j < gx; ++j) {
        int sum = 0;
        for (int c = 0; c < copies; ++c) sum += s_h[((j * 256 + tid) << shift) + ((c + tid) & (copies - 1))];
        if (sum) atomicAdd(hist + (((long long)t * gy + i) * gx + j) * 256 + tid, sum);
    }
}

__global__ void __launch_bounds__(FL_NTH)
flicker_local_curves_kernel(const int* __restrict__ hist, const int* __restrict__ scene, int L, int H, int W, int gy, int gx, int span,
                            int max_shift, int* __restrict__ Q, short* __restrict__ d16) {
    const int cells = gy * gx;
    const int t = (int)(blockIdx.x / (unsigned)cells), cell = (int)(blockIdx.x - (unsigned)t * (unsigned)cells);
    const int i = cell / gx, j = cell - i * gx;
    // H, W <= 2^26 and i, j < 8: the products stay below 2^30
    const int n = (((i + 1) * H) / gy - (i * H) / gy) * (((j + 1) * W) / gx - (j * W) / gx);
    fl_curves_row<false>(hist, scene, t, L, cells, cell, n, span, max_shift, Q, d16);
}

// q = ((2 i + 1) c) / n and the rest, c = 128 g <= 1024, i < n <= 2^26
__device__ __forceinline__ void fll_divide(int i, int c, int n, int& q, int& rest) {
    if (n <= (1 << 20)) {                                          // (2 n - 1) 1024 < 2^31
        const unsigned num = (2u * (unsigned)i + 1u) * (unsigned)c;
        q = (int)(num / (unsigned)n);
        rest = (int)(num - (unsigned)q * (unsigned)n);
    } else {
        const unsigned long long num = (2ull * (unsigned)i + 1ull) * (unsigned)c;
        q = (int)(num / (unsigned)n);
        rest = (int)(num - (unsigned long long)q * (unsigned)n);
    }
}

// the position of a quotient between the cell centres, in 1/256 of a cell
__device__ __forceinline__ int fll_pos(int q, int g) { return min(max(q - 128, 0), (g - 1) * 256); }

__global__ void __launch_bounds__(FL_NTH)
flicker_local_apply_kernel(const uint8_t* frames, const short* __restrict__ d16, int t0, int N, int H, int W, int gy, int gx, int nchunk,
                           FllRows bands, uint8_t* out) {
    __shared__ int s_d[FLL_G_MAX * 256];
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    int lo, hi, chunk;
    const int i0 = fll_run(bands, nchunk, W, lo, hi, chunk), i1 = min(i0 + 1, gy - 1);
    const int first = (lo & ~(FB_PX - 1)) + chunk * FLL_APX;
    if (first >= hi) return;                                       // the same for the whole workgroup
    for (int j = 0; j < gx; ++j) {
        const unsigned a = (unsigned short)d16[(((long long)t * gy + i0) * gx + j) * 256 + tid];
        const unsigned c = (unsigned short)d16[(((long long)t * gy + i1) * gx + j) * 256 + tid];
        s_d[j * 256 + tid] = (int)(a | (c << 16));
    }
    __syncthreads();
    const uint8_t* fr = frames + (long long)t * N * 3;
    uint8_t* fo = out + (long long)t * N * 3;
    const int p0 = first + tid * FB_PX;
    const bool aligned = (((uintptr_t)fr | (uintptr_t)fo) & 3) == 0;       // the same for every thread of the frame
    const int cx = 128 * gx, cy = 128 * gy;
    const int dq = (2 * cx) / W, dr = (2 * cx) - dq * W;           // what one column further adds to u's quotient and rest
    unsigned w[FLL_AIT][3];
    // frames and out may be the same buffer (no __restrict__): a thread reads the bytes of its groups before it writes any of them
    if (aligned) {
#pragma unroll
        for (int k = 0; k < FLL_AIT; ++k) {
            const int p = p0 + k * FL_NTH * FB_PX;
            w[k][0] = w[k][1] = w[k][2] = 0;
            if (p >= lo && p + FB_PX <= hi) fb_load_dwords(fr + (long long)p * 3, w[k]);       // the twelve bytes lie in the band
        }
    }
#pragma unroll
    for (int k = 0; k < FLL_AIT; ++k) {
        const int p = p0 + k * FL_NTH * FB_PX;
        if (p >= hi || p + FB_PX <= lo) continue;
        // the row and the column of the group's first pixel and their positions; fy is taken inside band i0
        int r = p / W, x = p - r * W, qx, rx, qy, ry;
        fll_divide(x, cx, W, qx, rx);
        fll_divide(min(r, H - 1), cy, H, qy, ry);
        int fy = fll_pos(qy, gy) - 256 * i0;
        const bool whole = aligned && p >= lo && p + FB_PX <= hi;
        int y[FB_PX], s[FB_PX];
        if (whole) fb_luma4(w[k], y);
#pragma unroll
        for (int j = 0; j < FB_PX; ++j) {
            const bool in = p + j >= lo && p + j < hi;
            if (!whole && in) {
                const uint8_t* q = fr + (long long)(p + j) * 3;
                y[j] = fb_luma(q[0], q[1], q[2]);
            }
            if (whole || in) {
                const int u = fll_pos(qx, gx), j0 = u >> 8, fx = u & 255, j1 = min(j0 + 1, gx - 1);
                const int ac = s_d[j0 * 256 + y[j]], be = s_d[j1 * 256 + y[j]];
                const int top = (int)(short)(unsigned short)ac * (256 - fx) + (int)(short)(unsigned short)be * fx;
                const int bot = (ac >> 16) * (256 - fx) + (be >> 16) * fx;
                const int D = (top * (256 - fy) + bot * fy + 32768) >> 16;
                s[j] = (D + 8) >> 4;
            }
            // one column further; at the end of the row the next row's first
            if (++x == W) {
                x = 0;
                ++r;
                fll_divide(0, cx, W, qx, rx);
                fll_divide(min(r, H - 1), cy, H, qy, ry);
                fy = fll_pos(qy, gy) - 256 * i0;
            } else {
                qx += dq;
                rx += dr;
                if (rx >= W) {
                    rx -= W;
                    ++qx;
                }
            }
        }
        if (whole) {
            unsigned b[12];
#pragma unroll
            for (int m = 0; m < 12; ++m) b[m] = fb_byte(fb_get(w[k], m) + s[m / 3]);
            unsigned* o = reinterpret_cast<unsigned*>(fo + (long long)p * 3);
#pragma unroll
            for (int m = 0; m < 3; ++m) o[m] = b[4 * m] | (b[4 * m + 1] << 8) | (b[4 * m + 2] << 16) | (b[4 * m + 3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < FB_PX; ++j) {
                if (p + j < lo || p + j >= hi) continue;
                const uint8_t* q = fr + (long long)(p + j) * 3;
                const int rr = q[0], g = q[1], bl = q[2];
                uint8_t* o = fo + (long long)(p + j) * 3;
                o[0] = (uint8_t)min(max(rr + s[j], 0), 255);
                o[1] = (uint8_t)min(max(g + s[j], 0), 255);
                o[2] = (uint8_t)min(max(bl + s[j], 0), 255);
            }
        }
    }
}

// the smallest row r of [0, n] whose quotient ((2 r + 1) 128 g) / n reaches `want` (n when none does): where band `want` starts
int fll_first(int n, int g, long long want) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (((2LL * mid + 1) * 128 * g) / n >= want) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

int fll_check(const char* who, int32_t L, int32_t H, int32_t W, int32_t gy, int32_t gx) {
    if (int rc = fb_check_sizes(who, L, H, W)) return rc;
    E2_REQUIRE(gy >= 1 && gy <= FLL_G_MAX && gx >= 1 && gx <= FLL_G_MAX, E2FGVI_EINVAL, "%s: gy and gx must be in [1, %d], got %d x %d",
               who, FLL_G_MAX, gy, gx);
    return 0;
}

// with work: every cell has a pixel
int fll_check_cells(const char* who, int32_t H, int32_t W, int32_t gy, int32_t gx) {
    E2_REQUIRE(H >= gy && W >= gx, E2FGVI_EINVAL, "%s: needs H >= gy and W >= gx, got %d x %d for a grid of %d x %d", who, H, W, gy, gx);
    return 0;
}

// the pieces of `piece` pixels that the longest run of `rows` needs, the lead-in of up to three pixels included
unsigned fll_chunks(const FllRows& rows, int g, int W, int piece) {
    long long most = 0;
    for (int i = 0; i < g; ++i) most = most > rows.at[i + 1] - rows.at[i] ? most : rows.at[i + 1] - rows.at[i];
    return (unsigned)((most * W + (FB_PX - 1) + piece - 1) / piece);
}

}  // namespace

extern "C" int e2fgvi_flicker_local_hist(const uint8_t* frames, int32_t* hist, int32_t L, int32_t H, int32_t W, int32_t gy, int32_t gx,
                                         void* stream) {
    if (int rc = fll_check("flicker_local_hist", L, H, W, gy, gx)) return rc;
    const int N = H * W;
    if (L == 0 || N == 0) return 0;                                // no pixel: no launch, and the pointers are not looked at
    if (int rc = fll_check_cells("flicker_local_hist", H, W, gy, gx)) return rc;
    E2_REQUIRE(frames && hist, E2FGVI_EINVAL, "flicker_local_hist: null pointer");
    E2_REQUIRE(((uintptr_t)hist & 3) == 0, E2FGVI_EINVAL, "flicker_local_hist: hist must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(hist, 0, sizeof(int32_t) * 256 * (size_t)gy * (size_t)gx * (size_t)L, st);
    E2_REQUIRE(e == hipSuccess, (int)e, "flicker_local_hist: hipMemsetAsync failed: %s", hipGetErrorString(e));
    FllRows rows;
    FllCols cols;
    for (int i = 0; i <= FLL_G_MAX; ++i) rows.at[i] = i <= gy ? (int)(((long long)i * H) / gy) : H;
    for (int j = 0; j < FLL_G_MAX - 1; ++j) cols.at[j] = j + 1 < gx ? (int)(((long long)(j + 1) * W) / gx) : FLL_NONE;
    const unsigned nchunk = fll_chunks(rows, gy, W, FLL_HPX);
    return fb_slabs("flicker_local_hist", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(flicker_local_hist_kernel, dim3(nchunk * (unsigned)gy, n), dim3(FL_NTH), 0, st, frames, t0, N, W, gy, gx,
                           (int)nchunk, rows, cols, hist);
    });
}

extern "C" int e2fgvi_flicker_local_curves(const int32_t* hist, const int32_t* scene, int32_t* Q, int16_t* d16, int32_t L, int32_t H,
                                           int32_t W, int32_t gy, int32_t gx, int32_t span, int32_t max_shift, void* stream) {
    if (int rc = fll_check("flicker_local_curves", L, H, W, gy, gx)) return rc;
    E2_REQUIRE(span >= 0 && span <= FL_SPAN_MAX, E2FGVI_EINVAL, "flicker_local_curves: span must be in [0, %d], got %d", FL_SPAN_MAX,
               span);
    E2_REQUIRE(max_shift >= 1 && max_shift <= FL_SHIFT_MAX, E2FGVI_EINVAL, "flicker_local_curves: max_shift must be in [1, %d], got %d",
               FL_SHIFT_MAX, max_shift);
    E2_REQUIRE((int64_t)L * gy * gx <= 0x7fffffff, E2FGVI_EINVAL, "flicker_local_curves: needs L * gy * gx < 2^31, got %d x %d x %d", L,
               gy, gx);
    if (L == 0 || (int64_t)H * W == 0) return 0;                   // no pixel: no launch, and the pointers are not looked at
    if (int rc = fll_check_cells("flicker_local_curves", H, W, gy, gx)) return rc;
    E2_REQUIRE(hist && scene && Q && d16, E2FGVI_EINVAL, "flicker_local_curves: null pointer");
    E2_REQUIRE((((uintptr_t)hist | (uintptr_t)scene | (uintptr_t)Q) & 3) == 0 && ((uintptr_t)d16 & 1) == 0, E2FGVI_EINVAL,
               "flicker_local_curves: hist, scene and Q must be 4-byte aligned, d16 2-byte aligned");
    hipLaunchKernelGGL(flicker_local_curves_kernel, dim3((unsigned)L * (unsigned)(gy * gx)), dim3(FL_NTH), 0, (hipStream_t)stream, hist,
                       scene, L, H, W, gy, gx, span, max_shift, Q, d16);
    E2_LAUNCH_CHECK("flicker_local_curves");
    return 0;
}

extern "C" int e2fgvi_flicker_local_apply(const uint8_t* frames, const int16_t* d16, uint8_t* out, int32_t L, int32_t H, int32_t W,
                                          int32_t gy, int32_t gx, void* stream) {
    if (int rc = fll_check("flicker_local_apply", L, H, W, gy, gx)) return rc;
    const int N = H * W;
    if (L == 0 || N == 0) return 0;                                // no pixel: no launch, and the pointers are not looked at
    if (int rc = fll_check_cells("flicker_local_apply", H, W, gy, gx)) return rc;
    E2_REQUIRE(frames && d16 && out, E2FGVI_EINVAL, "flicker_local_apply: null pointer");
    E2_REQUIRE(((uintptr_t)d16 & 1) == 0, E2FGVI_EINVAL, "flicker_local_apply: d16 must be 2-byte aligned");
    E2_REQUIRE(fb_same_or_disjoint(frames, out, (uint64_t)L * (uint64_t)N * 3), E2FGVI_EINVAL,
               "flicker_local_apply: out must be frames itself or not overlap it");
    // band b: the rows whose position v lies in [256 b, 256 (b + 1)), the last band to the end
    FllRows bands;
    bands.at[0] = 0;
    for (int i = 1; i <= FLL_G_MAX; ++i) bands.at[i] = i < gy ? fll_first(H, gy, 256LL * i + 128) : H;
    hipStream_t st = (hipStream_t)stream;
    const unsigned nchunk = fll_chunks(bands, gy, W, FLL_APX);
    return fb_slabs("flicker_local_apply", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(flicker_local_apply_kernel, dim3(nchunk * (unsigned)gy, n), dim3(FL_NTH), 0, st, frames, d16, t0, N, H, W, gy,
                           gx, (int)nchunk, bands, out);
    });
}
