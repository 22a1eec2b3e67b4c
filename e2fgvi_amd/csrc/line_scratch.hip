// Vertical line scratches (video.detect_line_scratches): a column that stands out against both its sides over most of the frame's
// height, frame after frame.  Pure integers; include/e2fgvi_hip.h has the definition, tests/line_scratch_cases.py restates it in
// numpy, entry for entry and byte for byte.
//   frames uint8 [L][H][W][3];  Y = (77 R + 150 G + 29 B + 128) >> 8 (the scene detector's luma);  nb = H / rows bands of `rows` rows
//
// The sums pass.  S[t][b][x] = the sum of Y over the rows of band b, int32 [L][nb][W].  A thread owns four pixels of a row -- three
// dwords when W % 4 == 0 and the frames are dword-aligned, twelve bytes otherwise (or fewer at the right edge) -- and walks down
// the rows of its band: every frame byte of a band is read once, the H % rows rows at the bottom are not read at all.  Sixty-four
// lanes read 768 consecutive bytes of a row.  Four sums per thread, one 16-byte store when the address allows.
//
// The columns pass works on S, 1 / rows of the pixels.  A workgroup owns LN_CW = 252 columns of one frame and walks down the bands,
// LN_CB = 4 of them per trip; thread i looks at column x0 - 2 + i.  Per band the thread forms the candidate bits of its column (bit
// 0 bright: S > the largest S of the side columns x-gap-side .. x-gap-1 and x+gap+1 .. x+gap+side plus tau rows; bit 1 dark: S <
// the smallest minus tau rows; a column with a side column outside the frame has neither) and puts them in LDS; after the one
// barrier of the trip the owners OR the bits of the columns x-drift .. x+drift (near) and keep, per polarity, the count of near
// bands, the first and the last.  The LDS rows are double-buffered: the bits of the next trip are written while a slower wave still
// reads those of this one.  The two columns on either side of the 252 are computed by the neighbouring workgroup as well, to the
// same bits; only the owner writes.
//
// The paint entry is two launches.  line_keep_kernel, one thread per frame and column: coln = col ORed over x-drift .. x+drift,
// votes = the frames u in [t-span, t+span] of the video with scene[u] == scene[t] and coln[u][x] set, avail = the number of such
// frames, keep = col[t][x] and votes >= min(persist, avail), per polarity; a wave adds its kept columns to counts[t] once (integer
// atomics: exact, the same in every run).  line_paint_kernel: a workgroup owns 256 columns of one band of one frame (the last band
// takes the H % rows rows below it along).  It stages, for its columns and `radius` more on either side, whether a kept column of
// either polarity spans the band (b0 <= b <= b1), in LDS -- a tile without one is zeros and ends there --, ORs 2 radius + 1 of them
// per pixel, and every wave writes the same dword per lane down its share of the band's rows: each mask byte is written once.
#include "frame_bytes.h"

namespace {

constexpr int LN_NTH = 256;
constexpr int LN_PX = FB_PX;              // pixels per thread of the sums and the paint kernel
constexpr int LN_ROWS_MIN = 4, LN_ROWS_MAX = 64;
constexpr int LN_GAP_MAX = 4, LN_SIDE_MAX = 8, LN_DRIFT_MAX = 2, LN_SPAN_MAX = 4;
constexpr int LN_RMAX = 16;               // largest paint radius the LDS row holds
constexpr int LN_CW = LN_NTH - 2 * LN_DRIFT_MAX;     // columns a workgroup of the columns kernel owns
constexpr int LN_CB = 4;                  // bands per trip of the columns kernel
constexpr int LN_TW = 64 * LN_PX;         // columns of a paint tile: a wave's row

__global__ void __launch_bounds__(LN_NTH)
line_sums_kernel(const uint8_t* __restrict__ frames, int t0, int H, int W, int rows, int nb, int wq, int* __restrict__ S) {
    const int t = t0 + (int)blockIdx.y;
    const long long idx = (long long)blockIdx.x * LN_NTH + threadIdx.x;       // (band, four-pixel group)
    if (idx >= (long long)nb * wq) return;
    const int b = (int)(idx / wq), xb = (int)(idx % wq) * LN_PX;
    const int nx = W - xb < LN_PX ? W - xb : LN_PX;
    const long long pitch = (long long)W * 3;
    // row b rows + r <= nb rows - 1 <= H - 1 and xb + nx <= W: every byte read lies in frame t
    const uint8_t* p = frames + ((long long)t * H * W + (long long)b * rows * W + xb) * 3;
    int s[LN_PX] = {0, 0, 0, 0};
    // decided once for the band, so that the loads of several rows are in flight together: with a pitch that is a multiple of four
    // bytes every row of the thread is dword-aligned when its first is
    if (nx == LN_PX && ((uintptr_t)p & 3) == 0 && (pitch & 3) == 0) {
#pragma unroll 4
        for (int r = 0; r < rows; ++r, p += pitch) {
            unsigned w[3];
            int y[LN_PX];
            fb_load_dwords(p, w);
            fb_luma4(w, y);
#pragma unroll
            for (int j = 0; j < LN_PX; ++j) s[j] += y[j];
        }
    } else {
        for (int r = 0; r < rows; ++r, p += pitch) {
#pragma unroll
            for (int j = 0; j < LN_PX; ++j)
                if (j < nx) s[j] += fb_luma(p[j * 3], p[j * 3 + 1], p[j * 3 + 2]);
        }
    }
    int* D = S + ((long long)t * nb + b) * W + xb;
    if (nx == LN_PX && ((uintptr_t)D & 15) == 0) {
        *reinterpret_cast<int4*>(D) = make_int4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
        for (int j = 0; j < LN_PX; ++j)
            if (j < nx) D[j] = s[j];
    }
}

__global__ void __launch_bounds__(LN_NTH)
line_columns_kernel(const int* __restrict__ S, int t0, int nb, int W, int thr, int gap, int side, int drift, int coverage,
                    uint8_t* __restrict__ cand, int* __restrict__ cnt, uint8_t* __restrict__ col, int* __restrict__ b0,
                    int* __restrict__ b1) {
    __shared__ uint8_t s_c[2][LN_CB][LN_NTH];
    const int t = t0 + (int)blockIdx.y;
    const int i = (int)threadIdx.x;
    const long long xl = (long long)blockIdx.x * LN_CW + i - LN_DRIFT_MAX;
    const int x = (int)xl;
    // every side column in the frame (which puts x itself there); nothing else is read from S
    const bool eligible = xl - gap - side >= 0 && xl + gap + side < W;
    // an owner has two threads on either side: the LDS reads below stay inside the row
    const bool owner = i >= LN_DRIFT_MAX && i < LN_NTH - LN_DRIFT_MAX && xl < W;
    int n[2] = {0, 0}, first[2] = {nb, nb}, last[2] = {-1, -1};
    // LN_CB bands per trip and barrier: their loads are in flight together (one band per trip waited for memory nb times in a row)
    for (int bb = 0, buf = 0; bb < nb; bb += LN_CB, buf ^= 1) {
        unsigned bits[LN_CB] = {0, 0, 0, 0};
        if (eligible) {
            // a trip past the last band reads the last band again (its bits are dropped below): no branch between the loads
            const int* row[LN_CB];
            int c[LN_CB], hi[LN_CB], lo[LN_CB];
#pragma unroll
            for (int k = 0; k < LN_CB; ++k) {
                row[k] = S + ((long long)t * nb + min(bb + k, nb - 1)) * W + x;
                c[k] = row[k][0];
                hi[k] = lo[k] = row[k][gap + 1];
            }
            for (int d = gap + 1; d <= gap + side; ++d) {
#pragma unroll
                for (int k = 0; k < LN_CB; ++k) {
                    const int l = row[k][-d], r = row[k][d];
                    hi[k] = max(hi[k], max(l, r));
                    lo[k] = min(lo[k], min(l, r));
                }
            }
#pragma unroll
            for (int k = 0; k < LN_CB; ++k) bits[k] = (c[k] > hi[k] + thr ? 1u : 0u) | (c[k] < lo[k] - thr ? 2u : 0u);
        }
#pragma unroll
        for (int k = 0; k < LN_CB; ++k) s_c[buf][k][i] = (uint8_t)bits[k];
        __syncthreads();
        if (owner) {
#pragma unroll
            for (int k = 0; k < LN_CB; ++k) {
                const int b = bb + k;
                if (b >= nb) break;
                cand[((long long)t * nb + b) * W + x] = (uint8_t)bits[k];
                unsigned near = 0;
                for (int j = -drift; j <= drift; ++j) near |= s_c[buf][k][i + j];
#pragma unroll
                for (int p = 0; p < 2; ++p)
                    if ((near >> p) & 1u) {
                        ++n[p];
                        first[p] = min(first[p], b);
                        last[p] = b;
                    }
            }
        }
    }
    if (owner) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const long long at = ((long long)t * 2 + p) * W + x;
            cnt[at] = n[p];
            col[at] = (long long)n[p] * 100 >= (long long)coverage * nb ? 1 : 0;
            b0[at] = first[p];
            b1[at] = last[p];
        }
    }
}

__global__ void __launch_bounds__(LN_NTH)
line_keep_kernel(const uint8_t* __restrict__ col, const int* __restrict__ scene, int t0, int L, int W, int drift, int span, int persist,
                 uint8_t* __restrict__ keep, int* __restrict__ counts) {
    const int t = t0 + (int)blockIdx.y;
    const long long xl = (long long)blockIdx.x * LN_NTH + threadIdx.x;
    int kept = 0;
    if (xl < W) {
        const int x = (int)xl;
        const int sc = scene[t];
        const int u0 = max(t - span, 0), u1 = min(t + span, L - 1);
        const int xa = max(x - drift, 0), xe = min(x + drift, W - 1);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const long long at = ((long long)t * 2 + p) * W + x;
            int k = 0;
            if (col[at]) {
                int votes = 0, avail = 0;
                for (int u = u0; u <= u1; ++u) {
                    if (scene[u] != sc) continue;
                    ++avail;
                    const uint8_t* c = col + ((long long)u * 2 + p) * W;
                    unsigned v = 0;
                    for (int xx = xa; xx <= xe; ++xx) v |= c[xx];
                    votes += v ? 1 : 0;
                }
                k = votes >= min(persist, avail) ? 1 : 0;
            }
            keep[at] = (uint8_t)k;
            kept += k;
        }
    }
    // no thread has left: the whole wave adds up, its first lane adds the sum once
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) kept += __shfl_xor(kept, s, 64);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(counts + t, kept);
}

__global__ void __launch_bounds__(LN_NTH)
line_paint_kernel(const uint8_t* __restrict__ keep, const int* __restrict__ b0, const int* __restrict__ b1, int t0, int H, int W,
                  int rows, int nb, int radius, int ntx, uint8_t* __restrict__ masks) {
    __shared__ uint8_t s_f[LN_TW + 2 * LN_RMAX];
    const int t = t0 + (int)blockIdx.y;
    const int b = (int)blockIdx.x / ntx, tx = (int)blockIdx.x - b * ntx;
    const int x0 = tx * LN_TW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned seen = 0;
    for (int i = threadIdx.x; i < LN_TW + 2 * radius; i += LN_NTH) {
        const int xx = x0 - radius + i;
        unsigned f = 0;
        if (xx >= 0 && xx < W) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const long long at = ((long long)t * 2 + p) * W + xx;
                if (keep[at] && b0[at] <= b && b <= b1[at]) f = 1;
            }
        }
        s_f[i] = (uint8_t)f;
        seen |= f;
    }
    // the same for every thread of the workgroup; without a kept column near the tile the word stays zero and LDS is not read
    unsigned word = 0;
    if (__syncthreads_or((int)seen)) {
#pragma unroll
        for (int j = 0; j < LN_PX; ++j) {
            unsigned v = 0;
            for (int k = 0; k <= 2 * radius; ++k) v |= s_f[lane * LN_PX + j + k];      // <= 255 + 2 radius
            word |= v ? 0xFFu << (8 * j) : 0u;
        }
    }
    const int xb = x0 + lane * LN_PX;
    if (xb >= W) return;
    const int nx = W - xb < LN_PX ? W - xb : LN_PX;
    const int y0 = b * rows, y1 = b == nb - 1 ? H : y0 + rows;       // the last band takes the remainder along
    for (int y = y0 + wave; y < y1; y += LN_NTH / 64) {
        uint8_t* D = masks + (long long)t * H * W + (long long)y * W + xb;
        if (nx == LN_PX && ((uintptr_t)D & 3) == 0) {
            *reinterpret_cast<unsigned*>(D) = word;
        } else {
#pragma unroll
            for (int j = 0; j < LN_PX; ++j)
                if (j < nx) D[j] = (uint8_t)(word >> (8 * j));
        }
    }
}

// (the unit's own: it takes frames of up to 2^31 - 256 pixels where fb_check_sizes stops at 2^26)
int ln_check_sizes(const char* who, int32_t L, int32_t H, int32_t W, int32_t rows) {
    E2_REQUIRE(L >= 0 && H >= 0 && W >= 0, E2FGVI_EINVAL, "%s: negative size (L = %d, H = %d, W = %d)", who, L, H, W);
    E2_REQUIRE((int64_t)H * W < 2147483647LL - 256, E2FGVI_EINVAL, "%s: needs H * W < 2^31 - 256, got %d x %d", who, H, W);
    E2_REQUIRE(rows >= LN_ROWS_MIN && rows <= LN_ROWS_MAX, E2FGVI_EINVAL, "%s: rows must be in [%d, %d], got %d", who, LN_ROWS_MIN,
               LN_ROWS_MAX, rows);
    return 0;
}

#define LN_RANGE(who, name, v, lo, hi) \
    E2_REQUIRE((v) >= (lo) && (v) <= (hi), E2FGVI_EINVAL, who ": " name " must be in [%d, %d], got %d", (int)(lo), (int)(hi), (int)(v))

}  // namespace

extern "C" int e2fgvi_line_sums(const uint8_t* frames, int32_t L, int32_t H, int32_t W, int32_t rows, int32_t* S, void* stream) {
    if (int rc = ln_check_sizes("line_sums", L, H, W, rows)) return rc;
    const int nb = H / rows;
    if (L == 0 || (int64_t)H * W == 0 || nb == 0) return 0;        // no band: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && S, E2FGVI_EINVAL, "line_sums: null pointer");
    E2_REQUIRE(((uintptr_t)S & 3) == 0, E2FGVI_EINVAL, "line_sums: S must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int wq = (W + LN_PX - 1) / LN_PX;
    const unsigned nblk = (unsigned)(((long long)nb * wq + LN_NTH - 1) / LN_NTH);
    return fb_slabs("line_sums", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(line_sums_kernel, dim3(nblk, n), dim3(LN_NTH), 0, st, frames, t0, H, W, rows, nb, wq, S);
    });
}

extern "C" int e2fgvi_line_columns(const int32_t* S, int32_t L, int32_t H, int32_t W, int32_t rows, int32_t tau, int32_t gap,
                                   int32_t side, int32_t drift, int32_t coverage, uint8_t* cand, int32_t* cnt, uint8_t* col,
                                   int32_t* b0, int32_t* b1, void* stream) {
    if (int rc = ln_check_sizes("line_columns", L, H, W, rows)) return rc;
    LN_RANGE("line_columns", "tau", tau, 0, 254);
    LN_RANGE("line_columns", "gap", gap, 0, LN_GAP_MAX);
    LN_RANGE("line_columns", "side", side, 1, LN_SIDE_MAX);
    LN_RANGE("line_columns", "drift", drift, 0, LN_DRIFT_MAX);
    LN_RANGE("line_columns", "coverage", coverage, 1, 100);
    const int nb = H / rows;
    if (L == 0 || (int64_t)H * W == 0 || nb == 0) return 0;        // no band: no launch, and the pointers are not looked at
    E2_REQUIRE(S && cand && cnt && col && b0 && b1, E2FGVI_EINVAL, "line_columns: null pointer");
    E2_REQUIRE((((uintptr_t)S | (uintptr_t)cnt | (uintptr_t)b0 | (uintptr_t)b1) & 3) == 0, E2FGVI_EINVAL,
               "line_columns: S, cnt, b0 and b1 must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned ntx = (unsigned)((W + LN_CW - 1) / LN_CW);
    return fb_slabs("line_columns", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(line_columns_kernel, dim3(ntx, n), dim3(LN_NTH), 0, st, S, t0, nb, W, tau * rows, gap, side, drift, coverage,
                           cand, cnt, col, b0, b1);
    });
}

extern "C" int e2fgvi_line_paint(const uint8_t* col, const int32_t* b0, const int32_t* b1, const int32_t* scene, int32_t L, int32_t H,
                                 int32_t W, int32_t rows, int32_t drift, int32_t span, int32_t persist, int32_t radius, uint8_t* keep,
                                 int32_t* counts, uint8_t* masks, void* stream) {
    if (int rc = ln_check_sizes("line_paint", L, H, W, rows)) return rc;
    LN_RANGE("line_paint", "drift", drift, 0, LN_DRIFT_MAX);
    LN_RANGE("line_paint", "span", span, 0, LN_SPAN_MAX);
    LN_RANGE("line_paint", "persist", persist, 1, 2 * span + 1);
    LN_RANGE("line_paint", "radius", radius, 0, LN_RMAX);
    const int nb = H / rows;
    if (L == 0 || (int64_t)H * W == 0 || nb == 0) return 0;        // no band: no launch, and the pointers are not looked at
    E2_REQUIRE(col && b0 && b1 && scene && keep && counts && masks, E2FGVI_EINVAL, "line_paint: null pointer");
    E2_REQUIRE((((uintptr_t)b0 | (uintptr_t)b1 | (uintptr_t)scene | (uintptr_t)counts) & 3) == 0, E2FGVI_EINVAL,
               "line_paint: b0, b1, scene and counts must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)L, st);
    E2_REQUIRE(e == hipSuccess, (int)e, "line_paint: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const unsigned nkx = (unsigned)((W + LN_NTH - 1) / LN_NTH);
    const int ntx = (W + LN_TW - 1) / LN_TW;
    // every slab's columns are kept before the first is painted: a frame's paint reads its own keep row alone
    const int rc = fb_slabs("line_paint", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(line_keep_kernel, dim3(nkx, n), dim3(LN_NTH), 0, st, col, scene, t0, L, W, drift, span, persist, keep, counts);
    });
    if (rc) return rc;
    return fb_slabs("line_paint", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(line_paint_kernel, dim3((unsigned)((long long)ntx * nb), n), dim3(LN_NTH), 0, st, keep, b0, b1, t0, H, W, rows,
                           nb, radius, ntx, masks);
    });
}
