// Inverse telecine (video.inverse_telecine, video.detect_telecine): the field-matching scores per cell of the scene detector's
// 4 x 4 grid, and the weave that puts the fields of two frames together row by row.  Pure integers; include/e2fgvi_hip.h has the
// definition, tests/telecine_cases.py restates it in numpy, word for word and byte for byte.
//   frames uint8 [L][H][W][3];  Y = (77 R + 150 G + 29 B + 128) >> 8 (the scene detector's luma)
//
// The scores pass is ONE launch per slab of frames.  M[t][q][j][cell] needs rows y - 1 and y + 1 of frame t and row y of frames
// t - 1, t and t + 1.  A thread owns a group of TC_PX = 16 pixels -- 48 bytes, three 16-byte loads a row and frame, issued at the
// byte the group starts on (the chip reads 16 bytes off their alignment; csrc/video.hip's overlay sums do the same with twelve
// bytes), so any base and any width take the same path -- and walks down a run of at most 32 rows: every row of the run is loaded
// once from each of the three frames (plus the row above the run's first and below its last one from frame t alone), its luma is
// computed once, and the luma of the last two rows stays in registers, the candidates' doubled.  A neighbour that is outside the
// video or in another scene is frame t: its rows are not loaded again, the luma of frame t is used.  Groups do not span cells:
// the columns of each cell are cut into groups of their own, the last one short (it is read as 48 bytes all the same where they
// lie inside the buffer -- they do everywhere but in the last row of the last frame, where the bytes go one by one -- and the
// luma of the pixels it does not own is zeroed), and a workgroup lies inside ONE row of cells: its four waves take four runs of
// rows of that cell row, its 64 lanes 64 consecutive groups.  So a thread adds to the six sums (q, j) of one cell: 32-bit in
// registers (32 rows of 16 pixels of at most 510), added over the lanes of each cell with shuffles, over the waves in LDS and
// into M with one 64-bit integer atomic per (q, j, cell) and workgroup (the entry clears M on the stream first): exact, the same
// in every run.
//
// The weave is ONE launch: a copy.  The bytes of an output frame are cut into pieces of 16 at the 16-byte marks of its own
// address -- a head of fewer than 16 bytes in front of the first mark, a tail behind the last -- and a thread moves four pieces,
// 256 apart: a whole piece that lies inside one row is one 16-byte load from the frame that row comes from and one aligned
// 16-byte store; a head, a tail and a piece that spans two rows go byte by byte, each byte from the frame of its own row.  Every
// byte is written once; frame ids are clamped to [0, L - 1], so no id reads outside the frames.
#include "frame_bytes.h"

namespace {

constexpr int TC_NTH = 256;
constexpr int TC_PX = 16;                 // pixels per group: 48 bytes, three 16-byte loads
constexpr int TC_WAVES = TC_NTH / 64;     // runs of rows per workgroup
constexpr int TC_ROWS = 32 * TC_WAVES;    // rows of a cell row per workgroup, at most: a run has at most 32 rows
constexpr int TC_PIECES = 4;              // 16-byte pieces per thread of the weave

struct TcGroup {                          // the 48 bytes of a group
    unsigned w[12];
};

// the group at p: three 16-byte loads at any alignment where `wide` (all 48 bytes lie inside the buffer), else its 3 n bytes one
// by one (the others read as 0)
__device__ __forceinline__ void tc_load(const uint8_t* p, int n, bool wide, TcGroup& g) {
    if (wide) {
        __builtin_memcpy(&g.w[0], p, 16);
        __builtin_memcpy(&g.w[4], p + 16, 16);
        __builtin_memcpy(&g.w[8], p + 32, 16);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) g.w[i] = 0;
#pragma unroll
        for (int i = 0; i < 3 * TC_PX; ++i)
            if (i < 3 * n) g.w[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
    }
}

// the luma of the 16 pixels of a group, four at a time from three dwords
__device__ __forceinline__ void tc_luma16(const TcGroup& g, int n, int (&y)[TC_PX]) {
#pragma unroll
    for (int k = 0; k < TC_PX / FB_PX; ++k) {
        const unsigned w[3] = {g.w[3 * k], g.w[3 * k + 1], g.w[3 * k + 2]};
        int y4[FB_PX];
        fb_luma4(w, y4);
#pragma unroll
        for (int j = 0; j < FB_PX; ++j) y[FB_PX * k + j] = y4[j];
    }
    if (n < TC_PX) {                                                    // a short group: the pixels behind it belong to another cell
#pragma unroll
        for (int i = 0; i < TC_PX; ++i)
            if (i >= n) y[i] = 0;
    }
}

__device__ __forceinline__ unsigned tc_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the first column of cell column c: the smallest x with (4 x) / W >= c
__host__ __device__ __forceinline__ int tc_cell_start(int c, int W) { return (int)(((long long)c * W + 3) >> 2); }

__global__ void __launch_bounds__(TC_NTH)
telecine_scores_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ scene, unsigned long long* __restrict__ M, int t0,
                       int L, int H, int W, int nbx, int nchunk, int per) {
    __shared__ unsigned s_sum[TC_WAVES][4][6];
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the workgroup: cell row cr, chunk of rows ch, block of 64 groups bx
    const int bid = (int)blockIdx.x;
    const int cr = bid / (nchunk * nbx), rem = bid - cr * (nchunk * nbx), ch = rem / nbx, bx = rem - ch * nbx;
    // the scored rows of the cell row: [1, 2 m] cut by (4 y) / H == cr
    const int last = 2 * ((H - 2) / 2);
    const int lo = max(tc_cell_start(cr, H), 1), hi = min(tc_cell_start(cr + 1, H) - 1, last);
    const int a = lo + (ch * TC_WAVES + wave) * per, b = min(a + per, hi + 1);      // the run [a, b): per <= 32 rows
    // the group: the g-th of the row, cells one after the other
    const int g = bx * 64 + lane;
    int cc = -1, x0 = 0, n = 0, gs = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int xs = tc_cell_start(c, W), xe = tc_cell_start(c + 1, W), ng = (xe - xs + TC_PX - 1) / TC_PX;
        if (g >= gs && g < gs + ng) {
            cc = c;
            x0 = xs + (g - gs) * TC_PX;
            n = min(TC_PX, xe - x0);
        }
        gs += ng;
    }
    const long long FB = 3LL * H * W;
    const int rowb = 3 * W;
    const bool hasP = t > 0 && scene[t - 1] == scene[t], hasN = t + 1 < L && scene[t + 1] == scene[t];      // the same for the workgroup
    const uint8_t* C = frames + t * FB + 3 * x0;
    const uint8_t* end = frames + (long long)L * FB;
    unsigned acc[2][3] = {{0, 0, 0}, {0, 0, 0}};
    if (n > 0 && a < b) {
        int c2[TC_PX], c1[TC_PX], p1[TC_PX], n1[TC_PX];                 // Y_t[r - 2], Y_t[r - 1], Y_{t-1}[r - 1], Y_{t+1}[r - 1]
        {
            TcGroup w;
            const uint8_t* p = C + (long long)(a - 1) * rowb;           // a >= 1
            tc_load(p, n, p + 3 * TC_PX <= end, w);
            tc_luma16(w, n, c1);
        }
#pragma unroll
        for (int i = 0; i < TC_PX; ++i) c2[i] = p1[i] = n1[i] = 0;
        for (int r = a; r <= b; ++r) {                                  // b <= hi + 1 <= H - 1
            TcGroup wc, wp, wn;
            int yc[TC_PX];
            const uint8_t* p = C + (long long)r * rowb;
            const bool inner = r < b;                                   // the row below the run is read from frame t alone
            tc_load(p, n, p + 3 * TC_PX <= end, wc);
            if (hasP && inner) tc_load(p - FB, n, p - FB + 3 * TC_PX <= end, wp);
            if (hasN && inner) tc_load(p + FB, n, p + FB + 3 * TC_PX <= end, wn);
            tc_luma16(wc, n, yc);
            if (r > a) {                                                // y = r - 1: rows r - 2 and r of frame t around it
                unsigned s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
                for (int i = 0; i < TC_PX; ++i) {
                    const int e = c2[i] + yc[i];
                    s0 += (unsigned)abs(2 * p1[i] - e);
                    s1 += (unsigned)abs(2 * c1[i] - e);
                    s2 += (unsigned)abs(2 * n1[i] - e);
                }
                const int q = (r - 1) & 1;
                acc[q][0] += s0;
                acc[q][1] += s1;
                acc[q][2] += s2;
            }
            if (inner) {
#pragma unroll
                for (int i = 0; i < TC_PX; ++i) {
                    c2[i] = c1[i];
                    c1[i] = p1[i] = n1[i] = yc[i];
                }
                if (hasP) tc_luma16(wp, n, p1);
                if (hasN) tc_luma16(wn, n, n1);
            }
        }
    }
    // over the lanes of each cell, over the waves, into M
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool any = __ballot(cc == c) != 0;                        // the same for the wave
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            unsigned v = 0;
            if (any) v = tc_wave_sum(cc == c ? acc[k / 3][k % 3] : 0u);
            if (lane == 0) s_sum[wave][c][k] = v;
        }
    }
    __syncthreads();
    if (tid < 24) {
        const int c = tid / 6, k = tid - 6 * c;
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < TC_WAVES; ++w) v += s_sum[w][c][k];
        if (v) atomicAdd(M + ((long long)t * 6 + k) * 16 + cr * 4 + c, v);
    }
}

__global__ void __launch_bounds__(TC_NTH)
telecine_weave_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ jobs, uint8_t* __restrict__ out, int n, int L, int H,
                      int W, int keep) {
    const long long i = (long long)blockIdx.z * FB_FRAMES_MAX + blockIdx.y;
    if (i >= n) return;
    const long long FB = 3LL * H * W;
    const int fb = (int)FB, rowb = 3 * W;                               // at most 3 * 2^26
    const int ja = min(max(jobs[2 * i], 0), L - 1), jb = min(max(jobs[2 * i + 1], 0), L - 1);
    const uint8_t* A = frames + ja * FB;                                // the rows of parity keep
    const uint8_t* B = frames + jb * FB;                                // the others
    uint8_t* D = out + i * FB;
    const int head = min((int)((16 - ((uintptr_t)D & 15)) & 15), fb);   // piece 0 is [0, head), piece k >= 1 is [head + 16 (k - 1), + 16)
    const int k0 = (int)blockIdx.x * (TC_NTH * TC_PIECES) + (int)threadIdx.x;      // a wave moves 1 KiB in a row, four times
#pragma unroll
    for (int u = 0; u < TC_PIECES; ++u) {
        const int k = k0 + u * TC_NTH;
        const int o0 = k == 0 ? 0 : min(head + 16 * (k - 1), fb);       // (k - 1 < 2^24: no overflow)
        const int o1 = k == 0 ? head : min(o0 + 16, fb);
        const int y0 = o0 / rowb;
        if (o1 - o0 == 16 && o1 <= (y0 + 1) * rowb) {
            uint4 v;
            __builtin_memcpy(&v, ((y0 & 1) == keep ? A : B) + o0, 16);
            *reinterpret_cast<uint4*>(D + o0) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {                              // a head, a tail, a piece over two rows: at most 16 bytes
                const int o = o0 + j;
                if (o < o1) D[o] = (((o / rowb) & 1) == keep ? A : B)[o];
            }
        }
    }
}

}  // namespace

extern "C" int e2fgvi_telecine_scores(const uint8_t* frames, const int32_t* scene, int64_t* M, int32_t L, int32_t H, int32_t W,
                                      void* stream) {
    if (int rc = fb_check_sizes("telecine_scores", L, H, W)) return rc;
    if (L == 0 || H == 0 || W == 0) return 0;                      // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && scene && M, E2FGVI_EINVAL, "telecine_scores: null pointer");
    E2_REQUIRE(((uintptr_t)scene & 3) == 0 && ((uintptr_t)M & 7) == 0, E2FGVI_EINVAL,
               "telecine_scores: scene must be 4-byte aligned and M 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(M, 0, sizeof(int64_t) * 96 * (size_t)L, st);
    E2_REQUIRE(e == hipSuccess, (int)e, "telecine_scores: hipMemsetAsync failed: %s", hipGetErrorString(e));
    if (H < 4) return 0;                                           // no row is scored: the zeros are the answer
    int groups = 0;
    for (int c = 0; c < 4; ++c) groups += cdiv(tc_cell_start(c + 1, W) - tc_cell_start(c, W), TC_PX);
    const int band = cdiv(H, 4);                                   // the rows of a cell row, at most
    const int nbx = cdiv(groups, 64), nchunk = cdiv(band, TC_ROWS), per = cdiv(band, nchunk * TC_WAVES);     // per <= 32
    const unsigned nblk = 4u * (unsigned)nchunk * (unsigned)nbx;   // at most 4 (2^26 / 128 + 1) (2^26 / 1024 + 2)-ish, far below 2^31
    return fb_slabs("telecine_scores", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(telecine_scores_kernel, dim3(nblk, n), dim3(TC_NTH), 0, st, frames, scene,
                           reinterpret_cast<unsigned long long*>(M), t0, L, H, W, nbx, nchunk, per);
    });
}

extern "C" int e2fgvi_field_weave(const uint8_t* frames, const int32_t* jobs, uint8_t* out, int32_t L, int32_t n, int32_t H, int32_t W,
                                  int32_t keep, void* stream) {
    if (int rc = fb_check_sizes("field_weave", L, H, W)) return rc;
    E2_REQUIRE(n >= 0, E2FGVI_EINVAL, "field_weave: negative size (n = %d)", n);
    E2_REQUIRE(keep == 0 || keep == 1, E2FGVI_EINVAL, "field_weave: keep must be 0 or 1, got %d", keep);
    if (n == 0 || H == 0 || W == 0) return 0;                      // no byte to write: no launch, and the pointers are not looked at
    E2_REQUIRE(L > 0, E2FGVI_EINVAL, "field_weave: L = 0: there is no frame to take the rows of %d jobs from", n);
    E2_REQUIRE(frames && jobs && out, E2FGVI_EINVAL, "field_weave: null pointer");
    E2_REQUIRE(((uintptr_t)jobs & 3) == 0, E2FGVI_EINVAL, "field_weave: jobs must be 4-byte aligned");
    const uint64_t fb = 3ull * (uint64_t)H * (uint64_t)W;
    E2_REQUIRE(fb_disjoint(frames, fb * (uint64_t)L, out, fb * (uint64_t)n), E2FGVI_EINVAL,
               "field_weave: out must not overlap frames (a row is read while another is written)");
    const unsigned pieces = (unsigned)(fb / 16 + 2);               // a head, the whole pieces, a tail: at most
    // one launch, the slabs of jobs on the grid's z axis (the kernel puts y and z together): no loop for fb_slabs to take over
    const dim3 grid((pieces + TC_NTH * TC_PIECES - 1) / (TC_NTH * TC_PIECES), (unsigned)(n < FB_FRAMES_MAX ? n : FB_FRAMES_MAX),
                    (unsigned)cdiv(n, FB_FRAMES_MAX));
    hipLaunchKernelGGL(telecine_weave_kernel, grid, dim3(TC_NTH), 0, (hipStream_t)stream, frames, jobs, out, n, L, H, W, keep);
    E2_LAUNCH_CHECK("field_weave");
    return 0;
}
