// Deinterlacer (video.deinterlace, video.detect_interlace): the two fields of an interlaced frame made into two pictures -- a kept
// row is copied, a missing row is the line average of the rows around it clamped to the temporal prediction's neighbourhood -- and
// the field-order scores.  Pure integers; include/e2fgvi_hip.h has the definition, tests/interlace_cases.py restates it in numpy,
// byte for byte and word for word.
//   frames uint8 [L][H][W][3];  Y = (77 R + 150 G + 29 B + 128) >> 8 (the scene detector's luma)
//
// The fields pass is ONE launch per slab of frames.  A thread owns a group of IL_PX = 4 pixels (12 bytes; groups do not span rows:
// a row has ceil(W / 4) of them) over IL_R = 4 consecutive rows of frame t, starting on an even row, and writes those rows of BOTH
// pictures of the frame: in the picture that keeps a row's parity the 12 bytes are copied, in the other one they are interpolated,
// so P, C, N are read once for both pictures (at frame rate the thread does the one of the two that the kept picture needs).  It
// reads its window first -- rows y0 - 2 .. y0 + 5 of P, C and N, 24 groups, all asked for before the first is used -- and keeps
// the bytes and their luma in registers: 6 group loads a row where a thread per row issues 12 (a missing row reads rows up and dn
// of three frames and rows y - 2, y, y + 2 of two), which was worth 15 %: the pass is bound by its vector arithmetic, not by its loads
// (profiles/interlace.txt).  Which of P and N a row's d comes from depends on the row's parity and the field order alone, so the
// field order is a template parameter and what a row does not need is never kept.  The rows above the first and below the last
// one (up = y + 1, dn = y - 1) are picked out of the window with selects.  A workgroup is a tile of IL_TX = 64 groups by 16 rows:
// a wave reads 768 consecutive bytes of a row.  Luma is recomputed from the bytes in registers, not staged in LDS: with
// edges == 0 (the default) a pixel's decisions need column x alone, so there is nothing to share between lanes, and the kernel
// has no barrier.  With edges >= 1 (a template parameter, so the default path carries none of it) the 10 luma values x - 3 ..
// x + 6 of rows up and dn come from byte loads with clamped columns, and a pixel whose direction J is not 0 reads its two taps
// by bytes.
// A group is read as three dwords when every group of the thread's window is whole and on a dword (a frame whose width is a
// multiple of four in a buffer that starts on a dword: one test per thread, no branch between the loads); otherwise group by
// group, as dwords where one happens to be whole and on a dword, byte by byte where not -- the last group of a row whose width is no
// multiple of four, and a row that starts off a dword -- and only the bytes the row owns are touched.  Stores go the same way.
//
// The scores pass.  D[t][q] needs rows y - 1, y + 1 of frame t and row y of frame t + 1.  A workgroup owns IL_SC = 16 groups of
// columns over the WHOLE height, cut into IL_SR = 16 runs of rows, a thread per (run, group).  A thread walks down its run and
// loads every row of it once from frame t and once from frame t + 1, keeping the luma of the last two rows in registers; the two
// terms that need a row of the run above or below (y = the run's first and last row) are finished after one barrier from the
// first and last luma rows every thread leaves in LDS.  So every frame byte is read at most twice: once as frame t and once as
// frame t + 1.  The sums are 64-bit per thread, added over the wave with shuffles, over the workgroup in LDS and into D with one
// integer atomic per parity (the entry clears D on the stream first): exact, the same in every run.
#include "frame_bytes.h"

namespace {

constexpr int IL_NTH = 256;
constexpr int IL_PX = FB_PX;              // pixels per group
constexpr int IL_TX = 64;                 // groups per tile row: a wave
constexpr int IL_TY = IL_NTH / IL_TX;     // threads above each other in a tile
constexpr int IL_R = 4;                   // rows per thread of the fields kernel: a tile is IL_TY * IL_R = 16 rows
constexpr int IL_WR = IL_R + 4;           // the rows a thread reads of each frame: two above and two below its own
constexpr int IL_SC = 16;                 // groups of columns per workgroup of the scores kernel
constexpr int IL_SR = IL_NTH / IL_SC;     // runs of rows per workgroup of the scores kernel

// (a + b) >> 1 of the four bytes of two words at once
__device__ __forceinline__ unsigned il_avg4(unsigned a, unsigned b) { return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1); }

__device__ __forceinline__ int il_luma_at(const uint8_t* row, int x) { return fb_luma(row[3 * x], row[3 * x + 1], row[3 * x + 2]); }

template <bool EDGES, int FIRST>
__global__ void __launch_bounds__(IL_NTH)
interlace_fields_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ scene, uint8_t* __restrict__ out, int t0, int L,
                        int H, int W, int mode, int guard, int edges) {
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    const int G = (W + IL_PX - 1) >> 2, nbx = (G + IL_TX - 1) / IL_TX;
    const int by = (int)blockIdx.x / nbx, bx = (int)blockIdx.x - by * nbx;
    const int g = bx * IL_TX + (tid & (IL_TX - 1)), y0 = (by * IL_TY + tid / IL_TX) * IL_R;     // y0 is even: row y0 + r has parity r & 1
    if (g >= G || y0 >= H) return;
    const int x0 = g * IL_PX, n = min(IL_PX, W - x0);
    const long long FB = 3LL * H * W;                                   // the bytes of a frame: at most 3 * 2^26
    const int rowb = 3 * W, col = 3 * x0;
    // a neighbour outside the video or in another scene is frame t itself (the same for the whole workgroup)
    const uint8_t* C = frames + t * FB;
    const uint8_t* P = (t > 0 && scene[t - 1] == scene[t]) ? C - FB : C;
    const uint8_t* N = (t + 1 < L && scene[t + 1] == scene[t]) ? C + FB : C;
    // the window: rows y0 - 2 .. y0 + IL_R + 1 of the three frames, each read once; a row outside the frame is not read (and not used)
    unsigned cw[IL_WR][3], pw[IL_WR][3], nw[IL_WR][3];
    if (n == IL_PX && (rowb & 3) == 0 && ((uintptr_t)(C + col) & 3) == 0) {      // every group of the window is whole and on a dword
#pragma unroll
        for (int w = 0; w < IL_WR; ++w) {
            const int row = y0 - 2 + w;
            cw[w][0] = cw[w][1] = cw[w][2] = pw[w][0] = pw[w][1] = pw[w][2] = nw[w][0] = nw[w][1] = nw[w][2] = 0;
            if (row >= 0 && row < H) {
                fb_load_dwords(C + row * rowb + col, cw[w]);
                fb_load_dwords(P + row * rowb + col, pw[w]);
                fb_load_dwords(N + row * rowb + col, nw[w]);
            }
        }
    } else {
#pragma unroll
        for (int w = 0; w < IL_WR; ++w) {
            const int row = y0 - 2 + w;
            cw[w][0] = cw[w][1] = cw[w][2] = pw[w][0] = pw[w][1] = pw[w][2] = nw[w][0] = nw[w][1] = nw[w][2] = 0;
            if (row >= 0 && row < H) {
                fb_load(C + row * rowb + col, n, cw[w]);
                fb_load(P + row * rowb + col, n, pw[w]);
                fb_load(N + row * rowb + col, n, nw[w]);
            }
        }
    }
    int cl[IL_WR][IL_PX], pl[IL_WR][IL_PX], nl[IL_WR][IL_PX];          // (what a row does not need is never computed)
#pragma unroll
    for (int w = 0; w < IL_WR; ++w) {
        fb_luma4(cw[w], cl[w]);
        fb_luma4(pw[w], pl[w]);
        fb_luma4(nw[w], nl[w]);
    }
#pragma unroll
    for (int r = 0; r < IL_R; ++r) {
        const int y = y0 + r, w = r + 2;
        if (y >= H) break;
        const int kp = ((r & 1) == FIRST) ? 0 : 1, mp = 1 - kp;        // the picture that keeps row y, and the one that misses it
        const int off = y * rowb + col;
        if (mode == 0 || kp == mode - 1) fb_store(out + (mode == 0 ? 2LL * t + kp : (long long)t) * FB + off, n, cw[w]);
        if (!(mode == 0 || mp == mode - 1)) continue;
        uint8_t* dst = out + (mode == 0 ? 2LL * t + mp : (long long)t) * FB + off;
        // A and B are C and X in either order, and every use of them is symmetric: X = P for the first picture, N for the second
        const auto& xw = mp == 0 ? pw : nw;
        const auto& xl = mp == 0 ? pl : nl;
        unsigned dw[3], o[3];                                           // d = (A + B) >> 1 per byte
#pragma unroll
        for (int i = 0; i < 3; ++i) dw[i] = il_avg4(xw[w][i], cw[w][i]);
        if (H == 1) {                                                   // no row above or below: the temporal mean alone
            fb_store(dst, n, dw);
            continue;
        }
        const bool top = y == 0, bot = y == H - 1;                      // up = y + 1 at the top, dn = y - 1 at the bottom
        const int up = top ? y + 1 : y - 1, dn = bot ? y - 1 : y + 1;
        unsigned cu[3], cd[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            cu[i] = top ? cw[w + 1][i] : cw[w - 1][i];
            cd[i] = bot ? cw[w - 1][i] : cw[w + 1][i];
        }
        int c[IL_PX], e[IL_PX], diff[IL_PX];
#pragma unroll
        for (int i = 0; i < IL_PX; ++i) {
            c[i] = top ? cl[w + 1][i] : cl[w - 1][i];
            e[i] = bot ? cl[w - 1][i] : cl[w + 1][i];
            const int ypu = top ? pl[w + 1][i] : pl[w - 1][i], ypd = bot ? pl[w - 1][i] : pl[w + 1][i];
            const int ynu = top ? nl[w + 1][i] : nl[w - 1][i], ynd = bot ? nl[w - 1][i] : nl[w + 1][i];
            const int t1 = (abs(ypu - c[i]) + abs(ypd - e[i])) >> 1, t2 = (abs(ynu - c[i]) + abs(ynd - e[i])) >> 1;
            diff[i] = max(abs(xl[w][i] - cl[w][i]) >> 1, max(t1, t2));
        }
        if (guard && y - 2 >= 0 && y + 2 <= H - 1) {                    // skipped at the border rows, not clamped
#pragma unroll
            for (int i = 0; i < IL_PX; ++i) {
                const int dY = (xl[w][i] + cl[w][i]) >> 1, b = (xl[w - 2][i] + cl[w - 2][i]) >> 1, f = (xl[w + 2][i] + cl[w + 2][i]) >> 1;
                const int mx = max(max(dY - e[i], dY - c[i]), min(b - c[i], f - e[i]));
                const int mn = min(min(dY - e[i], dY - c[i]), max(b - c[i], f - e[i]));
                diff[i] = max(diff[i], max(mn, -mx));
            }
        }
        unsigned sp[3];                                                 // (C[up][x] + C[dn][x]) >> 1 per byte: direction 0
#pragma unroll
        for (int i = 0; i < 3; ++i) sp[i] = il_avg4(cu[i], cd[i]);
        int J[IL_PX] = {0, 0, 0, 0};
        const uint8_t* rup = C + up * rowb;
        const uint8_t* rdn = C + dn * rowb;
        if constexpr (EDGES) {
            int lu[IL_PX + 6], ld[IL_PX + 6];                           // the luma of columns x0 - 3 .. x0 + 6, clamped to the row
#pragma unroll
            for (int k = 0; k < IL_PX + 6; ++k) {
                const int xc = min(max(x0 - 3 + k, 0), W - 1);
                lu[k] = il_luma_at(rup, xc);
                ld[k] = il_luma_at(rdn, xc);
            }
#pragma unroll
            for (int i = 0; i < IL_PX; ++i) {
                // score(j) = the sum over k of |Y[up][x + k + j] - Y[dn][x + k - j]|, x = x0 + i: column x0 - 3 is index 0
                auto score = [&](int j) {
                    int s = 0;
#pragma unroll
                    for (int k = -1; k <= 1; ++k) s += abs(lu[i + 3 + k + j] - ld[i + 3 + k - j]);
                    return s;
                };
                int best = score(0) - 1;
                const int sm1 = score(-1), sm2 = score(-2), sp1 = score(1), sp2 = score(2);
                if (sm1 < best) {
                    best = sm1;
                    J[i] = -1;
                    if (edges >= 2 && sm2 < best) { best = sm2; J[i] = -2; }
                }
                if (sp1 < best) {
                    best = sp1;
                    J[i] = 1;
                    if (edges >= 2 && sp2 < best) { best = sp2; J[i] = 2; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = 0;
#pragma unroll
        for (int i = 0; i < 3 * IL_PX; ++i) {
            const int px = i / 3, ch = i - 3 * px;
            int s = fb_get(sp, i);
            if constexpr (EDGES) {
                if (J[px] != 0 && px < n) {
                    const int xa = min(max(x0 + px + J[px], 0), W - 1), xb = min(max(x0 + px - J[px], 0), W - 1);
                    s = ((int)rup[3 * xa + ch] + (int)rdn[3 * xb + ch]) >> 1;
                }
            }
            const int d = fb_get(dw, i);
            const int v = min(max(s, d - diff[px]), d + diff[px]);      // diff >= 0 and d in [0, 255]: v is a byte
            o[i >> 2] |= (unsigned)v << (8 * (i & 3));
        }
        fb_store(dst, n, o);
    }
}

__device__ __forceinline__ unsigned long long il_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(IL_NTH)
interlace_scores_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ scene, unsigned long long* __restrict__ D, int t0,
                        int L, int H, int W) {
    __shared__ int s_first[IL_SR][IL_SC][IL_PX], s_last[IL_SR][IL_SC][IL_PX];
    __shared__ unsigned long long s_sum[IL_NTH / 64][2];
    const int t = t0 + (int)blockIdx.y;
    if (t + 1 >= L || scene[t + 1] != scene[t]) return;                 // the whole workgroup: the last frame of a scene keeps its zeros
    const int tid = (int)threadIdx.x, cgi = tid & (IL_SC - 1), run = tid / IL_SC;
    const int G = (W + IL_PX - 1) >> 2, g = (int)blockIdx.x * IL_SC + cgi;
    const int x0 = g * IL_PX, n = g < G ? min(IL_PX, W - x0) : 0;       // n == 0: a lane past the row, it adds nothing
    const int last = 2 * ((H - 2) / 2);                                 // the rows scored are [1, last]; H >= 4 here
    const int per = max(2, (H + IL_SR - 1) / IL_SR);                    // rows per run: two at least, so that a run's first row
    const int a = run * per, b = min(min(a + per, H), last + 2);        // that is scored has its second row in the same run
    const long long FB = 3LL * H * W;
    const uint8_t* C = frames + t * FB + 3 * x0;
    const uint8_t* N = C + FB;
    const int rowb = 3 * W;
    unsigned long long acc[2] = {0, 0};
    int c2[IL_PX] = {0, 0, 0, 0}, c1[IL_PX] = {0, 0, 0, 0}, n1[IL_PX] = {0, 0, 0, 0};   // Y_C[r - 2], Y_C[r - 1], Y_N[r - 1]
    int va[IL_PX] = {0, 0, 0, 0}, vb[IL_PX] = {0, 0, 0, 0};             // 2 Y_N[y] minus the one neighbour row the run owns, y = a and b - 1
    if (n > 0 && a < b) {
#pragma unroll 4
        for (int r = a; r < b; ++r) {
            unsigned wc[3], wn[3];
            int yc[IL_PX], yn[IL_PX];
            fb_load(C + (long long)r * rowb, n, wc);
            fb_load(N + (long long)r * rowb, n, wn);
            fb_luma4(wc, yc);
            fb_luma4(wn, yn);
            if (r == a) {
#pragma unroll
                for (int i = 0; i < IL_PX; ++i) s_first[run][cgi][i] = yc[i];
            }
            if (r == a + 1) {
#pragma unroll
                for (int i = 0; i < IL_PX; ++i) va[i] = 2 * n1[i] - yc[i];
            }
            if (r >= a + 2 && r - 1 <= last) {                          // y = r - 1 in [a + 1, b - 2]: all three rows are the run's
                int s = 0;
#pragma unroll
                for (int i = 0; i < IL_PX; ++i)
                    if (i < n) s += abs(2 * n1[i] - c2[i] - yc[i]);
                acc[(r - 1) & 1] += (unsigned)s;
            }
            if (r == b - 1) {
#pragma unroll
                for (int i = 0; i < IL_PX; ++i) {
                    s_last[run][cgi][i] = yc[i];
                    vb[i] = 2 * yn[i] - c1[i];
                }
            }
#pragma unroll
            for (int i = 0; i < IL_PX; ++i) {
                c2[i] = c1[i];
                c1[i] = yc[i];
                n1[i] = yn[i];
            }
        }
    }
    __syncthreads();
    if (n > 0 && a < b) {
        // y = a: the row above is the last row of the run above (a >= 1 means run >= 1; a <= last means that run ends at a)
        if (a >= 1 && a <= last) {
            int s = 0;
#pragma unroll
            for (int i = 0; i < IL_PX; ++i)
                if (i < n) s += abs(va[i] - s_last[run - 1][cgi][i]);
            acc[a & 1] += (unsigned)s;
        }
        // y = b - 1: the row below is the first row of the run below (b - 1 <= last means b = a + per <= H - 1)
        if (b - 1 > a && b - 1 <= last) {
            int s = 0;
#pragma unroll
            for (int i = 0; i < IL_PX; ++i)
                if (i < n) s += abs(vb[i] - s_first[run + 1][cgi][i]);
            acc[(b - 1) & 1] += (unsigned)s;
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned long long v = il_wave_sum(acc[q]);
        if (lane == 0) s_sum[wave][q] = v;
    }
    __syncthreads();
    if (tid < 2) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < IL_NTH / 64; ++w) v += s_sum[w][tid];
        if (v) atomicAdd(D + 2LL * t + tid, v);
    }
}

}  // namespace

extern "C" int e2fgvi_interlace_scores(const uint8_t* frames, const int32_t* scene, int64_t* D, int32_t L, int32_t H, int32_t W,
                                       void* stream) {
    if (int rc = fb_check_sizes("interlace_scores", L, H, W)) return rc;
    if (L == 0 || H == 0 || W == 0) return 0;                      // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && scene && D, E2FGVI_EINVAL, "interlace_scores: null pointer");
    E2_REQUIRE(((uintptr_t)scene & 3) == 0 && ((uintptr_t)D & 7) == 0, E2FGVI_EINVAL,
               "interlace_scores: scene must be 4-byte aligned and D 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(D, 0, sizeof(int64_t) * 2 * (size_t)L, st);
    E2_REQUIRE(e == hipSuccess, (int)e, "interlace_scores: hipMemsetAsync failed: %s", hipGetErrorString(e));
    if (H < 4 || L < 2) return 0;                                  // no row is scored, or no pair: the zeros are the answer
    const unsigned nblk = (unsigned)cdiv(cdiv(W, IL_PX), IL_SC);
    return fb_slabs("interlace_scores", L - 1, [&](int t0, unsigned n) {               // the L - 1 pairs
        hipLaunchKernelGGL(interlace_scores_kernel, dim3(nblk, n), dim3(IL_NTH), 0, st, frames, scene,
                           reinterpret_cast<unsigned long long*>(D), t0, L, H, W);
    });
}

extern "C" int e2fgvi_deinterlace(const uint8_t* frames, const int32_t* scene, uint8_t* out, int32_t L, int32_t H, int32_t W,
                                  int32_t tff, int32_t mode, int32_t guard, int32_t edges, void* stream) {
    if (int rc = fb_check_sizes("deinterlace", L, H, W)) return rc;
    E2_REQUIRE(tff == 0 || tff == 1, E2FGVI_EINVAL, "deinterlace: tff must be 0 or 1, got %d", tff);
    E2_REQUIRE(mode >= 0 && mode <= 2, E2FGVI_EINVAL, "deinterlace: mode must be in [0, 2], got %d", mode);
    E2_REQUIRE(guard == 0 || guard == 1, E2FGVI_EINVAL, "deinterlace: guard must be 0 or 1, got %d", guard);
    E2_REQUIRE(edges >= 0 && edges <= 2, E2FGVI_EINVAL, "deinterlace: edges must be in [0, 2], got %d", edges);
    if (L == 0 || H == 0 || W == 0) return 0;                      // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && scene && out, E2FGVI_EINVAL, "deinterlace: null pointer");
    E2_REQUIRE(((uintptr_t)scene & 3) == 0, E2FGVI_EINVAL, "deinterlace: scene must be 4-byte aligned");
    const uint64_t fb = 3ull * (uint64_t)H * (uint64_t)W;
    E2_REQUIRE(fb_disjoint(frames, fb * (uint64_t)L, out, fb * (uint64_t)L * (mode == 0 ? 2 : 1)), E2FGVI_EINVAL,
               "deinterlace: out must not overlap frames (a picture reads three frames)");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = (unsigned)(cdiv(cdiv(W, IL_PX), IL_TX) * cdiv(H, IL_TY * IL_R));       // at most 2^26 / 4 + 2^22 tiles
    auto kernel = edges > 0 ? (tff ? interlace_fields_kernel<true, 0> : interlace_fields_kernel<true, 1>)
                            : (tff ? interlace_fields_kernel<false, 0> : interlace_fields_kernel<false, 1>);
    return fb_slabs("deinterlace", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(kernel, dim3(nblk, n), dim3(IL_NTH), 0, st, frames, scene, out, t0, L, H, W, mode, guard, edges);
    });
}
