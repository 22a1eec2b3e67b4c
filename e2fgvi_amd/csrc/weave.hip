// Weave stabiliser (video.stabilize): the frame-to-frame translation of the picture from banded luma profiles, a smoothed path, and
// the frames moved back onto it.  Pure integers; include/e2fgvi_hip.h has the definition, tests/weave_cases.py restates it in
// numpy, word for word and byte for byte.
//   frames uint8 [L][H][W][3];  Y = (77 R + 150 G + 29 B + 128) >> 8 (the scene detector's luma);  WV_NB = 8 bands per axis
//
// The profiles pass.  col[t][b][x] = the sum of Y over the rows of band b, row[t][b][y] = the sum over the columns of band b.  A
// workgroup owns up to WV_RS = 32 consecutive rows of ONE row band of one frame, all columns: the rows are one run of pixels of the
// frame, read as in csrc/flicker.hip -- groups of four pixels, three dwords each when the frame starts on a dword, WV_UN = 4
// groups of a thread asked for before the first is used; a group that the run owns only in part (its ends, when W is no multiple
// of four) is read by bytes, and only the pixels the run owns: every frame byte is read once.  Both profile sets come from that
// read: Y goes to s_col[x] (neighbouring lanes hit neighbouring words: no bank conflict) and to the row sum of (row, column band)
// with integer LDS atomics; the row sums are kept in WV_RC = 8 copies (word (row 8 + band) 8 + tid % 8), since all lanes of a wave
// hit one or two of them, and four pixels of one row and band are one atomic of their sum.  The column band of x comes from a byte
// table in LDS, (8 x + 7) / W.  After the barrier the run's column sums are added to col with integer global atomics (the entry
// clears col on the stream first; a band has at most ceil(H / 8 / 32) runs) and its row sums are stored: a (row, band) pair belongs
// to one workgroup.  Integer atomics: exact, the same in every run.  The sides are at most WV_SIDE_MAX = 4096 (a profile lives in
// LDS here and in the match), so a sum is at most 255 * 512.
//
// The match pass is ONE launch: workgroup (t, axis).  Per band the gradient profiles of frames t - 1 and t go to LDS; the 2 R + 1
// shifts and the texture sum are jobs dealt to the four waves, a wave strides over the window and adds its lanes' 64-bit sums with
// shuffles: no barrier inside the loop over the shifts.  Thread 0 picks the best shift, the sub-pixel part and the validity of the
// band, and after the last band the lower median.
//
// The path pass: thread (t, axis).  q_t - p_t needs the motion of the 2 k_t <= 2 WV_SPAN_MAX pairs around t alone (p_t is an
// integer, so floor((2 sum p_u + n) / 2n) - p_t = floor((2 sum (p_u - p_t) + n) / 2n)): no scan over the segment.
//
// The apply pass.  The fractions fx, fy are the same for a whole frame.  A thread takes WV_AIT = 4 groups of four pixels of a row
// whose taps all lie inside the frame: per tap row the 5 C bytes from the first tap on are read as the dwords that hold them
// (inside the frames buffer, or the group goes the slow way) and shifted into place, so the taps of an output dword are four
// dwords in registers; they are blended two bytes at a time (wv_blend2), and a frame moved by whole pixels is copied.  The 4 C
// output bytes go out as C dwords when out starts on a dword, the four mask bytes as one.  Groups at the left and right border,
// groups that span two rows and the last group of a frame go byte by byte with clamped taps -- not where they are met, which
// holds up the wave of every row's end: they are listed in LDS and done after a barrier by a thread per (group, pixel, channel).
// profiles/weave.txt has what each of these steps measured.
#include "frame_bytes.h"

namespace {

constexpr int WV_NTH = 256;
constexpr int WV_NB = 8;                  // bands per axis
constexpr int WV_PX = FB_PX;              // pixels per group
constexpr int WV_RS = 32;                 // rows per workgroup of the profiles kernel
constexpr int WV_UN = 4;                  // groups of a thread in flight in the profiles kernel
constexpr int WV_RC = 8;                  // copies of the row sums in LDS: a power of two
constexpr int WV_AIT = 4;                 // groups per thread of the apply kernel
constexpr int WV_APX = WV_NTH * WV_PX * WV_AIT;
constexpr int WV_SIDE_MAX = 4096;         // H and W of the profiles and the match: a profile lives in LDS
constexpr int WV_RADIUS_MAX = 32, WV_SPAN_MAX = 16, WV_SHIFT_MAX = 64, WV_TEX_MAX = 65535;

__global__ void __launch_bounds__(WV_NTH)
weave_profiles_kernel(const uint8_t* __restrict__ frames, int t0, int H, int W, int nchunk, int* __restrict__ col,
                      int* __restrict__ row) {
    __shared__ int s_col[WV_SIDE_MAX];
    __shared__ int s_row[WV_RS * WV_NB * WV_RC];
    __shared__ uint8_t s_band[WV_SIDE_MAX];
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.x / nchunk, c = (int)blockIdx.x - b * nchunk;
    const int r0 = ((b * H) >> 3) + c * WV_RS, rend = ((b + 1) * H) >> 3;
    if (r0 >= rend) return;                                        // the whole workgroup: a short (or empty) band has fewer runs
    const int r1 = min(r0 + WV_RS, rend);
    for (int i = tid; i < W; i += WV_NTH) {
        s_col[i] = 0;
        s_band[i] = (uint8_t)((8 * i + 7) / W);                    // the last band that starts at or in front of column i
    }
    for (int i = tid; i < WV_RS * WV_NB * WV_RC; i += WV_NTH) s_row[i] = 0;
    __syncthreads();
    const int N = H * W;
    const uint8_t* fr = frames + (long long)t * N * 3;
    const int P0 = r0 * W, P1 = r1 * W;                            // the run's pixels
    const int g0 = P0 >> 2, g1 = (P1 + WV_PX - 1) >> 2;            // the groups that hold one of them
    const bool aligned = ((uintptr_t)fr & 3) == 0;                 // the same for every thread of the frame: a group is 12 bytes
    int* mine = s_row + (tid & (WV_RC - 1));
    // row and column of a group's first pixel: two divisions per thread, then steps
    int gy = (g0 + tid) * WV_PX / W, gx = (g0 + tid) * WV_PX - gy * W;
    const int sy = WV_NTH * WV_PX / W, sx = WV_NTH * WV_PX - sy * W;
    for (int base = g0; base < g1; base += WV_NTH * WV_UN) {
        unsigned w[WV_UN][3];
#pragma unroll
        for (int k = 0; k < WV_UN; ++k) {
            const int p = (base + k * WV_NTH + tid) * WV_PX;
            w[k][0] = w[k][1] = w[k][2] = 0;
            if (aligned && p >= P0 && p + WV_PX <= P1) fb_load_dwords(fr + (long long)p * 3, w[k]);       // the twelve bytes are the run's
        }
#pragma unroll
        for (int k = 0; k < WV_UN; ++k) {
            const int g = base + k * WV_NTH + tid;
            int yr = gy, x = gx;                                   // of the group's first pixel
            gx += sx;                                              // the thread's next group is WV_NTH groups on
            gy += sy;
            if (gx >= W) { gx -= W; ++gy; }
            if (g >= g1) continue;
            const int p = g * WV_PX;
            if (aligned && p >= P0 && p + WV_PX <= P1) {
                int y[WV_PX];
                fb_luma4(w[k], y);
                if (x + WV_PX <= W && s_band[x] == s_band[x + WV_PX - 1]) {          // one row, one band
#pragma unroll
                    for (int j = 0; j < WV_PX; ++j) atomicAdd(s_col + x + j, y[j]);
                    atomicAdd(mine + ((yr - r0) * WV_NB + (int)s_band[x]) * WV_RC, y[0] + y[1] + y[2] + y[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < WV_PX; ++j) {
                        atomicAdd(s_col + x, y[j]);
                        atomicAdd(mine + ((yr - r0) * WV_NB + (int)s_band[x]) * WV_RC, y[j]);
                        if (++x == W) { x = 0; ++yr; }
                    }
                }
            } else {
                for (int j = 0; j < WV_PX; ++j) {
                    const int pp = p + j;
                    if (pp >= P0 && pp < P1) {
                        const uint8_t* q = fr + (long long)pp * 3;
                        const int y = fb_luma(q[0], q[1], q[2]);
                        atomicAdd(s_col + x, y);
                        atomicAdd(mine + ((yr - r0) * WV_NB + (int)s_band[x]) * WV_RC, y);
                    }
                    if (++x == W) { x = 0; ++yr; }
                }
            }
        }
    }
    __syncthreads();
    int* cdst = col + ((long long)t * WV_NB + b) * W;
    for (int i = tid; i < W; i += WV_NTH) {
        const int v = s_col[i];
        if (v) atomicAdd(cdst + i, v);
    }
    for (int i = tid; i < (r1 - r0) * WV_NB; i += WV_NTH) {
        int sum = 0;
#pragma unroll
        for (int k = 0; k < WV_RC; ++k) sum += s_row[i * WV_RC + ((k + tid) & (WV_RC - 1))];
        row[((long long)t * WV_NB + (i & (WV_NB - 1))) * H + r0 + (i >> 3)] = sum;
    }
}

__device__ __forceinline__ long long wv_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ void __launch_bounds__(WV_NTH)
weave_match_kernel(const int* __restrict__ col, const int* __restrict__ row, const int* __restrict__ scene, int H, int W, int R,
                   int tex, int* __restrict__ motion) {
    __shared__ int s_g[2][WV_SIDE_MAX];              // the gradient band of frame t - 1 and of frame t
    __shared__ long long s_cost[2 * WV_RADIUS_MAX + 2];
    __shared__ int s_val[WV_NB];
    const int t = (int)blockIdx.x, axis = (int)blockIdx.y;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = axis ? H : W, other = axis ? W : H;
    const int* P = axis ? row : col;
    const int lo = R + 1, hi = n - R - 1;
    // the same for the whole workgroup: frame 0, the first frame of a scene and a window of fewer than 2 R elements measure nothing
    if (t == 0 || scene[t] != scene[t - 1] || hi - lo < 2 * R) {
        if (tid == 0) motion[4LL * t + axis] = motion[4LL * t + 2 + axis] = 0;
        return;
    }
    int nvalid = 0;                                   // thread 0's
    for (int b = 0; b < WV_NB; ++b) {
        if (((b * other) >> 3) == (((b + 1) * other) >> 3)) continue;        // an empty band
        const int* Pp = P + ((long long)(t - 1) * WV_NB + b) * n;
        const int* Pc = P + ((long long)t * WV_NB + b) * n;
        for (int i = tid; i < n; i += WV_NTH) {
            const bool in = i > 0 && i < n - 1;
            s_g[0][i] = in ? Pp[i + 1] - Pp[i - 1] : 0;
            s_g[1][i] = in ? Pc[i + 1] - Pc[i - 1] : 0;
        }
        __syncthreads();
        for (int j = wave; j < 2 * R + 2; j += WV_NTH / 64) {               // job j <= 2 R: the shift j - R; the last: the texture
            long long acc = 0;
            if (j <= 2 * R) {
                const int s = j - R;                                        // i + s in [1, n - 2]
                for (int i = lo + lane; i < hi; i += 64) acc += abs(s_g[1][i + s] - s_g[0][i]);
            } else {
                for (int i = lo + lane; i < hi; i += 64) acc += abs(s_g[0][i]);
            }
            acc = wv_wave_sum(acc);
            if (lane == 0) s_cost[j] = acc;
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0;
            long long c0 = s_cost[R];
            for (int a = 1; a <= R; ++a) {                                  // 0, -1, +1, -2, +2 ...: a tie keeps the earlier one
                if (s_cost[R - a] < c0) { c0 = s_cost[R - a]; best = -a; }
                if (s_cost[R + a] < c0) { c0 = s_cost[R + a]; best = a; }
            }
            if (best > -R && best < R) {
                const long long cm = s_cost[R + best - 1], cp = s_cost[R + best + 1];
                const long long den = cm - 2 * c0 + cp;
                if (den > 0 && s_cost[2 * R + 1] >= (long long)tex * (hi - lo)) {
                    long long delta = 0;
                    if (c0 != 0) {
                        const long long num = 16 * (cm - cp) + den;
                        delta = num / (2 * den);
                        if (num < 0 && delta * (2 * den) != num) --delta;   // the floor
                    }
                    s_val[nvalid++] = 16 * best + (int)delta;
                }
            }
        }
        __syncthreads();                                                    // s_g and s_cost are written again for the next band
    }
    if (tid == 0) {
        for (int i = 1; i < nvalid; ++i) {                                  // at most eight: insertion sort
            const int v = s_val[i];
            int j = i;
            for (; j > 0 && s_val[j - 1] > v; --j) s_val[j] = s_val[j - 1];
            s_val[j] = v;
        }
        motion[4LL * t + axis] = nvalid >= WV_NB / 2 ? s_val[(nvalid - 1) >> 1] : 0;
        motion[4LL * t + 2 + axis] = nvalid;
    }
}

__global__ void __launch_bounds__(WV_NTH)
weave_path_kernel(const int* __restrict__ motion, const int* __restrict__ scene, int L, int span, int max_shift, int subpixel,
                  int* __restrict__ shift) {
    const long long idx = (long long)blockIdx.x * WV_NTH + threadIdx.x;
    if (idx >= 2LL * L) return;
    const int t = (int)(idx >> 1), axis = (int)(idx & 1);
    // frame v starts a segment on this axis
    auto first = [&](int v) { return v == 0 || scene[v] != scene[v - 1] || motion[4LL * v + 2 + axis] < WV_NB / 2; };
    int back = 0, fwd = 0;
    while (back < span && !first(t - back)) ++back;
    while (fwd < span && t + fwd + 1 < L && !first(t + fwd + 1)) ++fwd;
    const int k = min(back, fwd);
    long long sum = 0, run = 0;                                             // the sum of p_u - p_t over the window
    for (int d = 1; d <= k; ++d) {
        run += motion[4LL * (t + d) + axis];
        sum += run;
    }
    run = 0;
    for (int d = 0; d < k; ++d) {
        run -= motion[4LL * (t - d) + axis];
        sum += run;
    }
    const long long nn = 2 * k + 1, num = 2 * sum + nn;
    long long q = num / (2 * nn);
    if (num < 0 && q * (2 * nn) != num) --q;                                // the floor
    const long long lim = 16LL * max_shift;
    int c = (int)(q < -lim ? -lim : (q > lim ? lim : q));
    if (!subpixel) c = ((c + 8) >> 4) * 16;
    shift[idx] = c;
}

// a dword of the byte string (lo, hi) that starts k bytes into lo
__device__ __forceinline__ unsigned wv_window(unsigned lo, unsigned hi, int k) {
    return (unsigned)(((((unsigned long long)hi) << 32) | lo) >> (8 * k));
}

// the blend of two bytes at a time: a .. d hold one byte in each half of a word, the weights are at most 256 and add up to 256.
// A sum is at most 255 * 256 + 128 < 2^16: the halves do not meet.  24-bit multiplies: the 32-bit one runs at a quarter of the rate
__device__ __forceinline__ unsigned wv_blend2(unsigned a, unsigned b, unsigned c, unsigned d, unsigned w00, unsigned w01, unsigned w10,
                                              unsigned w11) {
    return ((__umul24(a, w00) + __umul24(b, w01) + __umul24(c, w10) + __umul24(d, w11) + 0x00800080u) >> 8) & 0x00FF00FFu;
}

template <int C>
__global__ void __launch_bounds__(WV_NTH)
weave_apply_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ shift, int t0, int L, int H, int W,
                   uint8_t* __restrict__ out, uint8_t* __restrict__ mask) {
    constexpr int NS = (5 * C + 3) / 4;               // dwords that hold the 5 C bytes from the first tap on
    constexpr int ND = (5 * C + 3 + 3) / 4;           // the same when the first tap is up to 3 bytes into its dword
    const int t = t0 + (int)blockIdx.y;
    const int tid = (int)threadIdx.x;
    const int lim = 16 * WV_SHIFT_MAX;
    const int cx = min(max(shift[2LL * t], -lim), lim), cy = min(max(shift[2LL * t + 1], -lim), lim);
    // X = 16 x - cx: x0 = x + dx and the fraction is the same for every x
    const int dx = (-cx) >> 4, fx = (-cx) & 15, dy = (-cy) >> 4, fy = (-cy) & 15;
    const int w00 = (16 - fx) * (16 - fy), w01 = fx * (16 - fy), w10 = (16 - fx) * fy, w11 = fx * fy;
    const int N = H * W;
    const uint8_t* fr = frames + (long long)t * N * C;
    const uint8_t* end = frames + (long long)L * N * C;
    uint8_t* fo = out + (long long)t * N * C;
    uint8_t* fm = mask ? mask + (long long)t * N : nullptr;
    const bool out_dwords = ((uintptr_t)fo & 3) == 0, mask_dwords = ((uintptr_t)fm & 3) == 0;
    // the groups that go byte by byte (borders, a group over two rows, the end of a frame), listed here and done afterwards
    __shared__ int s_list[WV_NTH * WV_AIT];
    __shared__ int s_n;
    if (tid == 0) s_n = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < WV_AIT; ++k) {
        const int p = (int)blockIdx.x * WV_APX + k * WV_NTH * WV_PX + tid * WV_PX;      // < 2^26 + 4096
        if (p >= N) break;
        const int y = p / W, x = p - y * W;
        const int x0 = x + dx, y0 = y + dy;
        const int ya = min(max(y0, 0), H - 1), yb = min(max(y0 + 1, 0), H - 1);
        // four pixels of one row whose five tap columns x0 .. x0 + 4 lie in the frame
        bool fast = x + WV_PX <= W && x0 >= 0 && x0 + WV_PX <= W - 1;
        const uint8_t* A = fr + ((long long)ya * W + x0) * C;
        const uint8_t* B = fr + ((long long)yb * W + x0) * C;
        const int ka = (int)((uintptr_t)A & 3), kb = (int)((uintptr_t)B & 3);
        // the dwords read lie inside the frames buffer
        fast = fast && A - ka >= frames && A - ka + 4 * ND <= end && B - kb >= frames && B - kb + 4 * ND <= end;
        if (fast) {
            unsigned wa[ND + 1], wb[ND + 1], sa[NS], sb[NS], o[C];
            const unsigned* qa = reinterpret_cast<const unsigned*>(A - ka);
            const unsigned* qb = reinterpret_cast<const unsigned*>(B - kb);
#pragma unroll
            for (int i = 0; i < ND; ++i) wa[i] = qa[i];                     // (hipcc makes one or two wide loads of them)
            if (fy) {                                                       // the same for the whole frame
#pragma unroll
                for (int i = 0; i < ND; ++i) wb[i] = qb[i];
            } else {
#pragma unroll
                for (int i = 0; i < ND; ++i) wb[i] = 0;                     // weight 0
            }
            wa[ND] = wb[ND] = 0;
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                sa[i] = wv_window(wa[i], wa[i + 1], ka);
                sb[i] = wv_window(wb[i], wb[i + 1], kb);
            }
            if ((fx | fy) == 0) {                                           // whole pixels (the same for the whole frame): a copy
#pragma unroll
                for (int i = 0; i < C; ++i) o[i] = sa[i];
            } else {
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    // taps b and d are C bytes on; the even and the odd bytes of a dword are blended two at a time
                    const unsigned a4 = sa[i], b4 = wv_window(sa[i], sa[i + 1], C), c4 = sb[i], d4 = wv_window(sb[i], sb[i + 1], C);
                    o[i] = wv_blend2(a4 & 0x00FF00FFu, b4 & 0x00FF00FFu, c4 & 0x00FF00FFu, d4 & 0x00FF00FFu, w00, w01, w10, w11) |
                           (wv_blend2((a4 >> 8) & 0x00FF00FFu, (b4 >> 8) & 0x00FF00FFu, (c4 >> 8) & 0x00FF00FFu,
                                      (d4 >> 8) & 0x00FF00FFu, w00, w01, w10, w11) << 8);
                }
            }
            uint8_t* po = fo + (long long)p * C;
            if (out_dwords) {
#pragma unroll
                for (int i = 0; i < C; ++i) reinterpret_cast<unsigned*>(po)[i] = o[i];
            } else {
#pragma unroll
                for (int i = 0; i < 4 * C; ++i) po[i] = (uint8_t)(o[i >> 2] >> (8 * (i & 3)));
            }
            if (fm) {
                // the tap columns are inside: the tap rows decide
                const bool oy = y0 < 0 || y0 > H - 1 || (fy && y0 + 1 > H - 1);
                if (mask_dwords) {
                    *reinterpret_cast<unsigned*>(fm + p) = oy ? 0xFFFFFFFFu : 0u;
                } else {
#pragma unroll
                    for (int j = 0; j < WV_PX; ++j) fm[p + j] = oy ? 255 : 0;
                }
            }
        } else {
            s_list[atomicAdd(&s_n, 1)] = p;                                 // at most one entry per group of the workgroup
        }
    }
    __syncthreads();
    // the listed groups byte by byte, a thread per (group, pixel, channel): the order of the list does not matter
    const int items = s_n * WV_PX * C;
    for (int it = tid; it < items; it += WV_NTH) {
        const int gi = it / (WV_PX * C), r = it - gi * (WV_PX * C), j = r / C, ch = r - j * C;
        const int pp = s_list[gi] + j;
        if (pp >= N) continue;                                              // the last group of a frame may be short
        const int yy = pp / W, xx = pp - yy * W;
        const int u0 = xx + dx, v0 = yy + dy;
        const int xa = min(max(u0, 0), W - 1), xb = min(max(u0 + 1, 0), W - 1);
        const int va = min(max(v0, 0), H - 1), vb = min(max(v0 + 1, 0), H - 1);
        const uint8_t* ra = fr + (long long)va * W * C + ch;
        const uint8_t* rb = fr + (long long)vb * W * C + ch;
        const unsigned a = ra[xa * C], bq = ra[xb * C], cq = rb[xa * C], d = rb[xb * C];
        fo[(long long)pp * C + ch] = (uint8_t)((__umul24(a, w00) + __umul24(bq, w01) + __umul24(cq, w10) + __umul24(d, w11) + 128u) >> 8);
        if (fm && ch == 0) {
            const bool ox = u0 < 0 || u0 > W - 1 || (fx && (u0 + 1 < 0 || u0 + 1 > W - 1));
            const bool oy = v0 < 0 || v0 > H - 1 || (fy && (v0 + 1 < 0 || v0 + 1 > H - 1));
            fm[pp] = (ox || oy) ? 255 : 0;
        }
    }
}

int wv_check_sizes(const char* who, int32_t L, int32_t H, int32_t W, bool sides) {
    // a profile lives in LDS: a side beyond WV_SIDE_MAX is refused as such, however many pixels the frame has (4096^2 < 2^26, so
    // the shared check then only refuses a negative size, which it names first as before)
    if (sides && L >= 0 && H >= 0 && W >= 0)
        E2_REQUIRE(H <= WV_SIDE_MAX && W <= WV_SIDE_MAX, E2FGVI_EINVAL, "%s: needs H and W <= %d, got %d x %d", who, WV_SIDE_MAX, H, W);
    return fb_check_sizes(who, L, H, W);
}

}  // namespace

extern "C" int e2fgvi_weave_profiles(const uint8_t* frames, int32_t* col, int32_t* row, int32_t L, int32_t H, int32_t W,
                                     void* stream) {
    if (int rc = wv_check_sizes("weave_profiles", L, H, W, true)) return rc;
    if (L == 0 || H == 0 || W == 0) return 0;                      // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && col && row, E2FGVI_EINVAL, "weave_profiles: null pointer");
    E2_REQUIRE((((uintptr_t)col | (uintptr_t)row) & 3) == 0, E2FGVI_EINVAL, "weave_profiles: col and row must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(col, 0, sizeof(int32_t) * WV_NB * (size_t)W * (size_t)L, st);
    E2_REQUIRE(e == hipSuccess, (int)e, "weave_profiles: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const int nchunk = cdiv(cdiv(H, WV_NB), WV_RS);                // a band has at most ceil(H / 8) rows
    return fb_slabs("weave_profiles", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(weave_profiles_kernel, dim3((unsigned)(WV_NB * nchunk), n), dim3(WV_NTH), 0, st, frames, t0, H, W, nchunk, col,
                           row);
    });
}

extern "C" int e2fgvi_weave_match(const int32_t* col, const int32_t* row, const int32_t* scene, int32_t* motion, int32_t L,
                                  int32_t H, int32_t W, int32_t radius, int32_t tex, void* stream) {
    if (int rc = wv_check_sizes("weave_match", L, H, W, true)) return rc;
    E2_REQUIRE(radius >= 1 && radius <= WV_RADIUS_MAX, E2FGVI_EINVAL, "weave_match: radius must be in [1, %d], got %d", WV_RADIUS_MAX,
               radius);
    E2_REQUIRE(tex >= 0 && tex <= WV_TEX_MAX, E2FGVI_EINVAL, "weave_match: tex must be in [0, %d], got %d", WV_TEX_MAX, tex);
    if (L == 0 || H == 0 || W == 0) return 0;                      // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(col && row && scene && motion, E2FGVI_EINVAL, "weave_match: null pointer");
    E2_REQUIRE((((uintptr_t)col | (uintptr_t)row | (uintptr_t)scene | (uintptr_t)motion) & 3) == 0, E2FGVI_EINVAL,
               "weave_match: col, row, scene and motion must be 4-byte aligned");
    hipLaunchKernelGGL(weave_match_kernel, dim3((unsigned)L, 2, 1), dim3(WV_NTH), 0, (hipStream_t)stream, col, row, scene, H, W, radius,
                       tex, motion);
    E2_LAUNCH_CHECK("weave_match");
    return 0;
}

extern "C" int e2fgvi_weave_path(const int32_t* motion, const int32_t* scene, int32_t* shift, int32_t L, int32_t span,
                                 int32_t max_shift, int32_t subpixel, void* stream) {
    E2_REQUIRE(L >= 0, E2FGVI_EINVAL, "weave_path: negative size (L = %d)", L);
    E2_REQUIRE(span >= 0 && span <= WV_SPAN_MAX, E2FGVI_EINVAL, "weave_path: span must be in [0, %d], got %d", WV_SPAN_MAX, span);
    E2_REQUIRE(max_shift >= 1 && max_shift <= WV_SHIFT_MAX, E2FGVI_EINVAL, "weave_path: max_shift must be in [1, %d], got %d",
               WV_SHIFT_MAX, max_shift);
    E2_REQUIRE(subpixel == 0 || subpixel == 1, E2FGVI_EINVAL, "weave_path: subpixel must be 0 or 1, got %d", subpixel);
    if (L == 0) return 0;                                          // no frame: no launch, and the pointers are not looked at
    E2_REQUIRE(motion && scene && shift, E2FGVI_EINVAL, "weave_path: null pointer");
    E2_REQUIRE((((uintptr_t)motion | (uintptr_t)scene | (uintptr_t)shift) & 3) == 0, E2FGVI_EINVAL,
               "weave_path: motion, scene and shift must be 4-byte aligned");
    const unsigned nblk = (unsigned)cdiv64(2LL * L, WV_NTH);
    hipLaunchKernelGGL(weave_path_kernel, dim3(nblk), dim3(WV_NTH), 0, (hipStream_t)stream, motion, scene, L, span, max_shift,
                       subpixel, shift);
    E2_LAUNCH_CHECK("weave_path");
    return 0;
}

extern "C" int e2fgvi_weave_apply(const uint8_t* frames, const int32_t* shift, uint8_t* out, uint8_t* mask, int32_t L, int32_t H,
                                  int32_t W, int32_t C, void* stream) {
    if (int rc = wv_check_sizes("weave_apply", L, H, W, false)) return rc;
    E2_REQUIRE(C == 1 || C == 3, E2FGVI_EINVAL, "weave_apply: C must be 1 or 3, got %d", C);
    const int N = H * W;
    if (L == 0 || N == 0) return 0;                                // no pixel: no launch, and the pointers are not looked at
    E2_REQUIRE(frames && shift && out, E2FGVI_EINVAL, "weave_apply: null pointer");
    E2_REQUIRE(((uintptr_t)shift & 3) == 0, E2FGVI_EINVAL, "weave_apply: shift must be 4-byte aligned");
    const uint64_t px = (uint64_t)L * (uint64_t)N;
    E2_REQUIRE(fb_disjoint(frames, px * C, out, px * C), E2FGVI_EINVAL,
               "weave_apply: out must not overlap frames (a shifted read is not in order)");
    E2_REQUIRE(!mask || (fb_disjoint(frames, px * C, mask, px) && fb_disjoint(out, px * C, mask, px)), E2FGVI_EINVAL,
               "weave_apply: mask must not overlap frames or out");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = (unsigned)((N + WV_APX - 1) / WV_APX);
    auto kernel = C == 3 ? weave_apply_kernel<3> : weave_apply_kernel<1>;
    return fb_slabs("weave_apply", L, [&](int t0, unsigned n) {
        hipLaunchKernelGGL(kernel, dim3(nblk, n), dim3(WV_NTH), 0, st, frames, shift, t0, L, H, W, out, mask);
    });
}
