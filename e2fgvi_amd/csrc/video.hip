// Byte-side kernels of the sliding-window video driver: everything test.py does to the
// uint8 frames and masks around the model call, on the device.  HBM-bound integer / byte work: one thread per output
// element, coalesced along the innermost (channel / x) index; results are bit-exact with the numpy / PIL reference.
#include "frame_bytes.h"

namespace {

constexpr int NTH = 256;
// A launch holds fewer than 2^32 threads: the runtime keeps 32 bits of their number and runs `threads mod 2^32` of them without an
// error (float_to_u8 of 2^32 + 624 704 floats converted the first 624 896).  So the grid of a thread-per-element kernel is capped
// below that and its threads stride over what is left; up to 2^32 - 256 elements that is one element a thread, as before.
constexpr long long GRID_BLOCKS_MAX = (1LL << 24) - 1;
inline unsigned blocks_for(long long n) {
    const long long b = (n + NTH - 1) / NTH;
    return (unsigned)(b < GRID_BLOCKS_MAX ? b : GRID_BLOCKS_MAX);
}
// for (long long idx : the elements of this thread): the first is the thread's number in the grid, the step the grid's threads
#define E2_GRID_STRIDE(idx, n) \
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < (n); idx += (long long)gridDim.x * blockDim.x)

// Mask preparation (test.py:56-69): NEAREST resize to the frame size, binarise (> 0), 4x dilation with the 3x3 cross.
// The source row / column of every output row / column comes in as a table (Pillow builds the same tables in
// ImagingScaleAffine; the host mirrors its double arithmetic, e2fgvi_amd/video.py::nearest_table).
// With `ids` (a window of a video) output frame l is made from frame ids[l] of the Lsrc source frames; an id outside [0, Lsrc)
// gives an empty mask, so the kernel stays in bounds whatever the table holds.
__global__ void mask_prepare_kernel(const unsigned char* __restrict__ src, int Lsrc, const int* __restrict__ ids, int Hin, int Win,
                                    const int* __restrict__ ytab, const int* __restrict__ xtab, unsigned char* __restrict__ dst, int L,
                                    int H, int W, int iters) {
    E2_GRID_STRIDE(idx, (long long)L * H * W) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const int l = (int)(idx / ((long long)W * H));
        const int ls = ids ? ids[l] : l;
        if (ls < 0 || ls >= Lsrc) { dst[idx] = 0; continue; }
        const unsigned char* s = src + (long long)ls * Hin * Win;
        // `iters` dilations with the 3x3 cross = OR over the L1 ball of that radius, clipped to the image
        // (cv2.dilate ignores out-of-image pixels; test.py:64-68)
        int hit = 0;
        for (int dy = -iters; dy <= iters && !hit; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            const long long row = (long long)ytab[yy] * Win;
            const int r = iters - (dy < 0 ? -dy : dy);
            for (int dx = -r; dx <= r; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= W) continue;
                if (s[row + xtab[xx]] != 0) { hit = 1; break; }
            }
        }
        dst[idx] = (unsigned char)hit;
    }
}

// masked, normalised, mirror-padded clip (test.py:146-165): out[ti][c][y][x] = (frame/255*2-1) * (1 - mask), rows / columns
// past the frame take the flipped image (cat([x, flip(x)])[: h + pad])
__global__ void masked_clip_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ masks,
                                   const int* __restrict__ ids, float* __restrict__ out, int t, int H, int W, int Hp, int Wp) {
    E2_GRID_STRIDE(idx, (long long)t * 3 * Hp * Wp) {
        const int x = (int)(idx % Wp);
        long long r = idx / Wp;
        const int y = (int)(r % Hp);
        r /= Hp;
        const int c = (int)(r % 3);
        const int ti = (int)(r / 3);
        const int sy = y < H ? y : 2 * H - 1 - y;
        const int sx = x < W ? x : 2 * W - 1 - x;
        const long long pix = ((long long)ids[ti] * H + sy) * W + sx;
        const float v = ((float)frames[pix * 3 + c] / 255.0f) * 2.0f - 1.0f;
        const float m = (float)masks[pix];
        out[idx] = v * (1.0f - m);
    }
}

// compositing + 0.5/0.5 blending of overlapping windows (test.py:168-179):
//   img = uint8((pred+1)/2*255) * mask + frame * (1-mask);  comp = img (first time)  or  comp*0.5 + img*0.5
__global__ void composite_kernel(const float* __restrict__ pred, const int* __restrict__ ids, const unsigned char* __restrict__ first,
                                 const unsigned char* __restrict__ frames, const unsigned char* __restrict__ masks,
                                 float* __restrict__ comp, int n, int H, int W, int Hp, int Wp) {
    E2_GRID_STRIDE(idx, (long long)n * H * W * 3) {
        const int c = (int)(idx % 3);
        long long r = idx / 3;
        const int x = (int)(r % W);
        r /= W;
        const int y = (int)(r % H);
        const int i = (int)(r / H);
        const int f = ids[i];
        const long long pix = ((long long)f * H + y) * W + x;
        unsigned char img = frames[pix * 3 + c];
        if (masks[pix]) {
            const float p = pred[(((long long)i * 3 + c) * Hp + y) * Wp + x];
            img = (unsigned char)(int)(((p + 1.0f) / 2.0f) * 255.0f);
        }
        const float v = (float)img;
        comp[pix * 3 + c] = first[i] ? v : comp[pix * 3 + c] * 0.5f + v * 0.5f;
    }
}

// Frame resize (test.py:97-104,127, core/dataset.py:115): one separable pass of Pillow's 8-bit BICUBIC resample along H
// (VERTICAL) or W of uint8 [L,H,W,3].  Output o of the axis reads taps bounds[o] = (first, count) of the source axis with the
// fixed-point weights coeffs[o][*] (22 fraction bits, built by e2fgvi_amd/video.py::bicubic_tables like Pillow's
// precompute_coeffs) and stores clamp((2^21 + sum) >> 22, 0, 255) from an int32 accumulator, as Pillow does per pass.
// One block per output row (l, y) at a time, its threads along the row's x*3+c bytes: coalesced stores; the vertical pass
// also reads rows coalesced, the horizontal one reads a row's bytes at stride 3 per tap (L1 hits).  The horizontal pass takes a
// row window: it reads rows [row0, row0 + nrows) of every frame (frames H rows apart) and writes [L,nrows,n_out,3] (frames nrows
// rows apart) -- Pillow's ImagingResample runs its width pass only over the rows its height pass will read.  The vertical pass
// and the whole-frame horizontal one have row0 = 0, nrows = H.  With `ids` output frame l reads frame ids[l] of the Lsrc source
// frames (the frames of a window, picked out of the video by the pass itself: no source-size copy of them is made); an id
// outside [0, Lsrc) gives a frame of zeros.
template <bool VERTICAL>
__global__ void resample_u8_kernel(const unsigned char* __restrict__ src, int Lsrc, const int* __restrict__ ids,
                                   unsigned char* __restrict__ dst, int L, int H, int W, int n_out, int row0, int nrows,
                                   const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize) {
    const int Ho = VERTICAL ? n_out : nrows;
    const int Wo = VERTICAL ? W : n_out;
    const int n_in = VERTICAL ? H : W;
    const int row = Wo * 3;
    const long long rows = (long long)L * Ho;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int y = (int)(r % Ho);
        const long long l = ids ? (long long)ids[r / Ho] : r / Ho;
        unsigned char* d = dst + r * row;
        if (l < 0 || l >= Lsrc) {
            for (int xc = threadIdx.x; xc < row; xc += blockDim.x) d[xc] = 0;
            continue;
        }
        for (int xc = threadIdx.x; xc < row; xc += blockDim.x) {
            const int x = xc / 3;
            const int o = VERTICAL ? y : x;
            // the tap range is clipped to the source axis, so the loads stay in bounds whatever the tables hold
            int first = bounds[2 * o];
            first = first < 0 ? 0 : (first > n_in ? n_in : first);
            int taps = bounds[2 * o + 1];
            taps = taps < ksize ? taps : ksize;
            taps = taps < n_in - first ? taps : n_in - first;
            const int* k = coeffs + (long long)o * ksize;
            const unsigned char* s;
            long long step;
            if (VERTICAL) {
                s = src + (l * H + first) * (long long)W * 3 + xc;
                step = (long long)W * 3;
            } else {
                s = src + (l * H + row0 + y) * (long long)W * 3 + first * 3 + (xc - 3 * x);
                step = 3;
            }
            int acc = 1 << 21;
            for (int j = 0; j < taps; ++j) acc += (int)s[j * step] * k[j];
            acc >>= 22;
            d[xc] = (unsigned char)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
        }
    }
}

__global__ void float_to_u8_kernel(const float* __restrict__ src, unsigned char* __restrict__ dst, long long n) {
    E2_GRID_STRIDE(idx, n) dst[idx] = (unsigned char)(int)src[idx];
}

// ndarray.astype(float32) of uint8 frames: the source-size accumulator of inpaint_video(region="track") starts as the source.
// Four bytes per thread: one 32-bit load and one 16-byte store when VEC (both bases aligned), the last n % 4 bytes one by one.
template <bool VEC>
__global__ void u8_to_float_kernel(const unsigned char* __restrict__ src, float* __restrict__ dst, long long n) {
    E2_GRID_STRIDE(g, (n + 3) / 4) {
        const long long i = g * 4;
        if (VEC && i + 4 <= n) {
            const unsigned q = *reinterpret_cast<const unsigned*>(src + i);
            *reinterpret_cast<float4*>(dst + i) = make_float4((float)(q & 255u), (float)((q >> 8) & 255u), (float)((q >> 16) & 255u),
                                                              (float)(q >> 24));
        } else {
            for (long long k = i; k < n && k < i + 4; ++k) dst[k] = (float)src[k];
        }
    }
}

// model output NCHW float in (-1,1) -> NHWC uint8 (what test.py:168-171 turns a prediction into), cropped to H x W
__global__ void pred_to_u8_kernel(const float* __restrict__ pred, unsigned char* __restrict__ dst, int N, int H, int W, int Hp, int Wp) {
    E2_GRID_STRIDE(idx, (long long)N * H * W * 3) {
        const int c = (int)(idx % 3);
        long long r = idx / 3;
        const int x = (int)(r % W);
        r /= W;
        const int y = (int)(r % H);
        const int n = (int)(r / H);
        const float p = pred[(((long long)n * 3 + c) * Hp + y) * Wp + x];
        dst[idx] = (unsigned char)(int)(((p + 1.0f) / 2.0f) * 255.0f);
    }
}

// Frame slabs between a cache and a window (test.py:152: the frames of a window are picked by id out of the whole video;
// with reuse=True their encoder features and flows are picked out of a cache instead).  row i of `rows` [n][slab] pairs with
// slab ids[i] of `cache` [slots][slab]; SCATTER: cache[ids[i]] = rows[i], else rows[i] = cache[ids[i]].  A pure HBM copy:
// blockIdx.y is the row, the threads of a block walk the slab in consecutive V-sized words (V = uint4 whenever the slab and
// both bases are 16-byte multiples: one 1 KiB contiguous run per wave and instruction).  An id outside [0, slots) moves
// nothing (gather: the row is zero-filled), so the kernel stays in bounds whatever the table holds.
template <typename V, bool SCATTER>
__global__ void slab_copy_kernel(V* __restrict__ cache, V* __restrict__ rows, const int* __restrict__ ids, int slots,
                                 long long words) {
    const int i = blockIdx.y;
    const int id = ids[i];
    const bool ok = id >= 0 && id < slots;
    if (SCATTER && !ok) return;
    V* r = rows + (long long)i * words;
    V* c = cache + (long long)(ok ? id : 0) * words;
    const long long step = (long long)gridDim.x * blockDim.x;
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < words; k += step) {
        if (SCATTER) c[k] = r[k];
        else r[k] = ok ? c[k] : V{};
    }
}

template <bool SCATTER>
int slab_copy(const void* cache, const void* rows, const int32_t* ids, int32_t n, int32_t slots, int64_t slab_bytes, void* stream,
              const char* what) {
    E2_REQUIRE(cache && rows && ids && n > 0 && n <= 65535 && slots > 0 && slab_bytes > 0, E2FGVI_EINVAL, "%s: bad arguments", what);
    E2_REQUIRE(slab_bytes % 4 == 0, E2FGVI_EINVAL, "%s: slabs must be whole 32-bit words, got %lld bytes", what, (long long)slab_bytes);
    const unsigned long long align = (unsigned long long)(uintptr_t)cache | (unsigned long long)(uintptr_t)rows |
                                     (unsigned long long)slab_bytes;
    E2_REQUIRE(align % 4 == 0, E2FGVI_EINVAL, "%s: buffers must be 4-byte aligned", what);
    const int vec = align % 16 == 0 ? 16 : (align % 8 == 0 ? 8 : 4);
    const long long words = slab_bytes / vec;
    // enough blocks per slab to fill the chip with a few rows, at most 4 words per thread and launch dimension
    long long bx = (words + NTH * 4 - 1) / (NTH * 4);
    bx = bx < 1 ? 1 : (bx > 4096 ? 4096 : bx);
    const dim3 grid((unsigned)bx, (unsigned)n);
    if (vec == 16)
        hipLaunchKernelGGL((slab_copy_kernel<uint4, SCATTER>), grid, dim3(NTH), 0, (hipStream_t)stream, (uint4*)cache, (uint4*)rows, ids,
                           slots, words);
    else if (vec == 8)
        hipLaunchKernelGGL((slab_copy_kernel<uint2, SCATTER>), grid, dim3(NTH), 0, (hipStream_t)stream, (uint2*)cache, (uint2*)rows, ids,
                           slots, words);
    else
        hipLaunchKernelGGL((slab_copy_kernel<unsigned, SCATTER>), grid, dim3(NTH), 0, (hipStream_t)stream, (unsigned*)cache,
                           (unsigned*)rows, ids, slots, words);
    return 0;
}

// Paste-back at source resolution (what a front end does after test.py:168-179 when the frames were resized on the way in):
//   out = where(NEAREST(mask_lo) != 0, BICUBIC(lo), src)
// with Pillow's two 8-bit passes for the upscale -- width first, its uint8 result clamped, then height -- and Pillow's NEAREST
// tables for the mask, fused: nothing of source size is written but `out`.  A workgroup owns an RT_W x RT_H tile of output pixels
// of one frame (384-byte row segments: three 128-byte lines when the row pitch allows it).  It gathers the tile's mask bits
// first; the OR over the block decides, block-uniformly, between
//   * no hole pixel: the tile's row segments are copied src -> out with the widest words the two addresses share (16 bytes with
//     byte head / tail when both have the same phase, as slab_copy chooses per buffer), 32 lanes per row;
//   * otherwise: the rows / columns of `lo` the tile's taps reach (block min / max of the clipped bounds) are staged in LDS, the
//     horizontal pass of those rows runs LDS -> LDS (uint8, clamped, the intermediate Pillow keeps), and every thread does the
//     vertical pass for four output bytes and selects per pixel between it and src.  For an upscale the patch is smaller than
//     the tile (<= RT_H / scale + 4 rows).  A patch beyond the fixed LDS budget (a strongly shrinking axis) takes the direct
//     path: the same arithmetic with the horizontal values recomputed from global memory per vertical tap.
// Every table entry is clipped before it is used as an index, so the kernel stays in bounds whatever the tables hold.
// With a box (left, upper, Bw, Bh) inside the frame the paste is confined to it: the tables index box-relative pixels (ytab / by /
// cy have Bh entries, xtab / bx / cx have Bw), the grid stays tiled on the full frame, a pixel outside the box counts as "no hole"
// and takes src -- so a tile wholly outside the box is a copied tile.  The whole frame is the box (0, 0, W, H).
// BLEND (inpaint_video(region="track"): two windows of one frame have different boxes, so their results meet at source size):
// lo / mask hold n frames of a window, frame i belongs to frame ids[i] of the Lsrc frames of src and acc (an id outside
// [0, Lsrc) is skipped), and the pasted frame img -- the same arithmetic, to the byte -- goes into the fp32 accumulator like
// test.py:175-179 blends windows:  acc = first[i] ? img : acc * 0.5f + img * 0.5f.  Only the pixels of the `touch` rectangle
// (tl, tu, Tw, Th), which contains the box, are written, and the grid covers only the tiles that rectangle reaches (the tile
// grid stays aligned to the frame: tile (tx0 + blockIdx.x, ty0 + blockIdx.y)); between the box and the rim of touch img is src.
constexpr int RT_W = 128, RT_H = 8, RT_WB = RT_W * 3;
constexpr int RT_ROWS = 24;                    // horizontal-pass rows kept in LDS (RT_ROWS * RT_WB bytes)
constexpr int RT_PATCH = 8192;                 // bytes of `lo` staged in LDS
static_assert(NTH == RT_H * 32, "the copy path gives every tile row 32 lanes");

__device__ __forceinline__ void clipped_taps(const int* __restrict__ bounds, int o, int n_in, int ksize, int& first, int& taps) {
    first = bounds[2 * o];
    first = first < 0 ? 0 : (first > n_in ? n_in : first);
    taps = bounds[2 * o + 1];
    taps = taps < ksize ? taps : ksize;
    taps = taps < n_in - first ? taps : n_in - first;
}

__device__ __forceinline__ unsigned char pillow_clip8(int acc) {
    acc >>= 22;
    return (unsigned char)(acc < 0 ? 0 : (acc > 255 ? 255 : acc));
}

template <typename V>
__device__ __forceinline__ void copy_segment(const unsigned char* __restrict__ s, unsigned char* __restrict__ d, int n, int lane,
                                             int lanes) {
    constexpr int B = (int)sizeof(V);
    int head = (int)((B - (int)((uintptr_t)d & (B - 1))) & (B - 1));
    head = head < n ? head : n;
    const int body = (n - head) / B, t0 = head + body * B;
    for (int k = lane; k < head; k += lanes) d[k] = s[k];
    const V* sv = reinterpret_cast<const V*>(s + head);
    V* dv = reinterpret_cast<V*>(d + head);
    for (int k = lane; k < body; k += lanes) dv[k] = sv[k];
    for (int k = t0 + lane; k < n; k += lanes) d[k] = s[k];
}

// horizontal pass of one value straight from global memory (the direct path)
__device__ __forceinline__ int restore_hpass_global(const unsigned char* __restrict__ lo_row, int w, const int* __restrict__ bx,
                                                    const int* __restrict__ cx, int kx, int x, int c) {
    int f, n;
    clipped_taps(bx, x, w, kx, f, n);
    const int* k = cx + (long long)x * kx;
    const unsigned char* p = lo_row + (long long)f * 3 + c;
    int acc = 1 << 21;
#pragma unroll 1
    for (int j = 0; j < n; ++j) acc += (int)p[3 * j] * k[j];
    return pillow_clip8(acc);
}

struct RestoreTouch { int tl, tu, Tw, Th; };

__device__ __forceinline__ float blend_half(float a, float v, bool is_first) { return is_first ? v : a * 0.5f + v * 0.5f; }

// FEATHER (radius R >= 1): s_c holds c(p) of every tile pixel (0 outside the box) in place of the mask bits; the vertical pass
// runs where c > 0 and its value `up` is ramped into src:  (c up + (n - c) src + n / 2) / n,  n = nx ny from the window's extent
// clipped to the box.  c == n (every pixel of the pasted mask) keeps `up` itself.
template <bool STAGED, bool BLEND, bool FEATHER>
__device__ __forceinline__ void restore_vpass(const unsigned char* __restrict__ lo_l, const unsigned char* __restrict__ src,
                                              unsigned char* __restrict__ out, float* __restrict__ accum, bool is_first, RestoreTouch t,
                                              const unsigned char* s_m, const unsigned short* s_c, int R, const unsigned char* s_h,
                                              int r0, long long frame_off, int h, int w, int W, int x0, int y0, int nb, int th,
                                              int left, int upper, int Bw, int Bh, const int* __restrict__ bx, const int* __restrict__ cx,
                                              int kx, const int* __restrict__ by, const int* __restrict__ cy, int ky) {
    for (int u = threadIdx.x; u < th * (RT_WB / 4); u += NTH) {
        const int ty = u / (RT_WB / 4), xc0 = (u - ty * (RT_WB / 4)) * 4;
        if (xc0 >= nb) continue;
        const int y = y0 + ty;
        const int n4 = nb - xc0 < 4 ? nb - xc0 : 4;
        const long long off = frame_off + ((long long)y * W + x0) * 3 + xc0;
        unsigned char v[4] = {0, 0, 0, 0};
        if (n4 == 4 && ((uintptr_t)(src + off) & 3) == 0) {
            const unsigned q = *reinterpret_cast<const unsigned*>(src + off);
            v[0] = (unsigned char)q; v[1] = (unsigned char)(q >> 8); v[2] = (unsigned char)(q >> 16); v[3] = (unsigned char)(q >> 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n4) v[k] = src[off + k];
        }
        const bool inside = y >= upper && y - upper < Bh;      // a row outside the box has no hole pixel (s_m): no taps are read
        const int iy = inside ? y - upper : 0;
        int fy = 0, ny = 0;
        if (inside) clipped_taps(by, iy, h, ky, fy, ny);
        const int* kyp = cy + (long long)iy * ky;
        const int wy = FEATHER ? (iy + R < Bh - 1 ? iy + R : Bh - 1) - (iy > R ? iy - R : 0) + 1 : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xc = xc0 + k, x = xc / 3, c = xc - 3 * x;
            int cnt = 0;
            if constexpr (FEATHER) {
                if (k >= n4 || !(cnt = s_c[ty * RT_W + x])) continue;
            } else {
                if (k >= n4 || !s_m[ty * RT_W + x]) continue;
            }
            int acc = 1 << 21;
#pragma unroll 1
            for (int j = 0; j < ny; ++j) {
                const int r = fy + j;
                const int hv = STAGED ? (int)s_h[(r - r0) * RT_WB + xc]
                                      : restore_hpass_global(lo_l + (long long)r * w * 3, w, bx, cx, kx, x0 + x - left, c);
                acc += hv * kyp[j];
            }
            if constexpr (FEATHER) {
                const int ix = x0 + x - left;                      // c > 0 only inside the box
                const int n = wy * ((ix + R < Bw - 1 ? ix + R : Bw - 1) - (ix > R ? ix - R : 0) + 1);
                const int up = pillow_clip8(acc);
                v[k] = cnt >= n ? (unsigned char)up : (unsigned char)((cnt * up + (n - cnt) * (int)v[k] + n / 2) / n);
            } else {
                v[k] = pillow_clip8(acc);
            }
        }
        if constexpr (BLEND) {
            if (y < t.tu || y - t.tu >= t.Th) continue;
            float* a = accum + off;
            const int xa = x0 + xc0 / 3, xb = x0 + (xc0 + n4 - 1) / 3;          // the pixels of the first and the last byte
            if (n4 == 4 && xa >= t.tl && xb - t.tl < t.Tw && ((uintptr_t)a & 15) == 0) {
                float4 q = *reinterpret_cast<float4*>(a);
                q.x = blend_half(q.x, (float)v[0], is_first);
                q.y = blend_half(q.y, (float)v[1], is_first);
                q.z = blend_half(q.z, (float)v[2], is_first);
                q.w = blend_half(q.w, (float)v[3], is_first);
                *reinterpret_cast<float4*>(a) = q;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = x0 + (xc0 + k) / 3;
                    if (k < n4 && x >= t.tl && x - t.tl < t.Tw) a[k] = blend_half(a[k], (float)v[k], is_first);
                }
            }
        } else if (n4 == 4 && ((uintptr_t)(out + off) & 3) == 0) {
            *reinterpret_cast<unsigned*>(out + off) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n4) out[off + k] = v[k];
        }
    }
}

// The feathered paste (inpaint_video(feather=R), 1 <= R <= RF_MAX): inside the box, in box-relative pixels and with everything
// outside the box counting as 0,
//   M = NEAREST(mask),  D = M dilated by the (2R+1)^2 square,  c(p) = #{q in the box : |q - p| <= R, D(q)},  n(p) = #{q in the box :
//   |q - p| <= R},   out = (c BICUBIC(lo) + (n - c) src + n / 2) / n;      out = src outside the box.
// c is non-zero only within 2R of a pasted pixel, so a tile is a copied tile unless M has a pixel within 2R of it.  The NEAREST
// tables are monotone: the tile and its 2R halo, clipped to the box, read one rectangle of the low-resolution mask,
// ytab[first] .. ytab[last] x xtab[first] .. xtab[last].  That rectangle is staged in LDS and ORed for the block-uniform decision (for
// a shrinking axis the rectangle holds pixels no output reads: such a tile blends, finds c == 0 and writes src); only a tile that
// goes on expands it to M at source resolution -- and not even that when the rectangle holds nothing but hole pixels: c = n on the
// whole tile then.  A rectangle beyond the LDS buffer (an axis that shrinks, or keeps its size at a
// large R) is not staged: M is gathered through the tables straight away and ORed itself -- a bounded cost for any tables.
// Then four separable passes of sliding window sums over 2R + 1 entries, LDS -> LDS with a barrier after each:
//   M [RT_H + 4R][RT_W + 4R] -rows, > 0-> [RT_H + 4R][RT_W + 2R] -columns, > 0, inside the box-> D [RT_H + 2R][RT_W + 2R]
//   -rows-> [RT_H + 2R][RT_W] -columns, inside the box-> c [RT_H][RT_W] (uint16: c <= 33^2),
// in two buffers that afterwards hold the lo patch and its horizontal pass.
constexpr int RF_MAX = 16;                                       // video.FEATHER_MAX
constexpr int RF_W2 = RT_W + 4 * RF_MAX, RF_H2 = RT_H + 4 * RF_MAX, RF_W1 = RT_W + 2 * RF_MAX;
constexpr int RF_BUF0 = RF_H2 * RF_W2, RF_BUF1 = RF_H2 * RF_W1;
static_assert(RF_BUF0 >= RT_PATCH && RF_BUF1 >= RT_ROWS * RT_WB, "the window buffers are reused for the lo patch and its horizontal pass");
static_assert(RF_BUF0 % 16 == 0 && RF_BUF1 % 16 == 0, "the buffers follow each other 16-byte aligned");
static_assert(RF_W2 <= NTH, "a thread per column of the halo");

// out[line][o] = fin(in[line][o] + ... + in[line][o + 2R], line, o) for o < n_out (ROWS), or the same along the columns of `in`
// (line = column); a thread slides the window over RF_SEG consecutive outputs of one line
constexpr int RF_SEG = 8;
template <bool ROWS, typename T, typename F>
__device__ __forceinline__ void window_sums(const unsigned char* in, int ipitch, T* out, int opitch, int lines, int n_out, int R, F fin) {
    const int nseg = (n_out + RF_SEG - 1) / RF_SEG;
    const int istep = ROWS ? 1 : ipitch, ostep = ROWS ? 1 : opitch;
    for (int it = threadIdx.x; it < lines * nseg; it += NTH) {
        const int line = ROWS ? it / nseg : it % lines;
        const int o0 = (ROWS ? it % nseg : it / lines) * RF_SEG;
        const unsigned char* p = in + (ROWS ? line * ipitch + o0 : o0 * ipitch + line);
        T* q = out + (ROWS ? line * opitch + o0 : o0 * opitch + line);
        const int n = n_out - o0 < RF_SEG ? n_out - o0 : RF_SEG;
        int s = 0;
        for (int k = 0; k <= 2 * R; ++k) s += p[k * istep];
        q[0] = fin(s, line, o0);
        for (int t = 1; t < n; ++t) {
            s += (int)p[(t + 2 * R) * istep] - (int)p[(t - 1) * istep];
            q[t * ostep] = fin(s, line, o0 + t);
        }
    }
}

// the clipped NEAREST table entries of the tile's halo, W2 columns from x0 - 2R and H2 rows from y0 - 2R; -1 outside the box
__device__ __forceinline__ void feather_tables(int* s_xt, int* s_yt, const int* __restrict__ xtab, const int* __restrict__ ytab, int x0,
                                               int y0, int R, int left, int upper, int Bw, int Bh, int w, int h) {
    for (int i = threadIdx.x; i < RT_W + 4 * R; i += NTH) {
        const int ix = x0 - 2 * R + i - left;
        int mx = -1;
        if (ix >= 0 && ix < Bw) { mx = xtab[ix]; mx = mx < 0 ? 0 : (mx > w - 1 ? w - 1 : mx); }
        s_xt[i] = mx;
    }
    for (int i = threadIdx.x; i < RT_H + 4 * R; i += NTH) {
        const int iy = y0 - 2 * R + i - upper;
        int my = -1;
        if (iy >= 0 && iy < Bh) { my = ytab[iy]; my = my < 0 ? 0 : (my > h - 1 ? h - 1 : my); }
        s_yt[i] = my;
    }
    __syncthreads();
}

template <bool BLEND, bool FEATHER>
__global__ __launch_bounds__(NTH) void restore_u8_kernel(
    const unsigned char* __restrict__ lo, const unsigned char* __restrict__ mask, const unsigned char* __restrict__ src,
    unsigned char* __restrict__ out, float* __restrict__ accum, const int* __restrict__ ids, const unsigned char* __restrict__ first,
    int Lsrc, int tx0, int ty0, RestoreTouch touch, int L, int h, int w, int H, int W, int left, int upper, int Bw, int Bh,
    const int* __restrict__ ytab, const int* __restrict__ xtab, const int* __restrict__ bx, const int* __restrict__ cx, int kx,
    const int* __restrict__ by, const int* __restrict__ cy, int ky, int R) {
    // an instantiation keeps the arrays of its own path: s_m, s_patch, s_h, or with FEATHER the window buffers, s_c and the tables
    __shared__ unsigned char s_m[RT_H * RT_W];
    __shared__ __align__(16) unsigned char s_patch[RT_PATCH];
    __shared__ __align__(16) unsigned char s_h[RT_ROWS * RT_WB];
    __shared__ int s_rng[4];
    __shared__ __align__(16) unsigned char s_buf0[RF_BUF0];
    __shared__ __align__(16) unsigned char s_buf1[RF_BUF1];
    __shared__ unsigned short s_c[RT_H * RT_W];
    __shared__ int s_xt[RF_W2], s_yt[RF_H2];
    const int tid = threadIdx.x;
    const int x0 = (tx0 + (int)blockIdx.x) * RT_W, y0 = (ty0 + (int)blockIdx.y) * RT_H;
    const int tw = W - x0 < RT_W ? W - x0 : RT_W, th = H - y0 < RT_H ? H - y0 : RT_H;
    const int nb = tw * 3;
    if (tw <= 0 || th <= 0) return;
    // FEATHER: the tile with its 2R halo is W2 x H2 pixels from (x0 - 2R, y0 - 2R)
    const int W2 = RT_W + 4 * R, H2 = RT_H + 4 * R, W1 = RT_W + 2 * R, H1 = RT_H + 2 * R;
    int rx0 = 0, ry0 = 0, rw = 0, rh = 0;
    if constexpr (FEATHER) {
        // the rectangle of the low-resolution mask between the entries of the halo's first and last column / row inside the box
        const int gx0 = x0 - 2 * R > left ? x0 - 2 * R : left, gx1 = (x0 + RT_W + 2 * R < left + Bw ? x0 + RT_W + 2 * R : left + Bw) - 1;
        const int gy0 = y0 - 2 * R > upper ? y0 - 2 * R : upper, gy1 = (y0 + RT_H + 2 * R < upper + Bh ? y0 + RT_H + 2 * R : upper + Bh) - 1;
        if (gx0 <= gx1 && gy0 <= gy1) {
            int a = xtab[gx0 - left], b = xtab[gx1 - left];
            a = a < 0 ? 0 : (a > w - 1 ? w - 1 : a);
            b = b < 0 ? 0 : (b > w - 1 ? w - 1 : b);
            rx0 = a < b ? a : b;
            rw = (a < b ? b : a) - rx0 + 1;
            a = ytab[gy0 - upper], b = ytab[gy1 - upper];
            a = a < 0 ? 0 : (a > h - 1 ? h - 1 : a);
            b = b < 0 ? 0 : (b > h - 1 ? h - 1 : b);
            ry0 = a < b ? a : b;
            rh = (a < b ? b : a) - ry0 + 1;
        }
    }
    const bool staged = (long long)rw * rh <= RF_BUF1;     // a halo with no pixel in the box: a staged rectangle of 0 bytes
    // a copied tile with a staged rectangle never reads the halo's table entries: they wait for the first tile that goes on
    bool tabs = false;
    if (FEATHER && !staged) {
        feather_tables(s_xt, s_yt, xtab, ytab, x0, y0, R, left, upper, Bw, Bh, w, h);
        tabs = true;
    }
    for (int l = blockIdx.z; l < L; l += gridDim.z) {
        const int fr = BLEND ? ids[l] : l;               // the frame of src / out / accum; block-uniform
        if (BLEND && (fr < 0 || fr >= Lsrc)) continue;
        const bool is_first = BLEND ? first[l] != 0 : true;
        // the tile's mask bits through the two NEAREST tables; any hole pixel?
        const unsigned char* ml = mask + (long long)l * h * w;
        int any = 0, all = 1;
        if constexpr (FEATHER) {
            // ... any hole pixel within 2R of the tile?  nothing but hole pixels?
            if (staged) {
                for (int i = tid; i < rw * rh; i += NTH) {
                    const int r = i / rw;
                    const unsigned char m = ml[(long long)(ry0 + r) * w + rx0 + (i - r * rw)] != 0;
                    s_buf1[i] = m;
                    any |= m;
                    all &= m;
                }
            } else if (tid < W2) {                      // a thread per column of the halo
                const int mx = s_xt[tid];
                for (int row = 0; row < H2; ++row) {
                    const int my = s_yt[row];
                    const bool in = my >= 0 && mx >= 0;
                    const unsigned char m = in ? ml[(long long)my * w + mx] != 0 : 0;
                    s_buf0[row * W2 + tid] = m;
                    any |= m;
                    all &= m | !in;
                }
            }
        } else {
            for (int i = tid; i < RT_H * RT_W; i += NTH) {
                const int ty = i / RT_W, tx = i % RT_W;
                unsigned char m = 0;
                const int iy = y0 + ty - upper, ix = x0 + tx - left;
                if (ty < th && tx < tw && iy >= 0 && iy < Bh && ix >= 0 && ix < Bw) {
                    int my = ytab[iy], mx = xtab[ix];
                    my = my < 0 ? 0 : (my > h - 1 ? h - 1 : my);
                    mx = mx < 0 ? 0 : (mx > w - 1 ? w - 1 : mx);
                    m = ml[(long long)my * w + mx] != 0;
                }
                s_m[i] = m;
                any |= m;
            }
        }
        any = __syncthreads_or(any);
        const long long frame_off = (long long)fr * H * W * 3;
        if (!any) {
            const int ty = tid >> 5, lane = tid & 31;
            if (BLEND) {
                // img is src: 32 lanes along a row's bytes, consecutive floats of acc
                const int y = y0 + ty;
                if (ty < th && y >= touch.tu && y - touch.tu < touch.Th) {
                    const long long off = frame_off + ((long long)y * W + x0) * 3;
                    for (int k = lane; k < nb; k += 32) {
                        const int x = x0 + k / 3;
                        if (x >= touch.tl && x - touch.tl < touch.Tw) accum[off + k] = blend_half(accum[off + k], (float)src[off + k], is_first);
                    }
                }
            } else if (ty < th) {
                const long long off = frame_off + ((long long)(y0 + ty) * W + x0) * 3;
                const unsigned char* s = src + off;
                unsigned char* d = out + off;
                const unsigned phase = (unsigned)((uintptr_t)s ^ (uintptr_t)d);
                if ((phase & 15) == 0) copy_segment<uint4>(s, d, nb, lane, 32);
                else if ((phase & 3) == 0) copy_segment<unsigned>(s, d, nb, lane, 32);
                else copy_segment<unsigned char>(s, d, nb, lane, 32);
            }
            continue;                                   // s_m is not read on this path: the next frame may overwrite it
        }
        if (FEATHER && __syncthreads_and(all)) {
            // every pixel of the halo inside the box is a hole pixel, so D = 1 and c = n on the tile: no window passes
            for (int i = tid; i < RT_H * RT_W; i += NTH) {
                const int ix = x0 + i % RT_W - left, iy = y0 + i / RT_W - upper;
                s_c[i] = (ix >= 0 && ix < Bw && iy >= 0 && iy < Bh) ? 0xffff : 0;
            }
            __syncthreads();
        } else if constexpr (FEATHER) {
            if (staged) {
                if (!tabs) {
                    feather_tables(s_xt, s_yt, xtab, ytab, x0, y0, R, left, upper, Bw, Bh, w, h);
                    tabs = true;
                }
                if (tid < W2) {                         // a thread per column of the halo
                    const int mx = s_xt[tid], rx = mx - rx0;
                    const bool okx = mx >= 0 && rx >= 0 && rx < rw;     // tables that are not monotone may leave the rectangle: 0 then
                    for (int row = 0; row < H2; ++row) {
                        const int my = s_yt[row], ry = my - ry0;
                        s_buf0[row * W2 + tid] = (okx && my >= 0 && ry >= 0 && ry < rh) ? s_buf1[ry * rw + rx] : 0;
                    }
                }
                __syncthreads();
            }
            window_sums<true>(s_buf0, W2, s_buf1, W1, H2, W1, R, [](int s, int, int) { return (unsigned char)(s > 0); });
            __syncthreads();
            window_sums<false>(s_buf1, W1, s_buf0, W1, W1, H1, R, [=](int s, int col, int row) {
                const int ix = x0 - R + col - left, iy = y0 - R + row - upper;
                return (unsigned char)(s > 0 && ix >= 0 && ix < Bw && iy >= 0 && iy < Bh);
            });
            __syncthreads();
            window_sums<true>(s_buf0, W1, s_buf1, RT_W, H1, RT_W, R, [](int s, int, int) { return (unsigned char)s; });
            __syncthreads();
            window_sums<false>(s_buf1, RT_W, s_c, RT_W, RT_W, RT_H, R, [=](int s, int col, int row) {
                const int ix = x0 + col - left, iy = y0 + row - upper;
                return (unsigned short)((ix >= 0 && ix < Bw && iy >= 0 && iy < Bh) ? s : 0);
            });
            __syncthreads();                            // the two buffers are free: the lo patch and its horizontal pass go there
        }
        unsigned char* const s_patch_ = FEATHER ? s_buf0 : s_patch;
        unsigned char* const s_h_ = FEATHER ? s_buf1 : s_h;
        // rows [r0, r1) and columns [c0, c1) of lo that the tile's taps reach
        if (tid < 4) s_rng[tid] = (tid & 1) ? 0 : 0x7fffffff;
        __syncthreads();
        if (tid < th && y0 + tid >= upper && y0 + tid < upper + Bh) {
            int f, n;
            clipped_taps(by, y0 + tid - upper, h, ky, f, n);
            if (n > 0) { atomicMin(&s_rng[0], f); atomicMax(&s_rng[1], f + n); }
        }
        if (tid < tw && x0 + tid >= left && x0 + tid < left + Bw) {
            int f, n;
            clipped_taps(bx, x0 + tid - left, w, kx, f, n);
            if (n > 0) { atomicMin(&s_rng[2], f); atomicMax(&s_rng[3], f + n); }
        }
        __syncthreads();
        int r0 = s_rng[0], c0 = s_rng[2];
        const int pr = s_rng[1] > r0 ? s_rng[1] - r0 : 0, pc = s_rng[3] > c0 ? s_rng[3] - c0 : 0;
        if (!pr) r0 = 0;
        if (!pc) c0 = 0;
        const unsigned char* lo_l = lo + (long long)l * h * w * 3;
        if (pr <= RT_ROWS && (long long)pr * pc * 3 <= RT_PATCH) {
            const int pb = pc * 3;
            for (int i = tid; i < pr * pb; i += NTH) {
                const int r = i / pb;
                s_patch_[i] = lo_l[((long long)(r0 + r) * w + c0) * 3 + (i - r * pb)];
            }
            __syncthreads();
            for (int i = tid; i < pr * nb; i += NTH) {
                const int r = i / nb, xc = i - r * nb, x = xc / 3, c = xc - 3 * x;
                const int ix = x0 + x - left;
                if (ix < 0 || ix >= Bw) continue;       // a column outside the box: no hole pixel reads its s_h
                int f, n;
                clipped_taps(bx, ix, w, kx, f, n);
                const int* k = cx + (long long)ix * kx;
                const unsigned char* p = s_patch_ + r * pb + (f - c0) * 3 + c;        // n > 0 implies c0 <= f, f + n <= c0 + pc
                int acc = 1 << 21;
#pragma unroll 1
                for (int j = 0; j < n; ++j) acc += (int)p[3 * j] * k[j];
                s_h_[r * RT_WB + xc] = pillow_clip8(acc);
            }
            __syncthreads();
            restore_vpass<true, BLEND, FEATHER>(lo_l, src, out, accum, is_first, touch, s_m, s_c, R, s_h_, r0, frame_off, h, w, W, x0, y0, nb, th,
                                                left, upper, Bw, Bh, bx, cx, kx, by, cy, ky);
        } else {
            restore_vpass<false, BLEND, FEATHER>(lo_l, src, out, accum, is_first, touch, s_m, s_c, R, s_h_, r0, frame_off, h, w, W, x0, y0, nb, th,
                                                 left, upper, Bw, Bh, bx, cx, kx, by, cy, ky);
        }
        __syncthreads();                                // s_m, s_h are rewritten for the next frame
    }
}

// Bounding box of the hole over a whole video (the crop region of video.hole_region): masks uint8 [L,Hm,Wm], any non-zero byte
// is hole; box = (x0, y0, x1, y1), upper ends exclusive, starts at (0x7f7f7f7f, 0x7f7f7f7f, 0, 0) -- empty: x1 <= x0.  One pass,
// HBM-bound: a wave owns a mask row at a time (rows = L * Hm, grid-strided) and reads it as 16-byte words between a byte head up
// to the row's first 16-byte boundary and a byte tail (any pitch, any base), first / last non-zero byte of a word by ffs / clz;
// the lanes' boxes are reduced within the wave (wave64 shuffles), the waves' within the block through LDS, and a block that saw
// a hole pixel issues the four global atomicMin / atomicMax -- a block that saw none issues nothing.
// blockIdx.y picks one of several boxes, each over its own `rows` consecutive mask rows: one box over the L * Hm rows of the video
// (hole_bbox), or a box per frame over its Hm rows (hole_bbox_frames, the per-window regions of video.plan_track).
constexpr int BB_WAVES = NTH / 64;

__global__ void bbox_init_kernel(int* __restrict__ box, long long n) {
    E2_GRID_STRIDE(idx, n) box[idx] = (idx & 3) < 2 ? 0x7f7f7f7f : 0;
}

__device__ __forceinline__ void bbox_word(unsigned v, int x, int& lo, int& hi) {
    if (v) {
        const int a = x + ((__ffs((int)v) - 1) >> 3), b = x + ((31 - __clz((int)v)) >> 3) + 1;      // little endian: byte 0 is the lowest address
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
}

__global__ __launch_bounds__(NTH) void hole_bbox_kernel(const unsigned char* __restrict__ m, long long rows, int Hm, int Wm,
                                                        int* __restrict__ box) {
    __shared__ int s_box[BB_WAVES][4];
    m += (long long)blockIdx.y * rows * Wm;
    box += 4 * (long long)blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = 0, y1 = 0;
    const long long step = (long long)gridDim.x * BB_WAVES;
    for (long long r = (long long)blockIdx.x * BB_WAVES + wave; r < rows; r += step) {
        const unsigned char* p = m + r * Wm;
        int head = (int)((16 - (int)((uintptr_t)p & 15)) & 15);
        head = head < Wm ? head : Wm;
        const int body = (Wm - head) / 16, t0 = head + body * 16;
        int lo = 0x7fffffff, hi = 0;
        for (int k = lane; k < head; k += 64)
            if (p[k]) { lo = k < lo ? k : lo; hi = k + 1; }
        const uint4* pv = reinterpret_cast<const uint4*>(p + head);
        for (int k = lane; k < body; k += 64) {
            const uint4 v = pv[k];
            const int x = head + 16 * k;
            bbox_word(v.x, x, lo, hi);
            bbox_word(v.y, x + 4, lo, hi);
            bbox_word(v.z, x + 8, lo, hi);
            bbox_word(v.w, x + 12, lo, hi);
        }
        for (int k = t0 + lane; k < Wm; k += 64)
            if (p[k]) { lo = k < lo ? k : lo; hi = k + 1; }
        if (hi > lo) {
            const int y = (int)(r % Hm);
            x0 = lo < x0 ? lo : x0;
            x1 = hi > x1 ? hi : x1;
            y0 = y < y0 ? y : y0;
            y1 = y + 1 > y1 ? y + 1 : y1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(x0, o, 64), b = __shfl_xor(y0, o, 64), c = __shfl_xor(x1, o, 64), d = __shfl_xor(y1, o, 64);
        x0 = a < x0 ? a : x0;
        y0 = b < y0 ? b : y0;
        x1 = c > x1 ? c : x1;
        y1 = d > y1 ? d : y1;
    }
    if (lane == 0) { s_box[wave][0] = x0; s_box[wave][1] = y0; s_box[wave][2] = x1; s_box[wave][3] = y1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < BB_WAVES; ++i) {
            x0 = s_box[i][0] < x0 ? s_box[i][0] : x0;
            y0 = s_box[i][1] < y0 ? s_box[i][1] : y0;
            x1 = s_box[i][2] > x1 ? s_box[i][2] : x1;
            y1 = s_box[i][3] > y1 ? s_box[i][3] : y1;
        }
        if (x1 > x0) {
            atomicMin(box, x0);
            atomicMin(box + 1, y0);
            atomicMax(box + 2, x1);
            atomicMax(box + 3, y1);
        }
    }
}

// Scene cuts (video.detect_cuts): block-histogram difference of adjacent frames, integers only.  For a pixel (x, y) of frame t with
// bytes R, G, B:  Y = (77 R + 150 G + 29 B + 128) >> 8,  bin = Y >> 2 (64 bins),  cell = ((4 y) / H) * 4 + (4 x) / W (a 4 x 4 grid);
// hist[t][cell][bin] counts pixels and  out[t] = sum over cell, bin of |hist[t] - hist[t + 1]|,  0 <= t < L - 1.
// Pass 1, HBM-bound: a workgroup owns a strip of whole rows inside ONE cell row of one frame -- contiguous bytes, and only the
// 4 x 64 counters of that cell row.  The strip is read in 48-byte chunks (16 pixels) from the first 16-byte boundary on: three
// 16-byte loads and the dword behind them, shifted by the strip's pixel phase (the boundary falls 0, 1 or 2 bytes into a pixel;
// 48 is a multiple of 3, so every chunk has the same phase); the pixels in front of the first chunk and behind the last one that
// lies wholly inside the strip are read byte by byte.  Nothing outside the strip's own bytes is read, whatever the base and
// the row pitch.  A thread merges runs of equal counters among its 16 consecutive pixels in registers (a constant frame: one LDS
// add of 16 per chunk), and the LDS counters exist SD_REP times, picked by lane: on a smooth image the 64 lanes of an add meet
// on one counter 64 / SD_REP at a time instead of all at once.  The strip's non-zero counters then go to the frame's table with
// integer global atomics -- sums of integers, the same in any arrival order; the entry zeroes the table in front of the launch.
// Pass 2: a workgroup per pair of frames sums the 1024 absolute differences.
constexpr int SD_CELLS = 16, SD_BINS = 64, SD_TABLE = SD_CELLS * SD_BINS;      // counters per frame
constexpr int SD_ROW = 4 * SD_BINS;                                           // counters per cell row
constexpr int SD_REP = 8;
constexpr int SD_STRIP = 32768;                                               // bytes a workgroup aims for
static_assert(SD_ROW == NTH, "a thread per counter of the cell row");

// the top six bits of the luma
__device__ __forceinline__ int sd_bin(unsigned r, unsigned g, unsigned b) { return fb_luma(r, g, b) >> 2; }

// first row of cell row c: the smallest y with (4 y) / H >= c
__host__ __device__ inline int sd_row0(int c, int H) { return (int)(((long long)c * H + 3) / 4); }

struct SdRun {
    int cur, cnt;
    __device__ __forceinline__ void add(unsigned* s, int idx) {
        if (idx == cur) { ++cnt; return; }
        if (cnt) atomicAdd(s + cur * SD_REP, (unsigned)cnt);
        cur = idx;
        cnt = 1;
    }
};

__global__ __launch_bounds__(NTH) void scene_hist_kernel(const unsigned char* __restrict__ frames, unsigned* __restrict__ hist, int H,
                                                         int W, int rows_per_strip, int nstrips) {
    __shared__ unsigned s_hist[SD_ROW * SD_REP];
    const int tid = threadIdx.x;
    const int cy = blockIdx.x / nstrips, strip = blockIdx.x - cy * nstrips;
    const long long ya = (long long)sd_row0(cy, H) + (long long)strip * rows_per_strip;
    long long yb = ya + rows_per_strip;
    yb = yb < sd_row0(cy + 1, H) ? yb : sd_row0(cy + 1, H);
    if (ya >= yb) return;                               // block-uniform: an empty cell row (H < 4) or a strip past its end
    for (int i = tid; i < SD_ROW * SD_REP; i += NTH) s_hist[i] = 0;
    __syncthreads();
    const long long t = blockIdx.y;
    const unsigned char* p = frames + (t * H + ya) * W * 3;
    const unsigned npix = (unsigned)((yb - ya) * W);    // < 2^32: a strip is a single row, or at most SD_STRIP bytes and a row
    const long long nbytes = 3LL * npix;
    const int c1 = (int)((1LL * W + 3) / 4), c2 = (int)((2LL * W + 3) / 4), c3 = (int)((3LL * W + 3) / 4);  // first column of cell columns 1, 2, 3
    unsigned* const mine = s_hist + (tid & (SD_REP - 1));
    // the 48-byte chunks: from the first 16-byte boundary, as many as lie inside the strip with the dword behind them
    const int head = (int)((16 - (int)((uintptr_t)p & 15)) & 15);
    const int shift = (3 - head % 3) % 3;               // bytes of the chunk in front of its first whole pixel
    const unsigned nchunks = nbytes - head >= 52 ? (unsigned)((nbytes - head - 52) / 48 + 1) : 0u;
    const unsigned pfirst = nchunks ? (unsigned)(head + shift) / 3u : npix;    // the pixels in front of the chunks: byte by byte
    const unsigned ptail = nchunks ? pfirst + 16u * nchunks : npix;
    for (unsigned k = tid; k < nchunks; k += NTH) {
        const unsigned char* q = p + head + 48LL * k;
        const uint4 a = *reinterpret_cast<const uint4*>(q), b = *reinterpret_cast<const uint4*>(q + 16),
                    c = *reinterpret_cast<const uint4*>(q + 32);
        const unsigned e = *reinterpret_cast<const unsigned*>(q + 48);
        unsigned w[13] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, e};
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], (unsigned)shift);
        int x = (int)((pfirst + 16u * k) % (unsigned)W);
        SdRun run{-1, 0};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const unsigned d0 = w[3 * g], d1 = w[3 * g + 1], d2 = w[3 * g + 2];
            const int bins[4] = {sd_bin(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u), sd_bin(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u),
                                 sd_bin((d1 >> 16) & 255u, d1 >> 24, d2 & 255u), sd_bin((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cx = (x >= c1) + (x >= c2) + (x >= c3);
                run.add(mine, cx * SD_BINS + bins[j]);
                x = x + 1 == W ? 0 : x + 1;
            }
        }
        atomicAdd(mine + run.cur * SD_REP, (unsigned)run.cnt);
    }
    const unsigned nslow = pfirst + (npix - ptail);
    for (unsigned i = tid; i < nslow; i += NTH) {
        const unsigned px = i < pfirst ? i : ptail + (i - pfirst);
        const int x = (int)(px % (unsigned)W);
        const int cx = (x >= c1) + (x >= c2) + (x >= c3);
        const unsigned char* q = p + 3LL * px;
        atomicAdd(mine + (cx * SD_BINS + sd_bin(q[0], q[1], q[2])) * SD_REP, 1u);
    }
    __syncthreads();
    unsigned n = 0;
#pragma unroll
    for (int r = 0; r < SD_REP; ++r) n += s_hist[tid * SD_REP + r];
    if (n) atomicAdd(hist + t * SD_TABLE + cy * SD_ROW + tid, n);
}

__global__ __launch_bounds__(NTH) void scene_diff_kernel(const unsigned* __restrict__ hist, long long* __restrict__ out) {
    __shared__ long long s_sum[NTH / 64];
    const unsigned* a = hist + (long long)blockIdx.x * SD_TABLE;
    const unsigned* b = a + SD_TABLE;
    long long s = 0;
    for (int i = threadIdx.x; i < SD_TABLE; i += NTH) s += a[i] > b[i] ? a[i] - b[i] : b[i] - a[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < NTH / 64; ++i) s += s_sum[i];
        out[blockIdx.x] = s;
    }
}

// Static overlays (video.overlay_mask): per-pixel sums of the luma gradient over the frames, integers only.  With the scene
// detector's luma Y = (77 R + 150 G + 29 B + 128) >> 8 and clamped borders
//   gx = Y[y][min(x+1, W-1)] - Y[y][max(x-1, 0)],  gy = Y[min(y+1, H-1)][x] - Y[max(y-1, 0)][x]   per frame,
//   stats[0] = Sx = sum gx,  stats[1] = Sy = sum gy,  stats[2] = M = sum (|gx| + |gy|)   over the L frames, int32 [3][H][W].
// One read of the frames: a workgroup owns an OV_TW x OV_TH pixel tile and a chunk of consecutive frames.  Per frame the tile's
// luma with its one-pixel halo goes to LDS as bytes: a work item is four consecutive pixels of a halo row, 12 bytes read with one
// load at whatever alignment the pixels have (no byte outside the frame's row is read); an item that hangs over the frame's left
// or right edge loads the nearest four pixels of its row instead and a byte permute of the four lumas repeats the edge column
// (frames narrower than four pixels have an instantiation of their own that reads byte by byte).  Which item a thread has does
// not depend on the frame, so offsets and permutes are worked out once in front of the frame loop and every load in the loop is
// unconditional: a frame's three loads leave back to back, before the barrier, and are waited for only at the top of the next
// trip, behind the barrier and the sums of this one (the build checks the generated code for that: build.py
// verify_overlay_prefetch).  The luma tile is double buffered (one barrier per frame), and a thread keeps the three sums of its
// eight pixels -- one column, eight rows: a wave stores whole 256-byte rows -- in registers across the chunk.  Chunks of one tile
// meet in the planes with integer global atomic adds (the entry zeroes the planes first); a single chunk stores.  Sums of
// integers: exact in any arrival order.
constexpr int OV_TW = 64, OV_TH = 32;                              // the pixel tile of a workgroup
constexpr int OV_PER = OV_TH / (NTH / OV_TW);                      // rows per thread: 8
constexpr int OV_GROUPS = (OV_TW + 2 + 3) / 4;                     // four-pixel items per halo row: 17
constexpr int OV_ITEMS = ((OV_TH + 2) * OV_GROUPS + NTH - 1) / NTH;  // items per thread: 3
constexpr int OV_PITCH = OV_GROUPS * 4;                            // bytes per luma row in LDS (17 dwords: odd)
constexpr int OV_CHUNK = 8;                                        // ops.OVERLAY_CHUNK: no chunk of frames is shorter (unless L is)
constexpr int OV_BLOCKS = 2048;                                    // workgroups the chunking aims for (8 per CU)
constexpr int OV_LMAX = 1 << 22;                                   // M <= 510 L stays below 2^31
constexpr int OV_RMAX = 16;                                        // ops.OVERLAY_RADIUS_MAX
static_assert(OV_TW == 64 && NTH % OV_TW == 0 && OV_TH % (NTH / OV_TW) == 0, "a lane per tile column");

struct OvRaw { unsigned d0, d1, d2; };                             // four pixels: 12 bytes in memory order

// frames narrower than four pixels (OvItem::narrow): the item's four pixels byte by byte at clamped columns
__device__ __forceinline__ OvRaw ov_load_narrow(const unsigned char* __restrict__ row, int gx0, int W) {
    unsigned b[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int x = gx0 + j;
        x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
        const unsigned char* q = row + 3LL * x;
        b[3 * j] = q[0]; b[3 * j + 1] = q[1]; b[3 * j + 2] = q[2];
    }
    OvRaw v;
    v.d0 = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    v.d1 = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    v.d2 = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    return v;
}

// the four lumas, pixel j in byte j
__device__ __forceinline__ unsigned ov_luma4(const OvRaw& v) {
    const unsigned w[3] = {v.d0, v.d1, v.d2};
    int y[FB_PX];
    fb_luma4(w, y);
    return (unsigned)y[0] | ((unsigned)y[1] << 8) | ((unsigned)y[2] << 16) | ((unsigned)y[3] << 24);
}

template <bool ATOMIC, bool NARROW>
__global__ __launch_bounds__(NTH) void overlay_stats_kernel(const unsigned char* __restrict__ frames, int* __restrict__ stats, int L,
                                                            int H, int W, int ntx) {
    __shared__ unsigned s_y[2][(OV_TH + 2) * OV_GROUPS];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int x0 = tx * OV_TW, y0 = ty * OV_TH;
    const int tw = W - x0 < OV_TW ? W - x0 : OV_TW, th = H - y0 < OV_TH ? H - y0 : OV_TH;   // the tile's pixels inside the frame
    const int ngrp = (tw + 2 + 3) / 4, nitems = (th + 2) * ngrp;   // the halo rows and items this tile needs
    // the chunks split the L frames evenly: chunk c of n takes frames [c L / n, (c + 1) L / n), lengths that differ by one at most
    const int l0 = (int)((long long)blockIdx.y * L / gridDim.y), l1 = (int)(((long long)blockIdx.y + 1) * L / gridDim.y);
    if (l0 >= l1) return;                               // block-uniform; the entry plans no more chunks than frames
    const long long fbytes = 3LL * H * W;
    // this thread's items.  off: the byte in a frame where the item's load starts -- the item's own first pixel, or, for an item
    // that hangs over the frame's left or right edge, the nearest four pixels that lie in its row (W >= 4); sel: which of the four
    // loaded pixels each of the item's pixels is (v_perm_b32 on the four lumas), 0 1 2 3 unless a column was clamped; slot: its
    // dword in LDS.  A thread without a k-th item loads the frame's first four pixels and stores nothing: every load below is
    // unconditional, so the three of a frame leave back to back and nothing waits for them in front of the barrier.
    long long off[OV_ITEMS];
    unsigned sel[OV_ITEMS];
    int gx0[OV_ITEMS], slot[OV_ITEMS];
    bool have[OV_ITEMS];
#pragma unroll
    for (int k = 0; k < OV_ITEMS; ++k) {
        const int i = tid + k * NTH;
        have[k] = i < nitems;
        const int r = have[k] ? i / ngrp : 0, g = have[k] ? i - r * ngrp : 0;
        int yy = have[k] ? y0 - 1 + r : 0;
        yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
        gx0[k] = have[k] ? x0 - 1 + 4 * g : 0;
        slot[k] = r * OV_GROUPS + g;
        off[k] = 3LL * yy * W;
        sel[k] = 0x03020100u;
        if (!NARROW) {
            int w0 = gx0[k] < 0 ? 0 : gx0[k];
            w0 = w0 > W - 4 ? W - 4 : w0;
            off[k] += 3LL * w0;
            sel[k] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int x = gx0[k] + j;
                x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
                sel[k] |= (unsigned)(x - w0) << (8 * j);
            }
        }
    }
    const int lx = tid & (OV_TW - 1), ly0 = (tid / OV_TW) * OV_PER;
    int sx[OV_PER], sy[OV_PER], sm[OV_PER];
#pragma unroll
    for (int i = 0; i < OV_PER; ++i) sx[i] = sy[i] = sm[i] = 0;
    OvRaw raw[OV_ITEMS];
    const unsigned char* f = frames + (long long)l0 * fbytes;
    auto load = [&](int k) {
        if (NARROW) return ov_load_narrow(f + off[k], gx0[k], W);
        OvRaw v;
        __builtin_memcpy(&v, f + off[k], 12);           // one global_load_dwordx3 at any alignment
        return v;
    };
#pragma unroll
    for (int k = 0; k < OV_ITEMS; ++k) raw[k] = load(k);
    for (int l = l0; l < l1; ++l) {
        unsigned* const buf = s_y[(l - l0) & 1];
#pragma unroll
        for (int k = 0; k < OV_ITEMS; ++k) {
            const unsigned y = ov_luma4(raw[k]);
            if (have[k]) buf[slot[k]] = __builtin_amdgcn_perm(y, y, sel[k]);
        }
        if (l + 1 < l1) {                               // block-uniform; in flight across the barrier and the sums below
            f += fbytes;
#pragma unroll
            for (int k = 0; k < OV_ITEMS; ++k) raw[k] = load(k);
        }
        __syncthreads();
        // pixel (ly, lx) of the tile is byte (ly + 1, lx + 1) of the halo tile; a thread outside the frame reads bytes of the array
        // that nobody wrote and drops the sums below
        const unsigned char* yb = reinterpret_cast<const unsigned char*>(buf) + ly0 * OV_PITCH + lx;
        int up = yb[1], mid = yb[OV_PITCH + 1];
#pragma unroll
        for (int i = 0; i < OV_PER; ++i) {
            const unsigned char* q = yb + (i + 1) * OV_PITCH;
            const int down = q[OV_PITCH + 1];
            const int gx = (int)q[2] - (int)q[0], gy = down - up;
            sx[i] += gx;
            sy[i] += gy;
            sm[i] += (gx < 0 ? -gx : gx) + (gy < 0 ? -gy : gy);
            up = mid;
            mid = down;
        }
        // the buffer written two frames on is this one: every thread has passed the next frame's barrier by then, after these reads
    }
    if (lx >= tw) return;
    const long long N = (long long)H * W;
#pragma unroll
    for (int i = 0; i < OV_PER; ++i) {
        if (ly0 + i >= th) break;
        int* p = stats + (long long)(y0 + ly0 + i) * W + x0 + lx;
        if (ATOMIC) {
            atomicAdd(p, sx[i]);
            atomicAdd(p + N, sy[i]);
            atomicAdd(p + 2 * N, sm[i]);
        } else {
            p[0] = sx[i];
            p[N] = sy[i];
            p[2 * N] = sm[i];
        }
    }
}

// The persistent-edge map of those sums, dilated: E[y][x] = 1 iff M >= g_min L and 256 (|Sx| + |Sy|) >= coherence M (64-bit
// products), D = E dilated by the (2 r + 1) x (2 r + 1) box clipped at the frame (outside counts as 0), count = the number of
// set pixels of D.  A workgroup owns an OV_TW x OV_TH tile: E of the tile and its r-pixel halo goes to LDS as bytes, a row pass ORs
// 2 r + 1 neighbours, a column pass ORs 2 r + 1 rows of that; a wave counts its set pixels with a ballot and adds them once.
__global__ __launch_bounds__(NTH) void overlay_edges_kernel(const int* __restrict__ stats, int L, int H, int W, int g_min, int coherence,
                                                            int radius, int ntx, unsigned char* __restrict__ out, int* __restrict__ count) {
    __shared__ unsigned char s_e[OV_TH + 2 * OV_RMAX][OV_TW + 2 * OV_RMAX];
    __shared__ unsigned char s_h[OV_TH + 2 * OV_RMAX][OV_TW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ty = blockIdx.x / ntx, tx = blockIdx.x - ty * ntx;
    const int x0 = tx * OV_TW, y0 = ty * OV_TH;
    const int hh = OV_TH + 2 * radius, hw = OV_TW + 2 * radius, win = 2 * radius + 1;
    const long long N = (long long)H * W;
    const long long need = (long long)g_min * L;
    for (int r = wave; r < hh; r += NTH / 64) {
        const int y = y0 - radius + r;
        for (int c = lane; c < hw; c += 64) {
            const int x = x0 - radius + c;
            unsigned char e = 0;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                const long long i = (long long)y * W + x;
                const long long a = stats[i], b = stats[i + N], m = stats[i + 2 * N];
                e = m >= need && 256LL * ((a < 0 ? -a : a) + (b < 0 ? -b : b)) >= (long long)coherence * m;
            }
            s_e[r][c] = e;
        }
    }
    __syncthreads();
    for (int r = wave; r < hh; r += NTH / 64) {
        unsigned v = 0;
        for (int k = 0; k < win; ++k) v |= s_e[r][lane + k];
        s_h[r][lane] = (unsigned char)v;
    }
    __syncthreads();
    int n = 0;
    for (int i = 0; i < OV_PER; ++i) {
        const int ly = wave * OV_PER + i;
        unsigned v = 0;
        for (int k = 0; k < win; ++k) v |= s_h[ly + k][lane];
        const bool in = y0 + ly < H && x0 + lane < W;
        if (in) out[(long long)(y0 + ly) * W + x0 + lane] = (unsigned char)v;
        n += __popcll(__ballot(in && v));
    }
    if (lane == 0 && n) atomicAdd(count, n);
}

// Connected components of the hole's footprint (video.hole_regions: one crop region per group of holes).  U[y][x] = 1 iff some
// frame's mask byte at (x, y) is non-zero; labels[y][x] = 0 where U is 0, else the number 1 .. K of the pixel's 8-connected
// component, components numbered in raster order of their first pixel -- exact integers that do not depend on the order in which
// threads or atomics ran.  Six launches whatever the masks hold, no host read between them:
//   1 footprint   a thread ORs 16 consecutive pixels over the L frames (the L Hm Wm bytes that dominate the traffic): per frame the
//                 two aligned 16-byte words around its bytes, shifted by the frame's phase (v_alignbyte_b32; wave-uniform), so any
//                 base and pitch work; the chunks at the two ends of the buffer and the last partial chunk go byte by byte
//   2 tiles       a workgroup labels an LB_TW x LB_TH tile in LDS with a union-find; `labels` holds the forest afterwards:
//                 labels[i] = raster index of the tile-local root, -1 for background
//   3 borders     a thread per pixel of a tile's first row / first column unites it with its neighbours in the row above / the
//                 column to the left (the diagonal ones across a tile corner included), lock-free on the global forest
//   4 flatten     every pixel finds its root; a block of LB_SEG consecutive pixels counts its roots and ranks them in raster order
//   5 scan        one workgroup turns the blocks' counts into exclusive offsets and writes K
//   6 relabel     labels[i] = offset[block of root] + rank[root] + 1
// The forest keeps parent[i] <= i and entries only ever decrease: a union links the larger root under the smaller with atomicMin
// and goes on from the value that returns, a find halves its path with atomicMin.  Every loop walks to strictly smaller indices, so
// it ends by itself: no thread ever waits for another thread's write.  A root is therefore the smallest raster index of its set,
// which is what makes the numbering canonical.  Loads that race with those atomics may return an older parent: still an
// ancestor in the same set, so finds and unions stay correct.
// Which unions are needed: with the runs of a row joined (H: left neighbour), pixel p needs V (up) unless left and up-left are
// both set, and when up is not set UL unless left is set and UR unless right is set -- the rest follows by transitivity.  A tile
// does these for the neighbours it holds (a neighbour outside counts as not set, which only adds unions), the border pass does
// H / V / UL / UR across tile edges in the conservative form: the straight neighbour if set, else the two diagonal ones.
constexpr int LB_TW = 64, LB_TH = 32, LB_TILE = LB_TW * LB_TH;     // ops.LABEL_TILE_W / LABEL_TILE_H
constexpr int LB_PER = 4, LB_SEG = NTH * LB_PER;                    // consecutive pixels per thread / per block of the flatten pass
constexpr int LB_SLOTS = 256, LB_PROBES = 8;                        // label_boxes_kernel's LDS table
static_assert(LB_TW == 64 && NTH == 256, "a wave per tile row: the runs of a row come from one ballot");

__device__ __forceinline__ unsigned nz_bytes(unsigned v) {         // 1 in every byte of v that is not zero
    return ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) >> 7) & 0x01010101u;
}

__global__ __launch_bounds__(NTH) void hole_footprint_kernel(const unsigned char* __restrict__ m, int L, long long N,
                                                             unsigned char* __restrict__ foot) {
    const long long i0 = ((long long)blockIdx.x * NTH + threadIdx.x) * 16;
    if (i0 >= N) return;
    const unsigned char* const end = m + (long long)L * N;
    const bool whole = i0 + 16 <= N;
    unsigned a[4] = {0u, 0u, 0u, 0u};
#pragma unroll 2
    for (int l = 0; l < L; ++l) {
        const unsigned char* p = m + (long long)l * N + i0;
        const int sh = (int)((uintptr_t)p & 15);
        const unsigned char* q = p - sh;
        // both words lie inside the buffer: they may hold bytes of the neighbouring chunks or frames, which are shifted out
        if (whole && q >= m && q + (sh ? 32 : 16) <= end) {
            const uint4 lo = *reinterpret_cast<const uint4*>(q);
            if (sh == 0) {
                a[0] |= lo.x; a[1] |= lo.y; a[2] |= lo.z; a[3] |= lo.w;
            } else {
                const uint4 hi = *reinterpret_cast<const uint4*>(q + 16);
                unsigned s0, s1, s2, s3, s4;
                switch (sh >> 2) {
                    case 0: s0 = lo.x; s1 = lo.y; s2 = lo.z; s3 = lo.w; s4 = hi.x; break;
                    case 1: s0 = lo.y; s1 = lo.z; s2 = lo.w; s3 = hi.x; s4 = hi.y; break;
                    case 2: s0 = lo.z; s1 = lo.w; s2 = hi.x; s3 = hi.y; s4 = hi.z; break;
                    default: s0 = lo.w; s1 = hi.x; s2 = hi.y; s3 = hi.z; s4 = hi.w; break;
                }
                const unsigned b = (unsigned)(sh & 3);
                a[0] |= __builtin_amdgcn_alignbyte(s1, s0, b);
                a[1] |= __builtin_amdgcn_alignbyte(s2, s1, b);
                a[2] |= __builtin_amdgcn_alignbyte(s3, s2, b);
                a[3] |= __builtin_amdgcn_alignbyte(s4, s3, b);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (i0 + k < N) a[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
        }
    }
    if (whole) {
        *reinterpret_cast<uint4*>(foot + i0) = make_uint4(nz_bytes(a[0]), nz_bytes(a[1]), nz_bytes(a[2]), nz_bytes(a[3]));
    } else {
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (i0 + k < N) foot[i0 + k] = (unsigned char)(((a[k >> 2] >> (8 * (k & 3))) & 255u) != 0u);
    }
}

// the forest in LDS (a tile) and in global memory (the image): the same two loops
__device__ __forceinline__ int lb_load(const int* p, int i) { return *(const volatile int*)(p + i); }                    // LDS
__device__ __forceinline__ int lb_load_g(const int* p, int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <bool GLOBAL>
__device__ __forceinline__ int lb_find(int* p, int x) {
    int q = GLOBAL ? lb_load_g(p, x) : lb_load(p, x);
    while (q != x) {                                    // q < x: p[i] <= i
        const int g = GLOBAL ? lb_load_g(p, q) : lb_load(p, q);
        if (g != q) atomicMin(p + x, g);                // path halving; g < q < x is an ancestor of x
        x = q;
        q = g;
    }
    return x;
}

template <bool GLOBAL>
__device__ __forceinline__ void lb_unite(int* p, int a, int b) {
    for (;;) {
        a = lb_find<GLOBAL>(p, a);
        b = lb_find<GLOBAL>(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(p + a, b);            // the larger root under the smaller
        if (old == a) return;                           // a was still a root: linked
        a = old;                                        // someone linked a under old < a meanwhile: old's set and b's are still to be united
    }
}

__global__ __launch_bounds__(NTH) void label_tile_kernel(const unsigned char* __restrict__ foot, int* __restrict__ labels, int Hm,
                                                         int Wm, int ntx) {
    __shared__ int s_p[LB_TILE];
    const int ty = (int)(blockIdx.x / (unsigned)ntx), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)ntx);
    const int x0 = tx * LB_TW, y0 = ty * LB_TH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = x0 + lane;
    // a pixel starts under the first pixel of its run in the tile row: H is done
    for (int r = wave; r < LB_TH; r += NTH / 64) {
        const int y = y0 + r;
        const bool f = y < Hm && x < Wm && foot[(long long)y * Wm + x] != 0;
        const unsigned long long z = ~__ballot(f) & ((1ull << lane) - 1ull);      // background lanes below this one
        s_p[r * LB_TW + lane] = f ? r * LB_TW + (z ? 64 - __clzll((long long)z) : 0) : -1;
    }
    __syncthreads();
    for (int r = wave ? wave : NTH / 64; r < LB_TH; r += NTH / 64) {               // rows 1 .. LB_TH - 1
        const int i = r * LB_TW + lane;
        if (lb_load(s_p, i) < 0) continue;
        const bool up = lb_load(s_p, i - LB_TW) >= 0;
        const bool left = lane > 0 && lb_load(s_p, i - 1) >= 0, right = lane < LB_TW - 1 && lb_load(s_p, i + 1) >= 0;
        const bool ul = lane > 0 && lb_load(s_p, i - LB_TW - 1) >= 0, ur = lane < LB_TW - 1 && lb_load(s_p, i - LB_TW + 1) >= 0;
        if (up) {
            if (!(left && ul)) lb_unite<false>(s_p, i, i - LB_TW);
        } else {
            if (ul && !left) lb_unite<false>(s_p, i, i - LB_TW - 1);
            if (ur && !right) lb_unite<false>(s_p, i, i - LB_TW + 1);
        }
    }
    __syncthreads();
    for (int r = wave; r < LB_TH; r += NTH / 64) {
        const int y = y0 + r;
        if (y >= Hm || x >= Wm) continue;
        const int i = r * LB_TW + lane;
        int root = -1;
        if (lb_load(s_p, i) >= 0) {
            const int t = lb_find<false>(s_p, i);       // the smallest tile index of the set, so its smallest raster index too
            root = (int)((long long)(y0 + t / LB_TW) * Wm + x0 + t % LB_TW);
        }
        labels[(long long)y * Wm + x] = root;
    }
}

__global__ __launch_bounds__(NTH) void label_border_kernel(int* __restrict__ labels, int Hm, int Wm, long long nrow, long long total) {
    const long long t = (long long)blockIdx.x * NTH + threadIdx.x;
    if (t >= total) return;
    if (t < nrow) {                                     // pixel (x, y) of the first row of a tile row, y > 0
        const int b = (int)(t / Wm), x = (int)(t - (long long)b * Wm);
        const int i = (int)((long long)(b + 1) * LB_TH * Wm + x);
        if (lb_load_g(labels, i) < 0) return;
        const int up = i - Wm;
        if (lb_load_g(labels, up) >= 0) {
            lb_unite<true>(labels, i, up);
        } else {
            if (x > 0 && lb_load_g(labels, up - 1) >= 0) lb_unite<true>(labels, i, up - 1);
            if (x + 1 < Wm && lb_load_g(labels, up + 1) >= 0) lb_unite<true>(labels, i, up + 1);
        }
    } else {                                            // pixel (x, y) of the first column of a tile column, x > 0
        const long long u = t - nrow;
        const int b = (int)(u / Hm), y = (int)(u - (long long)b * Hm);
        const int i = (int)((long long)y * Wm + (long long)(b + 1) * LB_TW);
        if (lb_load_g(labels, i) < 0) return;
        const int lf = i - 1;
        if (lb_load_g(labels, lf) >= 0) {
            lb_unite<true>(labels, i, lf);
        } else {
            if (y > 0 && lb_load_g(labels, lf - Wm) >= 0) lb_unite<true>(labels, i, lf - Wm);
            if (y + 1 < Hm && lb_load_g(labels, lf + Wm) >= 0) lb_unite<true>(labels, i, lf + Wm);
        }
    }
}

// exclusive scan of one value per thread over the block (wave64 shuffles, the waves' totals through LDS); total: the block's sum
__device__ __forceinline__ int block_scan_excl(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(inc, o, 64);
        if (lane >= o) inc += n;
    }
    __syncthreads();                                    // s_w may still be read from the previous call
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NTH / 64; ++w) {
        if (w < wave) before += s_w[w];
        total += s_w[w];
    }
    return before + inc - v;
}

__global__ __launch_bounds__(NTH) void label_flatten_kernel(int* __restrict__ labels, int* __restrict__ rank, int* __restrict__ counts,
                                                            long long N) {
    __shared__ int s_w[NTH / 64];
    const long long i0 = (long long)blockIdx.x * LB_SEG + (long long)threadIdx.x * LB_PER;
    bool is_root[LB_PER];
    int c = 0;
#pragma unroll
    for (int k = 0; k < LB_PER; ++k) {
        const long long i = i0 + k;
        is_root[k] = false;
        if (i < N) {
            const int t = lb_load_g(labels, (int)i);
            if (t >= 0) {
                const int r = lb_find<true>(labels, t);
                labels[i] = r;                          // no union runs in this pass: r is the root for good
                is_root[k] = r == (int)i;
            }
        }
        c += is_root[k];
    }
    int total;
    int e = block_scan_excl(c, s_w, total);
#pragma unroll
    for (int k = 0; k < LB_PER; ++k)
        if (is_root[k]) rank[i0 + k] = e++;
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(NTH) void label_scan_kernel(int* __restrict__ counts, long long nblk, int* __restrict__ count) {
    __shared__ int s_w[NTH / 64];
    int carry = 0;
    for (long long base = 0; base < nblk; base += NTH) {
        const long long i = base + threadIdx.x;
        const int v = i < nblk ? counts[i] : 0;
        int total;
        const int e = block_scan_excl(v, s_w, total);
        if (i < nblk) counts[i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) *count = carry;
}

__global__ void label_number_kernel(int* __restrict__ labels, const int* __restrict__ rank, const int* __restrict__ offs, long long N) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int r = labels[i];
    labels[i] = r < 0 ? 0 : offs[r / LB_SEG] + rank[r] + 1;
}

// Bounding boxes and areas of labelled components: boxes[k-1] = (x0, y0, x1, y1, area) of label k, upper ends exclusive.  A
// workgroup owns a tile, a wave a row of it at a time: a run of equal labels is one entry (its first lane's, found with a shuffle
// and a ballot), entries of one label meet in an LDS table (open addressing, at most LB_PROBES probes -- a run that finds no slot
// goes to global memory itself), and every used slot issues five global atomics at the end.  A label outside [1, K] is skipped, so
// the kernel stays in bounds whatever the labels hold.
__global__ void label_boxes_init_kernel(int* __restrict__ boxes, long long n) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) boxes[idx] = idx % 5 < 2 ? 0x7fffffff : 0;
}

__device__ __forceinline__ void label_box_add(int* b, int x0, int y0, int x1, int y1, int area) {
    atomicMin(b, x0);
    atomicMin(b + 1, y0);
    atomicMax(b + 2, x1);
    atomicMax(b + 3, y1);
    atomicAdd(b + 4, area);
}

__global__ __launch_bounds__(NTH) void label_boxes_kernel(const int* __restrict__ labels, int Hm, int Wm, int ntx, int K,
                                                          int* __restrict__ boxes) {
    __shared__ int s_key[LB_SLOTS];
    __shared__ int s_box[LB_SLOTS][5];
    for (int i = threadIdx.x; i < LB_SLOTS; i += NTH) {
        s_key[i] = 0;
        s_box[i][0] = s_box[i][1] = 0x7fffffff;
        s_box[i][2] = s_box[i][3] = s_box[i][4] = 0;
    }
    __syncthreads();
    const int ty = (int)(blockIdx.x / (unsigned)ntx), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)ntx);
    const int x0 = tx * LB_TW, y0 = ty * LB_TH;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = x0 + lane;
    for (int r = wave; r < LB_TH; r += NTH / 64) {
        const int y = y0 + r;
        int lab = y < Hm && x < Wm ? labels[(long long)y * Wm + x] : 0;
        if (lab < 0 || lab > K) lab = 0;
        const int prev = __shfl_up(lab, 1, 64);
        const bool first = lane == 0 || prev != lab;
        const unsigned long long starts = __ballot(first);
        if (!first || !lab) continue;
        const unsigned long long later = lane == 63 ? 0ull : starts >> (lane + 1);
        const int len = later ? __ffsll((long long)later) : 64 - lane;
        int h = (int)(((unsigned)lab * 0x9E3779B1u) >> 24);
        bool done = false;
        for (int pr = 0; pr < LB_PROBES && !done; ++pr) {
            const int old = atomicCAS(&s_key[h], 0, lab);
            if (old == 0 || old == lab) {
                label_box_add(s_box[h], x, y, x + len, y + 1, len);
                done = true;
            }
            h = (h + 1) & (LB_SLOTS - 1);
        }
        if (!done) label_box_add(boxes + 5LL * (lab - 1), x, y, x + len, y + 1, len);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < LB_SLOTS; i += NTH)
        if (s_key[i]) label_box_add(boxes + 5LL * (s_key[i] - 1), s_box[i][0], s_box[i][1], s_box[i][2], s_box[i][3], s_box[i][4]);
}

// the workspace of e2fgvi_hole_label for N pixels: rank int32 [N] | footprint uint8 [N] | counts int32 [ceil(N / LB_SEG)], each
// part starting at a multiple of 16 bytes
struct LabelWork { long long rank, foot, counts, bytes, nblk; };
inline LabelWork label_work(long long N) {
    LabelWork w;
    w.nblk = (N + LB_SEG - 1) / LB_SEG;
    w.rank = 0;
    w.foot = (4 * N + 15) / 16 * 16;
    w.counts = w.foot + (N + 15) / 16 * 16;
    w.bytes = w.counts + (4 * w.nblk + 15) / 16 * 16;
    return w;
}

inline bool ranges_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

}  // namespace

// e2fgvi_restore_box_u8 (feather == 0) and e2fgvi_restore_feather_u8: the same checks, the kernel of their paste
static int restore_box(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, uint8_t* out, int32_t L, int32_t h, int32_t w,
                       int32_t H, int32_t W, int32_t left, int32_t upper, int32_t Bw, int32_t Bh, const int32_t* ytab,
                       const int32_t* xtab, const int32_t* bounds_x, const int32_t* coeffs_x, int32_t ksize_x, const int32_t* bounds_y,
                       const int32_t* coeffs_y, int32_t ksize_y, int32_t feather, void* stream) {
    E2_REQUIRE(lo && mask_lo && src && out && ytab && xtab && bounds_x && coeffs_x && bounds_y && coeffs_y, E2FGVI_EINVAL,
               "restore_u8: null pointer");
    E2_REQUIRE(L > 0 && h > 0 && w > 0 && H > 0 && W > 0 && ksize_x >= 1 && ksize_y >= 1, E2FGVI_EINVAL,
               "restore_u8: sizes and tap counts must be positive");
    E2_REQUIRE(left >= 0 && upper >= 0 && Bw > 0 && Bh > 0 && Bw <= W - left && Bh <= H - upper, E2FGVI_EINVAL,
               "restore_u8: the box (%d, %d) + %d x %d must be non-empty and lie inside the %d x %d frame", left, upper, Bw, Bh, W, H);
    E2_REQUIRE(W * 3LL <= 0x7fffffffLL && w * 3LL <= 0x7fffffffLL && (H + RT_H - 1) / RT_H <= 65535, E2FGVI_EINVAL,
               "restore_u8: frames too large");
    const long long n_out = (long long)L * H * W * 3, n_lo = (long long)L * h * w * 3;
    E2_REQUIRE(!ranges_overlap(out, n_out, src, n_out) && !ranges_overlap(out, n_out, lo, n_lo) &&
                   !ranges_overlap(out, n_out, mask_lo, n_lo / 3),
               E2FGVI_EINVAL, "restore_u8: out must not overlap src, lo or mask_lo");
    const dim3 grid((unsigned)((W + RT_W - 1) / RT_W), (unsigned)((H + RT_H - 1) / RT_H), (unsigned)(L < 1024 ? L : 1024));
    const RestoreTouch touch{0, 0, W, H};
    if (feather)
        hipLaunchKernelGGL((restore_u8_kernel<false, true>), grid, dim3(NTH), 0, (hipStream_t)stream, lo, mask_lo, src, out, (float*)nullptr,
                           (const int*)nullptr, (const unsigned char*)nullptr, L, 0, 0, touch, L, h, w, H, W, left, upper,
                           Bw, Bh, ytab, xtab, bounds_x, coeffs_x, ksize_x, bounds_y, coeffs_y, ksize_y, feather);
    else
        hipLaunchKernelGGL((restore_u8_kernel<false, false>), grid, dim3(NTH), 0, (hipStream_t)stream, lo, mask_lo, src, out, (float*)nullptr,
                           (const int*)nullptr, (const unsigned char*)nullptr, L, 0, 0, touch, L, h, w, H, W, left, upper,
                           Bw, Bh, ytab, xtab, bounds_x, coeffs_x, ksize_x, bounds_y, coeffs_y, ksize_y, 0);
    E2_LAUNCH_CHECK("restore_u8");
    return 0;
}

extern "C" int e2fgvi_restore_box_u8(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, uint8_t* out, int32_t L, int32_t h,
                                     int32_t w, int32_t H, int32_t W, int32_t left, int32_t upper, int32_t Bw, int32_t Bh,
                                     const int32_t* ytab, const int32_t* xtab, const int32_t* bounds_x, const int32_t* coeffs_x,
                                     int32_t ksize_x, const int32_t* bounds_y, const int32_t* coeffs_y, int32_t ksize_y, void* stream) {
    return restore_box(lo, mask_lo, src, out, L, h, w, H, W, left, upper, Bw, Bh, ytab, xtab, bounds_x, coeffs_x, ksize_x, bounds_y,
                       coeffs_y, ksize_y, 0, stream);
}

extern "C" int e2fgvi_restore_feather_u8(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, uint8_t* out, int32_t L,
                                         int32_t h, int32_t w, int32_t H, int32_t W, int32_t left, int32_t upper, int32_t Bw, int32_t Bh,
                                         const int32_t* ytab, const int32_t* xtab, const int32_t* bounds_x, const int32_t* coeffs_x,
                                         int32_t ksize_x, const int32_t* bounds_y, const int32_t* coeffs_y, int32_t ksize_y,
                                         int32_t feather, void* stream) {
    E2_REQUIRE(feather >= 1 && feather <= RF_MAX, E2FGVI_EINVAL, "restore_feather_u8: feather must be in [1, %d], got %d", RF_MAX, feather);
    return restore_box(lo, mask_lo, src, out, L, h, w, H, W, left, upper, Bw, Bh, ytab, xtab, bounds_x, coeffs_x, ksize_x, bounds_y,
                       coeffs_y, ksize_y, feather, stream);
}

// e2fgvi_restore_blend (feather == 0) and e2fgvi_restore_feather_blend: the same checks, the kernel of their paste
static int restore_blend(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, const int32_t* ids, const uint8_t* first,
                         float* acc, int32_t n, int32_t L, int32_t h, int32_t w, int32_t H, int32_t W, int32_t left, int32_t upper,
                         int32_t Bw, int32_t Bh, int32_t touch_left, int32_t touch_upper, int32_t Tw, int32_t Th, const int32_t* ytab,
                         const int32_t* xtab, const int32_t* bounds_x, const int32_t* coeffs_x, int32_t ksize_x, const int32_t* bounds_y,
                         const int32_t* coeffs_y, int32_t ksize_y, int32_t feather, void* stream) {
    E2_REQUIRE(lo && mask_lo && src && ids && first && acc && ytab && xtab && bounds_x && coeffs_x && bounds_y && coeffs_y, E2FGVI_EINVAL,
               "restore_blend: null pointer");
    E2_REQUIRE(n > 0 && L > 0 && h > 0 && w > 0 && H > 0 && W > 0 && ksize_x >= 1 && ksize_y >= 1, E2FGVI_EINVAL,
               "restore_blend: sizes and tap counts must be positive");
    E2_REQUIRE(left >= 0 && upper >= 0 && Bw > 0 && Bh > 0 && Bw <= W - left && Bh <= H - upper, E2FGVI_EINVAL,
               "restore_blend: the box (%d, %d) + %d x %d must be non-empty and lie inside the %d x %d frame", left, upper, Bw, Bh, W, H);
    E2_REQUIRE(touch_left >= 0 && touch_upper >= 0 && Tw > 0 && Th > 0 && Tw <= W - touch_left && Th <= H - touch_upper &&
                   touch_left <= left && touch_upper <= upper && Bw <= Tw - (left - touch_left) && Bh <= Th - (upper - touch_upper),
               E2FGVI_EINVAL, "restore_blend: the touched rectangle (%d, %d) + %d x %d must lie inside the frame and contain the box",
               touch_left, touch_upper, Tw, Th);
    E2_REQUIRE(W * 3LL <= 0x7fffffffLL && w * 3LL <= 0x7fffffffLL && (H + RT_H - 1) / RT_H <= 65535, E2FGVI_EINVAL,
               "restore_blend: frames too large");
    E2_REQUIRE((uintptr_t)acc % sizeof(float) == 0, E2FGVI_EINVAL, "restore_blend: acc must be aligned to 4 bytes");
    const long long n_src = (long long)L * H * W * 3, n_lo = (long long)n * h * w * 3;
    E2_REQUIRE(!ranges_overlap(acc, n_src * 4, src, n_src) && !ranges_overlap(acc, n_src * 4, lo, n_lo) &&
                   !ranges_overlap(acc, n_src * 4, mask_lo, n_lo / 3) && !ranges_overlap(acc, n_src * 4, ids, n * 4LL) &&
                   !ranges_overlap(acc, n_src * 4, first, n),
               E2FGVI_EINVAL, "restore_blend: acc must not overlap src, lo, mask_lo, ids or first");
    // the tiles of the frame-aligned tile grid that the touched rectangle reaches
    const int tx0 = touch_left / RT_W, ty0 = touch_upper / RT_H;
    const int tx1 = (touch_left + Tw - 1) / RT_W, ty1 = (touch_upper + Th - 1) / RT_H;
    const dim3 grid((unsigned)(tx1 - tx0 + 1), (unsigned)(ty1 - ty0 + 1), (unsigned)(n < 1024 ? n : 1024));
    const RestoreTouch touch{touch_left, touch_upper, Tw, Th};
    if (feather)
        hipLaunchKernelGGL((restore_u8_kernel<true, true>), grid, dim3(NTH), 0, (hipStream_t)stream, lo, mask_lo, src, (unsigned char*)nullptr,
                           acc, ids, first, L, tx0, ty0, touch, n, h, w, H, W, left, upper, Bw, Bh, ytab,
                           xtab, bounds_x, coeffs_x, ksize_x, bounds_y, coeffs_y, ksize_y, feather);
    else
        hipLaunchKernelGGL((restore_u8_kernel<true, false>), grid, dim3(NTH), 0, (hipStream_t)stream, lo, mask_lo, src, (unsigned char*)nullptr, acc,
                           ids, first, L, tx0, ty0, touch, n, h, w, H, W, left, upper, Bw, Bh, ytab,
                           xtab, bounds_x, coeffs_x, ksize_x, bounds_y, coeffs_y, ksize_y, 0);
    E2_LAUNCH_CHECK("restore_blend");
    return 0;
}

extern "C" int e2fgvi_restore_blend(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, const int32_t* ids,
                                    const uint8_t* first, float* acc, int32_t n, int32_t L, int32_t h, int32_t w, int32_t H, int32_t W,
                                    int32_t left, int32_t upper, int32_t Bw, int32_t Bh, int32_t touch_left, int32_t touch_upper,
                                    int32_t Tw, int32_t Th, const int32_t* ytab, const int32_t* xtab, const int32_t* bounds_x,
                                    const int32_t* coeffs_x, int32_t ksize_x, const int32_t* bounds_y, const int32_t* coeffs_y,
                                    int32_t ksize_y, void* stream) {
    return restore_blend(lo, mask_lo, src, ids, first, acc, n, L, h, w, H, W, left, upper, Bw, Bh, touch_left, touch_upper, Tw, Th, ytab,
                         xtab, bounds_x, coeffs_x, ksize_x, bounds_y, coeffs_y, ksize_y, 0, stream);
}

extern "C" int e2fgvi_restore_feather_blend(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, const int32_t* ids,
                                            const uint8_t* first, float* acc, int32_t n, int32_t L, int32_t h, int32_t w, int32_t H,
                                            int32_t W, int32_t left, int32_t upper, int32_t Bw, int32_t Bh, int32_t touch_left,
                                            int32_t touch_upper, int32_t Tw, int32_t Th, const int32_t* ytab, const int32_t* xtab,
                                            const int32_t* bounds_x, const int32_t* coeffs_x, int32_t ksize_x, const int32_t* bounds_y,
                                            const int32_t* coeffs_y, int32_t ksize_y, int32_t feather, void* stream) {
    E2_REQUIRE(feather >= 1 && feather <= RF_MAX, E2FGVI_EINVAL, "restore_feather_blend: feather must be in [1, %d], got %d", RF_MAX,
               feather);
    return restore_blend(lo, mask_lo, src, ids, first, acc, n, L, h, w, H, W, left, upper, Bw, Bh, touch_left, touch_upper, Tw, Th, ytab,
                         xtab, bounds_x, coeffs_x, ksize_x, bounds_y, coeffs_y, ksize_y, feather, stream);
}

// the whole frame as the box: the same checks, the same kernel
extern "C" int e2fgvi_restore_u8(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, uint8_t* out, int32_t L, int32_t h,
                                 int32_t w, int32_t H, int32_t W, const int32_t* ytab, const int32_t* xtab, const int32_t* bounds_x,
                                 const int32_t* coeffs_x, int32_t ksize_x, const int32_t* bounds_y, const int32_t* coeffs_y,
                                 int32_t ksize_y, void* stream) {
    E2_REQUIRE(H > 0 && W > 0, E2FGVI_EINVAL, "restore_u8: sizes and tap counts must be positive");
    return e2fgvi_restore_box_u8(lo, mask_lo, src, out, L, h, w, H, W, 0, 0, W, H, ytab, xtab, bounds_x, coeffs_x, ksize_x, bounds_y,
                                 coeffs_y, ksize_y, stream);
}

extern "C" int e2fgvi_hole_bbox(const uint8_t* masks, int32_t L, int32_t Hm, int32_t Wm, int32_t* box, void* stream) {
    E2_REQUIRE(box && L >= 0 && Hm >= 0 && Wm >= 0, E2FGVI_EINVAL, "hole_bbox: bad arguments");
    const long long rows = (long long)L * Hm;
    E2_REQUIRE(masks || rows * Wm == 0, E2FGVI_EINVAL, "hole_bbox: null masks");
    // the empty box (0x7f7f7f7f, 0x7f7f7f7f, 0, 0), on the stream of the launch that lowers / raises it
    hipError_t e = hipMemsetAsync(box, 0x7f, 2 * sizeof(int32_t), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(box + 2, 0, 2 * sizeof(int32_t), (hipStream_t)stream);
    E2_REQUIRE(e == hipSuccess, (int)e, "hole_bbox: hipMemsetAsync failed: %s", hipGetErrorString(e));
    if (rows * Wm == 0) return 0;
    // a wave per row; enough blocks to fill the chip, the rest grid-strided
    long long blocks = (rows + BB_WAVES - 1) / BB_WAVES;
    blocks = blocks < 2048 ? blocks : 2048;
    hipLaunchKernelGGL(hole_bbox_kernel, dim3((unsigned)blocks), dim3(NTH), 0, (hipStream_t)stream, masks, rows, Hm, Wm, box);
    E2_LAUNCH_CHECK("hole_bbox");
    return 0;
}

extern "C" int e2fgvi_hole_bbox_frames(const uint8_t* masks, int32_t L, int32_t Hm, int32_t Wm, int32_t* boxes, void* stream) {
    E2_REQUIRE(L >= 0 && Hm >= 0 && Wm >= 0, E2FGVI_EINVAL, "hole_bbox_frames: bad arguments");
    if (L == 0) return 0;
    E2_REQUIRE(boxes, E2FGVI_EINVAL, "hole_bbox_frames: null boxes");
    E2_REQUIRE(masks || (long long)Hm * Wm == 0, E2FGVI_EINVAL, "hole_bbox_frames: null masks");
    // every frame's box starts empty, (0x7f7f7f7f, 0x7f7f7f7f, 0, 0), on the stream of the launch that lowers / raises it
    hipLaunchKernelGGL(bbox_init_kernel, dim3(blocks_for(4LL * L)), dim3(NTH), 0, (hipStream_t)stream, boxes, 4LL * L);
    E2_LAUNCH_CHECK("hole_bbox_frames");
    if ((long long)Hm * Wm == 0) return 0;
    // a wave per row of a frame, a grid row per frame
    const int bx = (Hm + BB_WAVES - 1) / BB_WAVES < 2048 ? (Hm + BB_WAVES - 1) / BB_WAVES : 2048;
    return fb_slabs("hole_bbox_frames", L, [&](int l0, unsigned nl) {
        hipLaunchKernelGGL(hole_bbox_kernel, dim3((unsigned)bx, nl), dim3(NTH), 0, (hipStream_t)stream, masks + (long long)l0 * Hm * Wm,
                           (long long)Hm, Hm, Wm, boxes + 4LL * l0);
    });
}

extern "C" int e2fgvi_gather_slabs(const void* cache, int32_t slots, const int32_t* ids, int32_t n, int64_t slab_bytes, void* window,
                                   void* stream) {
    const int rc = slab_copy<false>(cache, window, ids, n, slots, slab_bytes, stream, "gather_slabs");
    if (rc) return rc;
    E2_LAUNCH_CHECK("gather_slabs");
    return 0;
}

extern "C" int e2fgvi_scatter_slabs(const void* rows, const int32_t* ids, int32_t n, int64_t slab_bytes, void* cache, int32_t slots,
                                    void* stream) {
    const int rc = slab_copy<true>(cache, rows, ids, n, slots, slab_bytes, stream, "scatter_slabs");
    if (rc) return rc;
    E2_LAUNCH_CHECK("scatter_slabs");
    return 0;
}

extern "C" int e2fgvi_mask_prepare(const uint8_t* masks, int32_t L, int32_t Hin, int32_t Win, const int32_t* ytab,
                                   const int32_t* xtab, uint8_t* out, int32_t H, int32_t W, int32_t iterations, void* stream) {
    E2_REQUIRE(masks && ytab && xtab && out && L > 0 && Hin > 0 && Win > 0 && H > 0 && W > 0 && iterations >= 0 && iterations <= 64,
               E2FGVI_EINVAL, "mask_prepare: bad arguments");
    hipLaunchKernelGGL(mask_prepare_kernel, dim3(blocks_for((long long)L * H * W)), dim3(NTH), 0, (hipStream_t)stream, masks, L,
                       (const int*)nullptr, Hin, Win, ytab, xtab, out, L, H, W, iterations);
    E2_LAUNCH_CHECK("mask_prepare");
    return 0;
}

extern "C" int e2fgvi_mask_prepare_ids(const uint8_t* masks, int32_t L, const int32_t* ids, int32_t n, int32_t Hin, int32_t Win,
                                       const int32_t* ytab, const int32_t* xtab, uint8_t* out, int32_t H, int32_t W, int32_t iterations,
                                       void* stream) {
    E2_REQUIRE(masks && ids && ytab && xtab && out && L > 0 && n > 0 && Hin > 0 && Win > 0 && H > 0 && W > 0 && iterations >= 0 &&
                   iterations <= 64,
               E2FGVI_EINVAL, "mask_prepare_ids: bad arguments");
    hipLaunchKernelGGL(mask_prepare_kernel, dim3(blocks_for((long long)n * H * W)), dim3(NTH), 0, (hipStream_t)stream, masks, L, ids,
                       Hin, Win, ytab, xtab, out, n, H, W, iterations);
    E2_LAUNCH_CHECK("mask_prepare_ids");
    return 0;
}

extern "C" int e2fgvi_masked_clip(const uint8_t* frames, const uint8_t* masks, const int32_t* ids, int32_t t, int32_t H, int32_t W,
                                  float* clip, int32_t Hp, int32_t Wp, void* stream) {
    E2_REQUIRE(frames && masks && ids && clip && t > 0 && H > 0 && W > 0, E2FGVI_EINVAL, "masked_clip: bad arguments");
    E2_REQUIRE(Hp >= H && Wp >= W && Hp <= 2 * H && Wp <= 2 * W, E2FGVI_EINVAL, "masked_clip: padded size must be in [size, 2 size]");
    hipLaunchKernelGGL(masked_clip_kernel, dim3(blocks_for((long long)t * 3 * Hp * Wp)), dim3(NTH), 0, (hipStream_t)stream, frames,
                       masks, ids, clip, t, H, W, Hp, Wp);
    E2_LAUNCH_CHECK("masked_clip");
    return 0;
}

extern "C" int e2fgvi_composite(const float* pred, const int32_t* ids, const uint8_t* first, int32_t n, const uint8_t* frames,
                                const uint8_t* masks, float* comp, int32_t H, int32_t W, int32_t Hp, int32_t Wp, void* stream) {
    E2_REQUIRE(pred && ids && first && frames && masks && comp && n > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W, E2FGVI_EINVAL,
               "composite: bad arguments");
    hipLaunchKernelGGL(composite_kernel, dim3(blocks_for((long long)n * H * W * 3)), dim3(NTH), 0, (hipStream_t)stream, pred, ids,
                       first, frames, masks, comp, n, H, W, Hp, Wp);
    E2_LAUNCH_CHECK("composite");
    return 0;
}

// the two resample entries and their variants with a frame table: Lsrc frames in src, output frame l from frame ids[l] (no
// table: Lsrc == L, frame l)
static int resample_rows(const char* what, const uint8_t* src, int32_t Lsrc, const int32_t* ids, uint8_t* dst, int32_t L, int32_t H,
                         int32_t W, int32_t n_out, int32_t row0, int32_t rows, const int32_t* bounds, const int32_t* coeffs,
                         int32_t ksize, void* stream) {
    E2_REQUIRE(src && dst && bounds && coeffs && L > 0 && Lsrc > 0 && H > 0 && W > 0 && n_out > 0 && ksize > 0, E2FGVI_EINVAL,
               "%s: bad arguments", what);
    E2_REQUIRE(row0 >= 0 && rows > 0 && rows <= H - row0, E2FGVI_EINVAL, "%s: rows [%d, %d + %d) leave the %d rows of a frame", what,
               row0, row0, rows, H);
    E2_REQUIRE(W * 3LL <= 0x7fffffffLL && n_out * 3LL <= 0x7fffffffLL, E2FGVI_EINVAL, "%s: rows too wide", what);
    const long long total = (long long)L * rows;
    const unsigned grid = (unsigned)(total < (1LL << 20) ? total : (1LL << 20));     // the kernel strides over the rest
    hipLaunchKernelGGL(resample_u8_kernel<false>, dim3(grid), dim3(NTH), 0, (hipStream_t)stream, src, Lsrc, ids, dst, L, H, W, n_out,
                       row0, rows, bounds, coeffs, ksize);
    E2_LAUNCH_CHECK(what);
    return 0;
}

static int resample_axis(const char* what, const uint8_t* src, int32_t Lsrc, const int32_t* ids, uint8_t* dst, int32_t L, int32_t H,
                         int32_t W, int32_t n_out, int32_t axis, const int32_t* bounds, const int32_t* coeffs, int32_t ksize,
                         void* stream) {
    E2_REQUIRE(src && dst && bounds && coeffs && L > 0 && Lsrc > 0 && H > 0 && W > 0 && n_out > 0 && ksize > 0, E2FGVI_EINVAL,
               "%s: bad arguments", what);
    E2_REQUIRE(axis == 1 || axis == 2, E2FGVI_EINVAL, "%s: axis must be 1 (H) or 2 (W), got %d", what, axis);
    const long long Wo = axis == 2 ? n_out : W;
    E2_REQUIRE(W * 3LL <= 0x7fffffffLL && Wo * 3 <= 0x7fffffffLL, E2FGVI_EINVAL, "%s: rows too wide", what);
    const long long rows = (long long)L * (axis == 1 ? n_out : H);
    const unsigned grid = (unsigned)(rows < (1LL << 20) ? rows : (1LL << 20));      // the kernel strides over the rest
    if (axis == 1)
        hipLaunchKernelGGL(resample_u8_kernel<true>, dim3(grid), dim3(NTH), 0, (hipStream_t)stream, src, Lsrc, ids, dst, L, H, W, n_out, 0,
                           H, bounds, coeffs, ksize);
    else
        hipLaunchKernelGGL(resample_u8_kernel<false>, dim3(grid), dim3(NTH), 0, (hipStream_t)stream, src, Lsrc, ids, dst, L, H, W, n_out, 0,
                           H, bounds, coeffs, ksize);
    E2_LAUNCH_CHECK(what);
    return 0;
}

extern "C" int e2fgvi_resample_rows_u8(const uint8_t* src, uint8_t* dst, int32_t L, int32_t H, int32_t W, int32_t n_out, int32_t row0,
                                       int32_t rows, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, void* stream) {
    return resample_rows("resample_rows_u8", src, L, nullptr, dst, L, H, W, n_out, row0, rows, bounds, coeffs, ksize, stream);
}

extern "C" int e2fgvi_resample_rows_ids_u8(const uint8_t* src, int32_t L, const int32_t* ids, int32_t n, uint8_t* dst, int32_t H,
                                           int32_t W, int32_t n_out, int32_t row0, int32_t rows, const int32_t* bounds,
                                           const int32_t* coeffs, int32_t ksize, void* stream) {
    E2_REQUIRE(ids, E2FGVI_EINVAL, "resample_rows_ids_u8: null ids");
    return resample_rows("resample_rows_ids_u8", src, L, ids, dst, n, H, W, n_out, row0, rows, bounds, coeffs, ksize, stream);
}

extern "C" int e2fgvi_resample_u8(const uint8_t* src, uint8_t* dst, int32_t L, int32_t H, int32_t W, int32_t n_out, int32_t axis,
                                  const int32_t* bounds, const int32_t* coeffs, int32_t ksize, void* stream) {
    return resample_axis("resample_u8", src, L, nullptr, dst, L, H, W, n_out, axis, bounds, coeffs, ksize, stream);
}

extern "C" int e2fgvi_resample_ids_u8(const uint8_t* src, int32_t L, const int32_t* ids, int32_t n, uint8_t* dst, int32_t H, int32_t W,
                                      int32_t n_out, int32_t axis, const int32_t* bounds, const int32_t* coeffs, int32_t ksize,
                                      void* stream) {
    E2_REQUIRE(ids, E2FGVI_EINVAL, "resample_ids_u8: null ids");
    return resample_axis("resample_ids_u8", src, L, ids, dst, n, H, W, n_out, axis, bounds, coeffs, ksize, stream);
}

extern "C" int e2fgvi_float_to_u8(const float* src, uint8_t* dst, int64_t n, void* stream) {
    E2_REQUIRE(src && dst && n > 0, E2FGVI_EINVAL, "float_to_u8: bad arguments");
    hipLaunchKernelGGL(float_to_u8_kernel, dim3(blocks_for(n)), dim3(NTH), 0, (hipStream_t)stream, src, dst, (long long)n);
    E2_LAUNCH_CHECK("float_to_u8");
    return 0;
}

extern "C" int e2fgvi_u8_to_float(const uint8_t* src, float* dst, int64_t n, void* stream) {
    E2_REQUIRE(src && dst && n > 0, E2FGVI_EINVAL, "u8_to_float: bad arguments");
    const unsigned grid = blocks_for((n + 3) / 4);
    if (((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 15) == 0)
        hipLaunchKernelGGL(u8_to_float_kernel<true>, dim3(grid), dim3(NTH), 0, (hipStream_t)stream, src, dst, (long long)n);
    else
        hipLaunchKernelGGL(u8_to_float_kernel<false>, dim3(grid), dim3(NTH), 0, (hipStream_t)stream, src, dst, (long long)n);
    E2_LAUNCH_CHECK("u8_to_float");
    return 0;
}

extern "C" int e2fgvi_pred_to_u8(const float* pred, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t Hp, int32_t Wp,
                                 void* stream) {
    E2_REQUIRE(pred && dst && N > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W, E2FGVI_EINVAL, "pred_to_u8: bad arguments");
    hipLaunchKernelGGL(pred_to_u8_kernel, dim3(blocks_for((long long)N * H * W * 3)), dim3(NTH), 0, (hipStream_t)stream, pred, dst, N,
                       H, W, Hp, Wp);
    E2_LAUNCH_CHECK("pred_to_u8");
    return 0;
}

extern "C" int64_t e2fgvi_scene_diff_workspace(int32_t L, int32_t H, int32_t W) {
    if (L < 2 || H < 1 || W < 1 || (int64_t)H * W >= (1LL << 31)) {
        e2fgvi_set_error("scene_diff_workspace: needs L >= 2 frames of H, W >= 1 with H * W < 2^31, got %d x %d x %d", L, H, W);
        return E2FGVI_EINVAL;
    }
    return (int64_t)L * SD_TABLE * (int64_t)sizeof(unsigned);
}

extern "C" int e2fgvi_scene_diff(const uint8_t* frames, int32_t L, int32_t H, int32_t W, void* workspace, int64_t* out, void* stream) {
    E2_REQUIRE(frames && workspace && out, E2FGVI_EINVAL, "scene_diff: null pointer");
    E2_REQUIRE(L >= 2, E2FGVI_EINVAL, "scene_diff: needs at least two frames, got %d", L);
    E2_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31), E2FGVI_EINVAL,
               "scene_diff: frames must have H, W >= 1 and H * W < 2^31, got %d x %d", H, W);
    E2_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)out & 7) == 0, E2FGVI_EINVAL,
               "scene_diff: workspace must be 4-byte aligned and out 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned* hist = (unsigned*)workspace;
    // the tables the atomics add to start at zero on the stream of the launch: the workspace may hold anything
    const hipError_t e = hipMemsetAsync(hist, 0, (size_t)L * SD_TABLE * sizeof(unsigned), st);
    E2_REQUIRE(e == hipSuccess, (int)e, "scene_diff: hipMemsetAsync failed: %s", hipGetErrorString(e));
    // strips of about SD_STRIP bytes, at least one row, inside a cell row (at most ceil(H / 4) rows); a grid row per frame
    long long rps = (SD_STRIP + 3LL * W - 1) / (3LL * W);
    const long long hmax = ((long long)H + 3) / 4;
    rps = rps < 1 ? 1 : (rps > hmax ? hmax : rps);
    const int nstrips = (int)((hmax + rps - 1) / rps);
    const int rc = fb_slabs("scene_diff", L, [&](int l0, unsigned nl) {
        hipLaunchKernelGGL(scene_hist_kernel, dim3(4u * (unsigned)nstrips, nl), dim3(NTH), 0, st, frames + (long long)l0 * H * W * 3,
                           hist + (long long)l0 * SD_TABLE, H, W, (int)rps, nstrips);
    });
    if (rc) return rc;
    for (int l0 = 0; l0 < L - 1; l0 += 1 << 30) {
        const int nl = L - 1 - l0 < (1 << 30) ? L - 1 - l0 : (1 << 30);
        hipLaunchKernelGGL(scene_diff_kernel, dim3((unsigned)nl), dim3(NTH), 0, st, hist + (long long)l0 * SD_TABLE,
                           (long long*)out + l0);
        E2_LAUNCH_CHECK("scene_diff");
    }
    return 0;
}

extern "C" int e2fgvi_overlay_stats(const uint8_t* frames, int32_t L, int32_t H, int32_t W, int32_t* stats, void* stream) {
    E2_REQUIRE(frames && stats, E2FGVI_EINVAL, "overlay_stats: null pointer");
    E2_REQUIRE(L >= 1 && L <= OV_LMAX, E2FGVI_EINVAL, "overlay_stats: needs 1 <= L <= 2^22 frames (the sums are int32), got %d", L);
    E2_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31), E2FGVI_EINVAL,
               "overlay_stats: frames must have H, W >= 1 and H * W < 2^31, got %d x %d", H, W);
    E2_REQUIRE(((uintptr_t)stats & 3) == 0, E2FGVI_EINVAL, "overlay_stats: stats must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    // the chunking, from the shape alone: as many chunks as bring the grid to about OV_BLOCKS workgroups, but no more than leave
    // every chunk OV_CHUNK frames or more (a chunk costs three atomic adds per pixel whatever its length); the kernel splits the
    // frames evenly, so a chunk holds floor or ceil of L / nchunks frames
    const int ntx = (W + OV_TW - 1) / OV_TW, nty = (H + OV_TH - 1) / OV_TH;
    const long long ntiles = (long long)ntx * nty;
    const long long want = (OV_BLOCKS + ntiles - 1) / ntiles, most = L / OV_CHUNK > 1 ? L / OV_CHUNK : 1;
    const int nchunks = (int)(want > most ? most : want);
    const dim3 grid((unsigned)ntiles, (unsigned)nchunks);
    const bool narrow = W < 4;                          // no room for a four-pixel load in a row: the byte-wise instantiation
    if (nchunks == 1) {
        if (narrow) hipLaunchKernelGGL((overlay_stats_kernel<false, true>), grid, dim3(NTH), 0, st, frames, stats, L, H, W, ntx);
        else hipLaunchKernelGGL((overlay_stats_kernel<false, false>), grid, dim3(NTH), 0, st, frames, stats, L, H, W, ntx);
    } else {
        // the planes the atomics add to start at zero on the stream of the launch
        const hipError_t e = hipMemsetAsync(stats, 0, 3 * (size_t)H * W * sizeof(int32_t), st);
        E2_REQUIRE(e == hipSuccess, (int)e, "overlay_stats: hipMemsetAsync failed: %s", hipGetErrorString(e));
        if (narrow) hipLaunchKernelGGL((overlay_stats_kernel<true, true>), grid, dim3(NTH), 0, st, frames, stats, L, H, W, ntx);
        else hipLaunchKernelGGL((overlay_stats_kernel<true, false>), grid, dim3(NTH), 0, st, frames, stats, L, H, W, ntx);
    }
    E2_LAUNCH_CHECK("overlay_stats");
    return 0;
}

extern "C" int e2fgvi_overlay_edges(const int32_t* stats, int32_t L, int32_t H, int32_t W, int32_t g_min, int32_t coherence,
                                    int32_t radius, uint8_t* out, int32_t* count, void* stream) {
    E2_REQUIRE(stats && out && count, E2FGVI_EINVAL, "overlay_edges: null pointer");
    E2_REQUIRE(L >= 1 && L <= OV_LMAX, E2FGVI_EINVAL, "overlay_edges: needs 1 <= L <= 2^22 frames, got %d", L);
    E2_REQUIRE(H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31), E2FGVI_EINVAL,
               "overlay_edges: the map must have H, W >= 1 and H * W < 2^31, got %d x %d", H, W);
    E2_REQUIRE(g_min >= 1, E2FGVI_EINVAL, "overlay_edges: g_min must be >= 1, got %d", g_min);
    E2_REQUIRE(coherence >= 1 && coherence <= 256, E2FGVI_EINVAL, "overlay_edges: coherence must be in [1, 256], got %d", coherence);
    E2_REQUIRE(radius >= 0 && radius <= OV_RMAX, E2FGVI_EINVAL, "overlay_edges: radius must be in [0, %d], got %d", OV_RMAX, radius);
    E2_REQUIRE(((uintptr_t)stats & 3) == 0 && ((uintptr_t)count & 3) == 0, E2FGVI_EINVAL,
               "overlay_edges: stats and count must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(int32_t), st);
    E2_REQUIRE(e == hipSuccess, (int)e, "overlay_edges: hipMemsetAsync failed: %s", hipGetErrorString(e));
    const int ntx = (W + OV_TW - 1) / OV_TW, nty = (H + OV_TH - 1) / OV_TH;
    hipLaunchKernelGGL(overlay_edges_kernel, dim3((unsigned)((long long)ntx * nty)), dim3(NTH), 0, st, stats, L, H, W, g_min, coherence,
                       radius, ntx, out, count);
    E2_LAUNCH_CHECK("overlay_edges");
    return 0;
}

static bool label_size_ok(const char* what, int32_t Hm, int32_t Wm) {
    if (Hm >= 1 && Wm >= 1 && (int64_t)Hm * Wm < (1LL << 31)) return true;
    e2fgvi_set_error("%s: needs Hm, Wm >= 1 with Hm * Wm < 2^31, got %d x %d", what, Hm, Wm);
    return false;
}

extern "C" int64_t e2fgvi_hole_label_workspace(int32_t Hm, int32_t Wm) {
    if (!label_size_ok("hole_label_workspace", Hm, Wm)) return E2FGVI_EINVAL;
    return (int64_t)label_work((long long)Hm * Wm).bytes;
}

extern "C" int e2fgvi_hole_label(const uint8_t* masks, int32_t L, int32_t Hm, int32_t Wm, void* workspace, int32_t* labels,
                                 int32_t* count, void* stream) {
    E2_REQUIRE(workspace && labels && count, E2FGVI_EINVAL, "hole_label: null pointer");
    E2_REQUIRE(L >= 0, E2FGVI_EINVAL, "hole_label: the number of frames must be >= 0, got %d", L);
    if (!label_size_ok("hole_label", Hm, Wm)) return E2FGVI_EINVAL;
    E2_REQUIRE(masks || L == 0, E2FGVI_EINVAL, "hole_label: null masks");
    E2_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)count & 3) == 0, E2FGVI_EINVAL,
               "hole_label: workspace must be 16-byte aligned, labels and count 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long N = (long long)Hm * Wm;
    if (L == 0) {                                       // no frame, no hole
        hipError_t e = hipMemsetAsync(labels, 0, (size_t)N * sizeof(int32_t), st);
        if (e == hipSuccess) e = hipMemsetAsync(count, 0, sizeof(int32_t), st);
        E2_REQUIRE(e == hipSuccess, (int)e, "hole_label: hipMemsetAsync failed: %s", hipGetErrorString(e));
        return 0;
    }
    const LabelWork w = label_work(N);
    int* rank = (int*)((char*)workspace + w.rank);
    unsigned char* foot = (unsigned char*)workspace + w.foot;
    int* counts = (int*)((char*)workspace + w.counts);
    // every launch below writes all it later reads: the workspace may hold anything.  Their number depends on (Hm, Wm) alone.
    hipLaunchKernelGGL(hole_footprint_kernel, dim3(blocks_for((N + 15) / 16)), dim3(NTH), 0, st, masks, L, N, foot);
    E2_LAUNCH_CHECK("hole_label");
    const int ntx = (Wm + LB_TW - 1) / LB_TW, nty = (Hm + LB_TH - 1) / LB_TH;
    hipLaunchKernelGGL(label_tile_kernel, dim3((unsigned)((long long)ntx * nty)), dim3(NTH), 0, st, foot, labels, Hm, Wm, ntx);
    E2_LAUNCH_CHECK("hole_label");
    const long long nrow = (long long)((Hm - 1) / LB_TH) * Wm, total = nrow + (long long)((Wm - 1) / LB_TW) * Hm;
    if (total > 0) {
        hipLaunchKernelGGL(label_border_kernel, dim3(blocks_for(total)), dim3(NTH), 0, st, labels, Hm, Wm, nrow, total);
        E2_LAUNCH_CHECK("hole_label");
    }
    hipLaunchKernelGGL(label_flatten_kernel, dim3((unsigned)w.nblk), dim3(NTH), 0, st, labels, rank, counts, N);
    E2_LAUNCH_CHECK("hole_label");
    hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(NTH), 0, st, counts, w.nblk, count);
    E2_LAUNCH_CHECK("hole_label");
    hipLaunchKernelGGL(label_number_kernel, dim3(blocks_for(N)), dim3(NTH), 0, st, labels, rank, counts, N);
    E2_LAUNCH_CHECK("hole_label");
    return 0;
}

extern "C" int e2fgvi_label_boxes(const int32_t* labels, int32_t Hm, int32_t Wm, int32_t K, int32_t* boxes, void* stream) {
    E2_REQUIRE(K >= 0, E2FGVI_EINVAL, "label_boxes: the number of components must be >= 0, got %d", K);
    if (!label_size_ok("label_boxes", Hm, Wm)) return E2FGVI_EINVAL;
    if (K == 0) return 0;
    E2_REQUIRE(labels && boxes, E2FGVI_EINVAL, "label_boxes: null pointer");
    E2_REQUIRE(((uintptr_t)labels & 3) == 0 && ((uintptr_t)boxes & 3) == 0, E2FGVI_EINVAL,
               "label_boxes: labels and boxes must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(label_boxes_init_kernel, dim3(blocks_for(5LL * K)), dim3(NTH), 0, st, boxes, 5LL * K);
    E2_LAUNCH_CHECK("label_boxes");
    const int ntx = (Wm + LB_TW - 1) / LB_TW, nty = (Hm + LB_TH - 1) / LB_TH;
    hipLaunchKernelGGL(label_boxes_kernel, dim3((unsigned)((long long)ntx * nty)), dim3(NTH), 0, st, labels, Hm, Wm, ntx, K, boxes);
    E2_LAUNCH_CHECK("label_boxes");
    return 0;
}
