/* e2fgvi_hip.h -- C ABI of libe2fgvi_hip.so (MI355X / gfx950 kernels for the E2FGVI forward).
 *
 * The reference (MCG-NKU/E2FGVI) is pure Python: every native instruction it executes is reached
 * through torch / mmcv operator calls.  This header is the replacement for that operator boundary
 * on the inference hot path: one entry point per fused stage.  Each entry
 * cites the reference operator call it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - raw device pointers (fp32 unless stated), explicit int dims, caller-owned buffers: no
 *     allocation, no synchronisation, no host<->device copies inside;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - activations are NHWC ("channels last"): element (n,y,x,c) at ((n*H+y)*W+x)*ld + c, where the
 *     pixel stride `ld` (in floats) may exceed C so that callers can address channel slices;
 *   - returns 0 on success, a negative E2FGVI_E* code on bad arguments, a positive hipError_t on a
 *     launch failure; e2fgvi_last_error() gives the thread-local message;
 *   - re-entrant; no global mutable state.
 */
#ifndef E2FGVI_HIP_H
#define E2FGVI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define E2FGVI_EINVAL (-1)   /* bad argument */
#define E2FGVI_EUNSUP (-2)   /* valid but unsupported configuration */

#define E2FGVI_ACT_NONE 0
#define E2FGVI_ACT_RELU 1
#define E2FGVI_ACT_LRELU 2   /* slope in desc */
#define E2FGVI_ACT_TANH 3
/* ------------------------------------------------------------------------------------------------
 * Byte side of the sliding-window video driver (reference: test.py).
 * uint8 frames [L,H,W,3] and masks stay on the device; all results are bit-exact with the numpy / PIL reference.
 * ------------------------------------------------------------------------------------------------ */
/* test.py:56-69 read_mask: NEAREST resize of [L,Hin,Win] masks to H x W (ytab[H] / xtab[W] = source row / column of
 * every output row / column, built like Pillow's ImagingScaleAffine), binarise (> 0), `iterations` dilations with the
 * 3x3 cross (cv2.dilate, out-of-image pixels ignored).  out: [L,H,W] of 0 / 1. */
int e2fgvi_mask_prepare(const uint8_t* masks, int32_t L, int32_t Hin, int32_t Win, const int32_t* ytab, const int32_t* xtab,
                        uint8_t* out, int32_t H, int32_t W, int32_t iterations, void* stream);
/* e2fgvi_mask_prepare of chosen frames (the frames of one window of video.inpaint_video(region="track")): out [n,H,W], frame l
 * made from frame ids[l] of the L frames of masks; ids is a device table and is range-checked in the kernel -- an id outside
 * [0, L) gives an empty mask. */
int e2fgvi_mask_prepare_ids(const uint8_t* masks, int32_t L, const int32_t* ids, int32_t n, int32_t Hin, int32_t Win,
                            const int32_t* ytab, const int32_t* xtab, uint8_t* out, int32_t H, int32_t W, int32_t iterations,
                            void* stream);
/* test.py:146-165: clip[ti][c][y][x] = (frames[ids[ti]]/255*2-1) * (1 - masks[ids[ti]]), fp32 NCHW [t,3,Hp,Wp], rows /
 * columns beyond H / W mirror the frame (cat([x, flip(x)])[:Hp]). */
int e2fgvi_masked_clip(const uint8_t* frames, const uint8_t* masks, const int32_t* ids, int32_t t, int32_t H, int32_t W,
                       float* clip, int32_t Hp, int32_t Wp, void* stream);
/* test.py:168-179: for the first n frames of pred [*,3,Hp,Wp] (model output in (-1,1)):
 * img = uint8((pred+1)/2*255) * mask + frame * (1-mask); comp[ids[i]] = first[i] ? img : comp*0.5 + img*0.5 (float [L,H,W,3]). */
int e2fgvi_composite(const float* pred, const int32_t* ids, const uint8_t* first, int32_t n, const uint8_t* frames,
                     const uint8_t* masks, float* comp, int32_t H, int32_t W, int32_t Hp, int32_t Wp, void* stream);
/* test.py:97-104,127 resize_frames and core/dataset.py:115: PIL Image.resize(size) of RGB frames (BICUBIC), one separable pass
 * of uint8 [L,H,W,3] -> dst along `axis` (1: H -> n_out rows, 2: W -> n_out columns).  bounds[n_out][2] = (first source index,
 * tap count), coeffs[n_out][ksize] = fixed-point weights with 22 fraction bits (Pillow's precompute_coeffs +
 * normalize_coeffs_8bpc, e2fgvi_amd/video.py::bicubic_tables); dst = clamp((2^21 + sum src * coeff) >> 22, 0, 255).
 * Pillow runs the W pass first and each pass only if that dimension changes. */
int e2fgvi_resample_u8(const uint8_t* src, uint8_t* dst, int32_t L, int32_t H, int32_t W, int32_t n_out, int32_t axis,
                       const int32_t* bounds, const int32_t* coeffs, int32_t ksize, void* stream);
/* The width pass of e2fgvi_resample_u8 (axis 2) over a row window: rows [row0, row0 + rows) of every frame of src [L,H,W,3] ->
 * dst [L,rows,n_out,3] (frames H rows apart in src, `rows` apart in dst).  Pillow's ImagingResample runs the width pass of
 * Image.resize(size, box=...) only over the source rows its height pass reads; the height pass then takes bounds relative to
 * row0.  bounds hold absolute source columns (a box's taps reach past the box, not past the frame) and are clipped to [0, W) in
 * the kernel; ksize >= 1 is the tables' own.  0 <= row0, row0 + rows <= H (E2FGVI_EINVAL). */
int e2fgvi_resample_rows_u8(const uint8_t* src, uint8_t* dst, int32_t L, int32_t H, int32_t W, int32_t n_out, int32_t row0,
                            int32_t rows, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, void* stream);
/* The two passes above on chosen frames: dst frame l (of n) is the pass over frame ids[l] of the L frames of src -- a window's
 * frames are resized straight out of the video, no copy of them at source size is made.  ids is a device table, range-checked in
 * the kernel: an id outside [0, L) gives a frame of zeros. */
int e2fgvi_resample_ids_u8(const uint8_t* src, int32_t L, const int32_t* ids, int32_t n, uint8_t* dst, int32_t H, int32_t W,
                           int32_t n_out, int32_t axis, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, void* stream);
int e2fgvi_resample_rows_ids_u8(const uint8_t* src, int32_t L, const int32_t* ids, int32_t n, uint8_t* dst, int32_t H, int32_t W,
                                int32_t n_out, int32_t row0, int32_t rows, const int32_t* bounds, const int32_t* coeffs, int32_t ksize,
                                void* stream);
/* Bounding box of the hole of a whole video, for a driver that feeds the model only a region around it
 * (video.inpaint_video(region="hole")): masks uint8 [L,Hm,Wm] as test.py:56-69 reads them (any non-zero byte is hole) ->
 * box int32 [4] on the device = (x0, y0, x1, y1), upper ends exclusive; x1 <= x0 when no byte is set (the box is then
 * (0x7f7f7f7f, 0x7f7f7f7f, 0, 0)).  One pass over the masks, 16-byte loads between a byte head and tail per row; box is
 * initialised on `stream` in front of the launch.  L * Hm * Wm == 0 launches nothing and leaves the empty box. */
int e2fgvi_hole_bbox(const uint8_t* masks, int32_t L, int32_t Hm, int32_t Wm, int32_t* box, void* stream);
/* e2fgvi_hole_bbox per frame (video.inpaint_video(region="track") plans one region per window from them): boxes int32 [L][4] on
 * the device, frame l's (x0, y0, x1, y1) in the same convention -- a frame without a hole keeps (0x7f7f7f7f, 0x7f7f7f7f, 0, 0).
 * One pass over the masks, any pitch and base; L == 0 launches nothing. */
int e2fgvi_hole_bbox_frames(const uint8_t* masks, int32_t L, int32_t Hm, int32_t Wm, int32_t* boxes, void* stream);
/* The paste-back that follows test.py:168-179 when test.py:97-104,127 resized the frames on the way in (the reference stops at
 * the resized video; a front end writes the result at source size): for every frame
 *   out = where(Image.fromarray(mask_lo * 255).resize((W, H), NEAREST) != 0, Image.fromarray(lo).resize((W, H)), src)
 * lo [L,h,w,3] finished frames, mask_lo [L,h,w] of 0 / 1 (e2fgvi_mask_prepare's output), src / out [L,H,W,3], all uint8.  One
 * fused launch: tiles of `out` without a hole pixel are copied src -> out, the others recompute Pillow's two BICUBIC passes
 * (width first, its uint8 result clamped, then height) from a patch of lo.  ytab[H] / xtab[W]: NEAREST tables as for
 * e2fgvi_mask_prepare; bounds_x[W][2], coeffs_x[W][ksize_x] and bounds_y[H][2], coeffs_y[H][ksize_y]: tap tables as for
 * e2fgvi_resample_u8; an axis that keeps its size takes the identity -- bounds (o, 1), coeffs 1 << 22, ksize 1 -- as Pillow
 * skips that pass.  Table entries are clipped in the kernel.  out must not overlap src, lo or mask_lo (E2FGVI_EINVAL). */
int e2fgvi_restore_u8(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, uint8_t* out, int32_t L, int32_t h, int32_t w,
                      int32_t H, int32_t W, const int32_t* ytab, const int32_t* xtab, const int32_t* bounds_x,
                      const int32_t* coeffs_x, int32_t ksize_x, const int32_t* bounds_y, const int32_t* coeffs_y, int32_t ksize_y,
                      void* stream);
/* e2fgvi_restore_u8 confined to a box of the frame -- left <= x < left + Bw, upper <= y < upper + Bh, inside W x H
 * (E2FGVI_EINVAL otherwise): out = src outside the box and, on the sub-image src[upper:upper+Bh, left:left+Bw], the three lines
 * above with (Bw, Bh) for (W, H).  The tables index box-relative pixels: ytab[Bh], xtab[Bw], bounds_x[Bw][2], coeffs_x[Bw][ksize_x],
 * bounds_y[Bh][2], coeffs_y[Bh][ksize_y].  The same kernel (e2fgvi_restore_u8 is the box (0, 0, W, H)): tiles of `out` that lie
 * outside the box are copied like tiles without a hole pixel. */
int e2fgvi_restore_box_u8(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, uint8_t* out, int32_t L, int32_t h,
                          int32_t w, int32_t H, int32_t W, int32_t left, int32_t upper, int32_t Bw, int32_t Bh, const int32_t* ytab,
                          const int32_t* xtab, const int32_t* bounds_x, const int32_t* coeffs_x, int32_t ksize_x,
                          const int32_t* bounds_y, const int32_t* coeffs_y, int32_t ksize_y, void* stream);
/* e2fgvi_restore_box_u8 with test.py:175-179's blend of overlapping windows moved to source size: lo [n,h,w,3] / mask_lo [n,h,w]
 * are the finished frames of ONE window, frame i belonging to frame ids[i] of the L frames of src [L,H,W,3] uint8 and acc
 * [L,H,W,3] float.  With img = the frame e2fgvi_restore_box_u8 would write for it (the same tables, the same arithmetic),
 *   acc[ids[i]] = first[i] ? img : acc[ids[i]] * 0.5f + img * 0.5f
 * on the pixels of the touched rectangle (touch_left, touch_upper) + Tw x Th, which must contain the box and lie inside the frame
 * (E2FGVI_EINVAL otherwise); between the box and the rim of that rectangle img is src.  Nothing else of acc is read or written and
 * only the tiles the rectangle reaches are launched.  ids / first are device tables; an id outside [0, L) is skipped.  acc must
 * not overlap any input (E2FGVI_EINVAL). */
int e2fgvi_restore_blend(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, const int32_t* ids, const uint8_t* first,
                         float* acc, int32_t n, int32_t L, int32_t h, int32_t w, int32_t H, int32_t W, int32_t left, int32_t upper,
                         int32_t Bw, int32_t Bh, int32_t touch_left, int32_t touch_upper, int32_t Tw, int32_t Th, const int32_t* ytab,
                         const int32_t* xtab, const int32_t* bounds_x, const int32_t* coeffs_x, int32_t ksize_x,
                         const int32_t* bounds_y, const int32_t* coeffs_y, int32_t ksize_y, void* stream);
/* The feathered paste: e2fgvi_restore_box_u8 with the edge of the pasted mask ramped into the source over `feather` = r pixels,
 * 1 <= r <= 16 (E2FGVI_EINVAL otherwise; r = 0 is e2fgvi_restore_box_u8 itself).  In box-relative pixels, everything outside the
 * box counting as 0, with up = BICUBIC(lo) and M = NEAREST(mask_lo) as above:
 *   D(p) = 1 iff some q with |q - p|_inf <= r has M(q) = 1;   c(p) = #{q in the box : |q - p|_inf <= r, D(q) = 1};
 *   n(p) = #{q in the box : |q - p|_inf <= r};   out = (c * up + (n - c) * src + n / 2) / n  per byte (integers), out = src outside.
 * A pixel of M has c = n and gets `up` itself; a pixel farther than 2 r from M is src; the ramp is cut at the box's edge. */
int e2fgvi_restore_feather_u8(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, uint8_t* out, int32_t L, int32_t h,
                              int32_t w, int32_t H, int32_t W, int32_t left, int32_t upper, int32_t Bw, int32_t Bh,
                              const int32_t* ytab, const int32_t* xtab, const int32_t* bounds_x, const int32_t* coeffs_x,
                              int32_t ksize_x, const int32_t* bounds_y, const int32_t* coeffs_y, int32_t ksize_y, int32_t feather,
                              void* stream);
/* e2fgvi_restore_blend with img = the frame e2fgvi_restore_feather_u8 would write; the same checks plus 1 <= feather <= 16 */
int e2fgvi_restore_feather_blend(const uint8_t* lo, const uint8_t* mask_lo, const uint8_t* src, const int32_t* ids,
                                 const uint8_t* first, float* acc, int32_t n, int32_t L, int32_t h, int32_t w, int32_t H, int32_t W,
                                 int32_t left, int32_t upper, int32_t Bw, int32_t Bh, int32_t touch_left, int32_t touch_upper,
                                 int32_t Tw, int32_t Th, const int32_t* ytab, const int32_t* xtab, const int32_t* bounds_x,
                                 const int32_t* coeffs_x, int32_t ksize_x, const int32_t* bounds_y, const int32_t* coeffs_y,
                                 int32_t ksize_y, int32_t feather, void* stream);
/* ndarray.astype(float32) of uint8 values: the accumulator above starts as the source frames */
int e2fgvi_u8_to_float(const uint8_t* src, float* dst, int64_t n, void* stream);
/* ndarray.astype(uint8) of the blended frames (truncation) */
int e2fgvi_float_to_u8(const float* src, uint8_t* dst, int64_t n, void* stream);
/* model output [N,3,Hp,Wp] in (-1,1) -> uint8 NHWC [N,H,W,3] = uint8((pred+1)/2*255): the form the clip-sharded runner
 * gathers over xGMI (4x fewer bytes than fp32). */
int e2fgvi_pred_to_u8(const float* pred, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t Hp, int32_t Wp, void* stream);
/* test.py:152 (selected_imgs = imgs[:1, neighbor_ids + ref_ids]) for a driver that keeps per-frame results instead of
 * recomputing them in every window (video.inpaint_video(reuse=True)): window[i] = cache[ids[i]], i < n, for slabs of
 * slab_bytes bytes each -- cache [slots][slab], window [n][slab], any element type: encoder features [h,w,128] in fp32 /
 * bf16 / fp16 and flows [h,w,2] alike.  slab_bytes a multiple of 4; 16-byte loads and stores whenever slab_bytes and both
 * bases are multiples of 16 (8-byte ones at multiples of 8).  ids are device int32 and nothing is read on the host; an id
 * outside [0, slots) zero-fills its window slab (gather) or is skipped (scatter).  n <= 65535. */
int e2fgvi_gather_slabs(const void* cache, int32_t slots, const int32_t* ids, int32_t n, int64_t slab_bytes, void* window,
                        void* stream);
/* the mirror: cache[ids[i]] = rows[i] -- newly encoded frames / newly computed flows into their cache slots (ids distinct) */
int e2fgvi_scatter_slabs(const void* rows, const int32_t* ids, int32_t n, int64_t slab_bytes, void* cache, int32_t slots,
                         void* stream);
/* Scene cuts (video.detect_cuts; test.py treats its clip as one shot): the block-histogram difference of adjacent frames, in
 * integers only.  frames uint8 [L,H,W,3]; for frame t and pixel (x, y) with bytes R, G, B
 *   Y = (77 R + 150 G + 29 B + 128) >> 8 (0..255),  bin = Y >> 2 (64 bins),  cell = ((4 y) / H) * 4 + (4 x) / W (a 4 x 4 grid,
 *   integer division; cells are empty when H < 4 or W < 4),  hist[t][cell][bin] = number of such pixels,
 *   out[t] = sum over cell, bin of |hist[t][cell][bin] - hist[t+1][cell][bin]|,  0 <= t < L - 1:  0 .. 2 H W.
 * out int64 [L-1] on the device.  One pass over the frames (16-byte loads between byte heads and tails: any base, any row pitch)
 * builds the tables in `workspace` -- e2fgvi_scene_diff_workspace(L,H,W) bytes, caller-owned, 4-byte aligned, its contents on
 * entry do not matter: it is zeroed on `stream` -- with integer atomics, a second launch sums the differences per pair: exact,
 * and the same in every run.  L >= 2, H, W >= 1, H * W < 2^31 (E2FGVI_EINVAL otherwise, from both entries). */
int64_t e2fgvi_scene_diff_workspace(int32_t L, int32_t H, int32_t W);
int e2fgvi_scene_diff(const uint8_t* frames, int32_t L, int32_t H, int32_t W, void* workspace, int64_t* out, void* stream);
/* Connected components of the hole's footprint (video.hole_regions / inpaint_video(region="holes"): holes far apart get a crop
 * region each).  masks uint8 [L,Hm,Wm], any non-zero byte is hole:
 *   U[y][x] = 1 iff masks[l][y][x] != 0 for some l;   labels[y][x] = 0 where U is 0, elsewhere the number 1 .. K of the pixel's
 *   8-connected component of U, the components numbered in raster order of their first pixel (smallest y * Wm + x);  count[0] = K.
 * The numbering is canonical: the integers do not depend on the order in which threads or atomics ran, and they are the ones
 * scipy.ndimage.label(U, np.ones((3, 3))) gives.  labels int32 [Hm][Wm] and count int32 [1] on the device, 4-byte aligned.
 * L == 0 (masks may be null) or masks without a hole pixel give labels of 0 and K = 0.  Hm, Wm >= 1 and Hm * Wm < 2^31
 * (E2FGVI_EINVAL otherwise, from all three entries).  `workspace`: e2fgvi_hole_label_workspace(Hm, Wm) bytes, caller-owned,
 * 16-byte aligned (an int32 rank per pixel, the footprint bytes, a counter per 1024 pixels, each part a multiple of 16 bytes),
 * its contents on entry do not matter.  A fixed number of launches for a given (Hm, Wm), no host read: the OR over
 * the frames, a union-find per tile in LDS, a lock-free merge across the tile borders, flatten, a scan of the roots, the dense
 * numbers.  The forest keeps parent[i] <= i and only ever lowers an entry (atomicMin), so no thread waits for another. */
int64_t e2fgvi_hole_label_workspace(int32_t Hm, int32_t Wm);
int e2fgvi_hole_label(const uint8_t* masks, int32_t L, int32_t Hm, int32_t Wm, void* workspace, int32_t* labels, int32_t* count,
                      void* stream);
/* The table of the components above: boxes int32 [K][5] on the device, boxes[k-1] = (x0, y0, x1, y1, area) of the pixels with
 * labels[y][x] == k, upper ends exclusive as for e2fgvi_hole_bbox.  K >= 0 is what e2fgvi_hole_label counted (K == 0 launches
 * nothing); a label outside [1, K] is skipped.  Runs and tiles are reduced in registers and LDS in front of the global atomics. */
int e2fgvi_label_boxes(const int32_t* labels, int32_t Hm, int32_t Wm, int32_t K, int32_t* boxes, void* stream);
/* Static overlays (video.overlay_mask: the mask of a station logo, a watermark or a fixed caption, from the frames themselves), in
 * integers only.  frames uint8 [L,H,W,3]; with the luma of the scene detector and borders clamped, per frame
 *   Y = (77 R + 150 G + 29 B + 128) >> 8,
 *   gx = Y[y][min(x+1, W-1)] - Y[y][max(x-1, 0)],   gy = Y[min(y+1, H-1)][x] - Y[max(y-1, 0)][x],
 * and over the L frames, per pixel,  Sx = sum gx,  Sy = sum gy,  M = sum (|gx| + |gy|):
 *   stats int32 [3][H][W] = (Sx, Sy, M) on the device, 4-byte aligned, its contents on entry do not matter.
 * An overlay's contour keeps the direction of its gradient frame after frame, also when the overlay is half transparent, so
 * |sum G| stays close to sum |G|; the gradients of moving content change direction at a fixed pixel and cancel.
 * One pass over the frames; the frames are split into chunks by a rule of (L, H, W) alone and the chunks meet with integer
 * atomics: exact, and the same in every run.  1 <= L <= 2^22 (M <= 510 L fits int32), H, W >= 1, H * W < 2^31 (E2FGVI_EINVAL
 * otherwise). */
int e2fgvi_overlay_stats(const uint8_t* frames, int32_t L, int32_t H, int32_t W, int32_t* stats, void* stream);
/* The persistent edges of those sums, dilated.  A pixel is a persistent edge when
 *   M >= g_min * L   and   256 * (|Sx| + |Sy|) >= coherence * M        (both in 64 bits: the left side passes 2^31 from L = 16449 on);
 * out uint8 [H][W] = D, 1 where a persistent edge lies in the pixel's (2 radius + 1) x (2 radius + 1) box and 0 elsewhere -- the
 * box is clipped at the frame: outside counts as no edge -- and count int32 [1] (4-byte aligned) = the number of set pixels of D,
 * both on the device, one launch.  L as for e2fgvi_overlay_stats (the number of frames the sums were taken over), g_min >= 1,
 * 1 <= coherence <= 256, 0 <= radius <= 16 (E2FGVI_EINVAL otherwise). */
int e2fgvi_overlay_edges(const int32_t* stats, int32_t L, int32_t H, int32_t W, int32_t g_min, int32_t coherence, int32_t radius,
                         uint8_t* out, int32_t* count, void* stream);

/* Pixel formats (video.yuv420_to_rgb / rgb_to_yuv420, inpaint_video(pixel_format=)): 8-bit 4:2:0 YUV frames as decoders hand them
 * over, in place of the chain of float torch expressions -- several passes over source-size frames, two roundings and a chroma
 * resampling of every byte -- a caller of the RGB-only driver has to write around it.  A frame is 3 H W / 2 contiguous bytes, H and W
 * even: H rows of W luma bytes, then E2FGVI_YUV_NV12: H/2 rows of W/2 interleaved (U, V) pairs; E2FGVI_YUV_I420: the H/2 x W/2 U
 * plane, then the V plane.  yuv uint8 [L][3H/2][W], rgb uint8 [L][H][W][3], both on the device, neither need be aligned (8-byte
 * loads and stores where W % 8 == 0 and every base is a multiple of 8, bytes otherwise).  All arithmetic is int32, >> the floor
 * shift, clip to [0, 255].  Chroma at pixel (y, x) from the plane C[j][i], indices clamped to the plane:
 *   E2FGVI_CHROMA_NEAREST: C' = C[y >> 1][x >> 1];
 *   E2FGVI_CHROMA_LEFT (MPEG-2 / H.264 siting): C' = (sum wv wh C + 4) >> 3 with horizontal taps {i: 2} at x = 2i and
 *   {i: 1, i+1: 1} at x = 2i+1, vertical taps {j-1: 1, j: 3} at y = 2j and {j: 3, j+1: 1} at y = 2j+1.
 * coef: HOST int32 [6] = (cy, crv, cgu, cgv, cbu, yo) in Q14 (video.yuv_coefficients), read before the call returns:
 *   yy = cy (Y - yo), u = U' - 128, v = V' - 128;
 *   R = clip((yy + crv v + 8192) >> 14), G = clip((yy - cgu u - cgv v + 8192) >> 14), B = clip((yy + cbu u + 8192) >> 14).
 * Odd H or W, an unknown layout or chroma mode: E2FGVI_EINVAL; L H W = 0 launches nothing; H W < 2^31. */
#define E2FGVI_YUV_NV12 0
#define E2FGVI_YUV_I420 1
#define E2FGVI_CHROMA_LEFT 0
#define E2FGVI_CHROMA_NEAREST 1
int e2fgvi_yuv420_to_rgb(const uint8_t* yuv, uint8_t* rgb, int32_t L, int32_t H, int32_t W, int32_t layout, int32_t chroma,
                         const int32_t* coef, void* stream);
/* The way back, replacing the same chain of float expressions on the result.  coef: HOST int32 [10] = (yr, yg, yb, ur, ug, ub, vr,
 * vg, vb, yo) in Q14; with SR, SG, SB the sums over the four pixels of block (j, i) -- the box average, one rounding:
 *   Y(y, x) = clip(yo + ((yr R + yg G + yb B + 8192) >> 14)),
 *   U(j, i) = clip(128 + ((ur SR + ug SG + ub SB + 32768) >> 16)),   V likewise with (vr, vg, vb).
 * like / like_rgb (both or neither; NULL: the plain encode): the caller's YUV frames [L][3H/2][W] and what they decoded to
 * [L][H][W][3].  A pixel is unchanged when its three bytes of rgb equal those of like_rgb; an unchanged pixel's luma byte is like's,
 * and a chroma sample whose four pixels are all unchanged is like's pair of bytes; everything else is encoded from rgb (an
 * unchanged pixel in a changed block keeps its luma and gets the block's new chroma).  One launch either way, every byte of yuv
 * written once; yuv must not overlap an input.  Errors as above. */
int e2fgvi_rgb_to_yuv420(const uint8_t* rgb, const uint8_t* like_rgb, const uint8_t* like, uint8_t* yuv, int32_t L, int32_t H,
                         int32_t W, int32_t layout, const int32_t* coef, void* stream);

/* ------------------------------------------------------------------------------------------------
 * evaluate.py metrics (core/metrics.py:20-56): per image pair of fp32 NHWC [N,H,W,3] frames in
 * [0,255]: out[2n] = PSNR (inf when identical), out[2n+1] = SSIM as skimage compare_ssim(data_range=255,
 * multichannel=True, win_size) computes it (uniform window, sample covariance, K1 .01, K2 .03, crop (win-1)/2).
 * fp64 like the reference.  workspace: e2fgvi_psnr_ssim_workspace(N,H,W) bytes, caller-owned.
 * N <= 65535 pairs per call (they ride on the grid's y axis); more is E2FGVI_EINVAL.
 * ------------------------------------------------------------------------------------------------ */
int64_t e2fgvi_psnr_ssim_workspace(int32_t N, int32_t H, int32_t W);
int e2fgvi_psnr_ssim(const float* img1, const float* img2, int32_t N, int32_t H, int32_t W, int32_t win_size,
                     void* workspace, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * E_warp, the flow-warping temporal error of the paper's result table (SURVEY.md lines 242-243; evaluate.py:142-151 saves its
 * frames "for evaluating warping errors"), after Lai et al., ECCV 2018, with the occlusion test of Ruder et al. 2016.
 *   frames [L,H,W,3]  of frame_dtype: E2FGVI_F32 (finite, in [0,255]) or E2FGVI_U8
 *   fwd    [L-1,H,W,2] fp32: fwd[t] = flow from frame t to t+1 on frame t's grid, pixels, channel 0 = x
 *   bwd    [L-1,H,W,2] fp32: bwd[t] = flow from frame t+1 to t on frame t+1's grid
 *   valid  [L,H,W] uint8 or NULL
 * For pair t, A = frames[t], B = frames[t+1], f = fwd[t], g = bwd[t], all arithmetic fp64, pixel p = (x, y):
 *   q = (x + f_x(p), y + f_y(p));  inside = 0 <= q_x <= W-1 and 0 <= q_y <= H-1 (decided in floating point, before any
 *       conversion to an integer: a flow of 1e30 is simply outside);
 *   bil(T, q) = the 4-corner bilinear sample, corners outside the image contribute 0 (flow_comp.py:345-383 with
 *       padding_mode='zeros': grid_sample(align_corners=True));  g_w = bil(g, q), B_w = bil(B, q);
 *   occluded        |f + g_w|^2 > 0.01 (|f|^2 + |g_w|^2) + 0.5;
 *   motion boundary |dx f|^2 + |dy f|^2 > 0.01 |f|^2 + 0.002 with the forward differences dx f = f(x+1,y) - f(x,y),
 *       dy f = f(x,y+1) - f(x,y), a difference being 0 on the last column / row;
 *   M(p) = inside, not occluded, not on a motion boundary, valid[t](p) != 0 (when valid is given) and f(p), f at the right and
 *       lower neighbour used above and g_w all finite -- excluded pixels are dropped by select, never multiplied by 0;
 *   n_t = sum M,  e_t = sum_p M(p) sum_c ((A_c - B_w,c) / 255)^2 / n_t,  e_t = 0 when n_t = 0.
 * out: float64 [L-1][2] = (e_t, n_t); the video's score is the mean of e_t over the pairs with n_t > 0.  One launch over all
 * pairs (one thread per pixel, one (sum, count) partial per block) and one that sums each pair's partials in a fixed order: no
 * floating-point atomics, two runs return the same bits; the counts are exact.  workspace: e2fgvi_warp_error_workspace(L,H,W)
 * bytes, caller-owned, 8-byte aligned.  H * W < 2^31 - 256.
 * ------------------------------------------------------------------------------------------------ */
#define E2FGVI_U8 4          /* uint8 frames (e2fgvi_warp_error only) */
int64_t e2fgvi_warp_error_workspace(int32_t L, int32_t H, int32_t W);
int e2fgvi_warp_error(const void* frames, int32_t frame_dtype, const float* fwd, const float* bwd, const uint8_t* valid, int32_t L,
                      int32_t H, int32_t W, void* workspace, double* out, void* stream);
/* Masks from keyframes (video.propagate_masks, inpaint_video(mask_keys=)): one step of pulling a binary mask along those flows.
 *   planes [2,L,H,W] uint8 of 0 / 1, read and written: plane 0 is carried forward in time, plane 1 backward
 *   fwd, bwd [L-1,H,W,2] fp32 as above, 8-byte aligned;  jobs int32 [n][2] = (pair t, dir) on the device
 * dir 0 reads plane 0 frame t and writes plane 0 frame t+1 with the pull flow g = bwd[t] and the check flow c = fwd[t];
 * dir 1 reads plane 1 frame t+1 and writes plane 1 frame t with g = fwd[t] and c = bwd[t].  One launch runs all n jobs (in slabs
 * of 65535); within a call no job may write a frame of a plane that another job reads or writes (video.plan_mask_chains); a job
 * outside [0, L-1) x {0, 1} writes nothing.  Destination pixel p = (x, y), source mask M, fp64 on the fp32 / uint8 inputs in the
 * order written, no fused multiply-add:
 *   q = (x + g_x(p), y + g_y(p));  inside = g(p) finite, 0 <= q_x <= W-1 and 0 <= q_y <= H-1 (in floating point, before any
 *       conversion to an integer);  s = bil(M, q), c_w = bil(c, q) with the sampler above, corners added in the order (y0, x0),
 *       (y0, x0+1), (y0+1, x0), (y0+1, x0+1);
 *   inconsistent = c_w not finite, or  sx sx + sy sy > 0.01 ((g_x g_x + g_y g_y) + (c_wx c_wx + c_wy c_wy)) + 0.5,  s = g + c_w;
 *   dst(p) = 1 iff inside and s >= 0.5 and (check == 0 or not inconsistent): a tie s == 0.5 is inside the mask.
 * Excluded pixels are dropped by select; c is gathered only for pixels that passed `inside` and s >= 0.5.  No atomics: the same
 * inputs give the same bits.  L >= 2, n, H, W >= 0, check in {0, 1}, H * W < 2^31 - 256 (E2FGVI_EINVAL otherwise); n == 0 or
 * H * W == 0 returns 0 without a launch and without looking at the pointers; a null pointer with work is E2FGVI_EINVAL. */
int e2fgvi_mask_track_step(uint8_t* planes, const float* fwd, const float* bwd, const int32_t* jobs, int32_t n, int32_t L, int32_t H,
                           int32_t W, int32_t check, void* stream);
/* Dust and dirt (video.detect_defects, inpaint_video(masks_u8="defects")): a motion-compensated temporal spike test over those
 * flows, in envelope form -- exact integers after one floor.
 *   frames uint8 [L,H,W,3];  fwd, bwd [L-1,H,W,2] fp32 as above, 8-byte aligned;  ids int32 [n] on the device: the centre frames
 *   to do, distinct;  Y = (77 R + 150 G + 29 B + 128) >> 8, the scene detector's luma, formed where the RGB bytes are gathered.
 * Centre frame t with 1 <= t <= L-2 (an id outside writes nothing), pixel p = (x, y), neighbour A = frame t-1 with g = bwd[t-1],
 * neighbour B = frame t+1 with g = fwd[t], both on frame t's grid.  Per neighbour N:
 *   q = (x + g_x(p), y + g_y(p)) in fp64;  inside_N = g(p) finite, 0 <= q_x <= W-1 and 0 <= q_y <= H-1 (in floating point, before
 *       any conversion to an integer: 1e30 or a NaN is simply outside);  (x0, y0) = floor(q);
 *   lo_N, hi_N = min, max of Y_N over the pixels (x0 + i, y0 + j) with -slack <= i, j <= 1 + slack that lie in the frame.
 *   cand[t](p) = 1 iff inside_A and inside_B and ((Y_t(p) > hi_A + tau and Y_t(p) > hi_B + tau) or
 *                                                 (Y_t(p) < lo_A - tau and Y_t(p) < lo_B - tau)), else 0: strict comparisons,
 *       brighter than both envelopes or darker than both -- one neighbour is never enough.
 * The candidate entry writes cand uint8 [L,H,W] for the listed frames only, one launch over all n frames (in slabs of 65535).
 * The cleaning entry reads cand (any non-zero byte is a candidate) of the listed frames and writes for them
 *   n3(p) = the number of candidates in the 3 x 3 box around p, clipped at the frame, p included;  K = cand and n3 >= support;
 *   D(p) = 1 iff some K lies in the (2 radius + 1)-pixel box around p, clipped at the frame;  out[t] = 255 D;
 * and counts int32 [L]: sum D for a listed frame and 0 for every other (the entry clears all L first; integer atomics, exact).
 * Support test and dilation are one launch over a (2 radius + 3)-pixel stencil staged in LDS.  The same inputs give the same
 * bits in every run; nothing is read on the host.  n, L, H, W >= 0, L >= 3 when n > 0, H * W < 2^31 - 256, tau in [0, 254],
 * slack in [0, 2], support in [1, 9], radius in [0, 16] (E2FGVI_EINVAL otherwise, from the arguments alone); n == 0 or
 * H * W == 0 returns 0 without a launch and without looking at the pointers; a null or misaligned pointer with work is
 * E2FGVI_EINVAL (fwd, bwd 8-byte, ids and counts 4-byte aligned). */
int e2fgvi_defect_candidates(const uint8_t* frames, const float* fwd, const float* bwd, const int32_t* ids, int32_t n, int32_t L,
                             int32_t H, int32_t W, int32_t tau, int32_t slack, uint8_t* cand, void* stream);
int e2fgvi_defect_clean(const uint8_t* cand, const int32_t* ids, int32_t n, int32_t L, int32_t H, int32_t W, int32_t support,
                        int32_t radius, uint8_t* out, int32_t* counts, void* stream);
/* Real pixels for restored holes (video.propagate_pixels): for every hole pixel, where in which frame its colour can be seen,
 * carried along those flows, and one bilinear read of that colour at the end.  Coordinates travel, not colours.
 *   hole   uint8 [L,H,W] of 0 / 1;  fwd, bwd [L-1,H,W,2] fp32 as above, 8-byte aligned;  jobs int32 [n][2] = (pair t, dir)
 *   age    uint8 [2,L,H,W]: 255 = not reached, 0 = a known pixel, a = reached after a steps; the caller sets both planes to
 *          255 * hole.  Plane 0 travels forward in time, plane 1 backward.
 *   origin fp32 [2,L,H,W,2] = (x, y), 8-byte aligned, uninitialised: meaningful only where 1 <= age <= 254 (a pixel of age 0 is
 *          its own origin).  The origin of a reached pixel of frame d lies in frame d - age (plane 0) or d + age (plane 1).
 * The step.  dir 0: source frame s = t, destination d = t+1, pull flow g = bwd[t], check flow c = fwd[t], plane 0;  dir 1: s = t+1,
 * d = t, g = fwd[t], c = bwd[t], plane 1.  One launch runs all n jobs (in slabs of 65535); within a call no job may write a frame of
 * a plane that another job reads or writes (video.plan_pixel_chains); a job outside [0, L-1) x {0, 1} writes nothing.  For a
 * destination pixel p = (x, y) with hole[d](p) == 1 -- no other pixel is touched -- fp64 on the fp32 / uint8 inputs in the order
 * written, no fused multiply-add:
 *   q = (x + g_x(p), y + g_y(p));  inside = g(p) finite, 0 <= q_x <= W-1 and 0 <= q_y <= H-1 (in floating point, before any
 *       conversion to an integer);
 *   c* = (floor(q_x + 0.5), floor(q_y + 0.5)), the nearest pixel, a half goes up;  a = age[dir, s](c*);
 *   c_w = bil(c, q) with the sampler and the corner order of e2fgvi_mask_track_step, and `inconsistent` exactly its test;
 *   reached = inside and a != 255 and a + 1 <= reach and (check == 0 or not inconsistent);
 *   reached:  age[dir, d](p) = a + 1 and origin[dir, d](p) = O_c + (q - c*) per component, the difference first, then the sum, the
 *       sum rounded to fp32 by the store;  O_c = c* when a == 0, else origin[dir, s](c*) widened to fp64;
 *   otherwise age[dir, d](p) = 255.
 * A thread owns four consecutive pixels and is done after one dword when none of their hole bytes is set.  L >= 2, n, H, W >= 0,
 * reach in [1, 254], check in {0, 1}, H * W < 2^31 - 256 (E2FGVI_EINVAL otherwise); n == 0 or H * W == 0 returns 0 without a launch
 * and without looking at the pointers; a null or misaligned pointer with work is E2FGVI_EINVAL (fwd, bwd, origin 8-byte, jobs
 * 4-byte aligned).
 * The fill, one launch over all frames.  src uint8 [L,H,W,3]: the frames the colours are read from;  out uint8 [L,H,W,3]: read and
 * written, only hole pixels are written;  source uint8 [L,H,W] or NULL.  For a pixel p with hole[t](p) == 1:
 *   the candidates are the two planes in the order of their ages at p, a tie goes to plane 0, a plane of age 255 is none;
 *   a candidate of age a names the frame f = t - a (plane 0) or t + a (plane 1) and the point O = origin[plane, t](p) (O = p when
 *       a == 0);  it holds iff 0 <= f < L, O is finite with 0 <= O_x <= W-1 and 0 <= O_y <= H-1, and every one of the four
 *       bilinear corners of O with a non-zero weight lies in the image and has hole[f] == 0;
 *   the first candidate that holds gives out[t](p)[ch] = min(255, floor(bil(src[f], O)[ch] + 0.5)); when none holds out keeps its
 *       bytes;
 *   source[t](p) = 1 (plane 0), 2 (plane 1) or 3 (left as it was), and 0 where hole is not 1.
 * L, H, W >= 0, H * W < 2^31 - 256 (E2FGVI_EINVAL otherwise); L == 0 or H * W == 0 returns 0 without a launch and without looking at
 * the pointers; a null pointer with work (source excepted) or a misaligned origin is E2FGVI_EINVAL.  Neither entry has atomics: the
 * same inputs give the same bits in every run. */
int e2fgvi_pixel_track_step(const uint8_t* hole, uint8_t* age, float* origin, const float* fwd, const float* bwd, const int32_t* jobs,
                            int32_t n, int32_t L, int32_t H, int32_t W, int32_t reach, int32_t check, void* stream);
int e2fgvi_pixel_fill(const uint8_t* src, const uint8_t* hole, const uint8_t* age, const float* origin, uint8_t* out, uint8_t* source,
                      int32_t L, int32_t H, int32_t W, void* stream);
/* Film grain for restored holes (video.match_grain): the grain of the caller's frames is measured block by block, turned into a
 * table of strengths per scene, luma and channel, and synthetic grain of that strength is laid over the pixels a restoration
 * filled in.  All arithmetic is integer.  Y = (77 R + 150 G + 29 B + 128) >> 8, the scene detector's luma.
 *   frames, filled, out uint8 [L,H,W,3];  hole, where uint8 [L,H,W], non-zero = set;  scene_of int32 [L] on the device.
 * Blocks.  Hb = max(0, (H - 2) / 8), Wb likewise; block (by, bx) covers y in [1 + 8 by, 9 + 8 by), x in [1 + 8 bx, 9 + 8 bx).
 *   r = 4 p - p(x-1) - p(x+1) - p(y-1) - p(y+1) per pixel and channel;  energy[t,by,bx,c] = sum r^2 over the 64 pixels (<= 6.7e7);
 *   band[t,by,bx] = (sum Y >> 6) >> 5 in 0..7, or 255 = not measured when one of the block's 192 bytes is 0 or 255 (clipped) or a
 *   pixel of its 10 x 10 footprint y in [8 by, 8 by + 10), x in [8 bx, 8 bx + 10) has hole != 0 (hole may be NULL: none has).
 *   energy int32 [L,Hb,Wb,3] and band uint8 [L,Hb,Wb] are written whole, every entry once (energy also where band is 255).
 * Levels (ops.grain_lut, between the two launches, on the device; GRAIN_MIN_BLOCKS = 32).  A frame belongs to scene scene_of[t]
 * when that is in [0, n_scenes), to none otherwise.  Per scene s and channel c, over the measured blocks (band != 255) of its
 * frames: quartile(list) = the element at index (n - 1) / 4 of the n energies in ascending order.
 *   G[s,c] = quartile of all measured blocks of the scene; fewer than 32 of them: every level of the scene is 0.
 *   E[s,k,c] = quartile of those with band == k when they are >= 32; otherwise that of the nearest band that has 32 (a tie: the
 *       darker band), and G[s,c] when no band has;  then E is clamped to [G >> 2, G << 2].
 *   S[s,k,c] = isqrt(E * 196611 * 19 / (1280 * 16)), integer division:  1280 = 64 pixels x 20, the variance gain of r on white
 *       noise;  19 / 16 undoes the bias of the quartile;  196611 = (2^32 - 1) / 21845 with 21845 the variance of n below.
 *   lut[s,y,c] for y in 0..255, linear between the band centres 16 + 32 k:  u = y - 16;  u < 0: S[0];  u >= 224: S[7];  otherwise
 *       k = u >> 5, f = u & 31, (S[k] (32 - f) + S[k+1] f + 16) >> 5;  then lut = min((lut q8 + 128) >> 8, GRAIN_SCALE_MAX = 2^22 - 1)
 *       with q8 = round(256 strength).
 * Synthesis, counter-based.  mix(x) in uint32: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *   h = mix(mix(seed + 0x9E3779B9 t) ^ ((y W + x) 3 + c)), everything mod 2^32;  n = the sum of h's four bytes - 510: zero mean,
 *   variance 21845.  Where where != 0 and frame t has a scene:
 *   out = clamp(filled + ((n g + 32768) >> 16), 0, 255), the shift arithmetic, g = lut[scene_of[t], Y(filled pixel), c] read as 0
 *   when negative and as GRAIN_SCALE_MAX when larger;  every other byte of out is filled's.  out may be filled itself.
 * No atomics in either entry: the same inputs give the same bits in every run.  L, H, W, n_scenes >= 0, H * W < 2^31 - 256
 * (E2FGVI_EINVAL otherwise); L == 0 or no block (blocks), L == 0 or H * W == 0 (apply) returns 0 without a launch and without
 * looking at the pointers; a null pointer with work (hole excepted, and lut when n_scenes == 0) or an energy, lut or scene_of that
 * is not 4-byte aligned is E2FGVI_EINVAL. */
int e2fgvi_grain_blocks(const uint8_t* frames, const uint8_t* hole, int32_t L, int32_t H, int32_t W, int32_t* energy, uint8_t* band,
                        void* stream);
int e2fgvi_grain_apply(const uint8_t* filled, const uint8_t* where, const int32_t* lut, const int32_t* scene_of, int32_t n_scenes,
                       uint32_t seed, int32_t L, int32_t H, int32_t W, uint8_t* out, void* stream);
/* Vertical line scratches (video.detect_line_scratches): a column that stands out against both its sides, over most of the frame's
 * height, frame after frame -- the persistent film defect a temporal test cannot see.  All arithmetic is integer.
 *   frames uint8 [L,H,W,3];  Y = (77 R + 150 G + 29 B + 128) >> 8, the scene detector's luma;  scene int32 [L] on the device: two
 *   frames are in one scene when their entries are equal.  Parameters rows, tau, gap, side, drift, coverage (per cent), span,
 *   persist, radius.  Polarity p = 0 is bright, p = 1 dark; the two never mix in any step.
 * 1. Band sums.  nb = H / rows;  S[t,b,x] = the sum of Y over the rows b rows .. b rows + rows - 1, int32 [L,nb,W].  The H mod rows
 *    rows at the bottom are in no band and are not read; they are only painted (5).
 * 2. Cross-section test, in envelope form.  The side columns of x are x-gap-side .. x-gap-1 and x+gap+1 .. x+gap+side; a column
 *    with a side column outside the frame is never a candidate.  bright[t,b,x] = S > (the largest S of the sides) + tau rows,
 *    dark[t,b,x] = S < (the smallest) - tau rows: strict.  cand uint8 [L,nb,W] = bright | dark << 1.
 * 3. Height.  near_p[t,b,x] = the OR of the candidates of polarity p at the columns x-drift .. x+drift that lie in the frame;
 *    cnt[t,p,x] = the number of bands with near_p;  col[t,p,x] = cnt 100 >= coverage nb;  b0, b1[t,p,x] = the first and the last
 *    band with near_p, nb and -1 when there is none.  cnt, b0, b1 int32 [L,2,W], col uint8 [L,2,W] of 0 / 1.
 * 4. Persistence.  coln[t,p,x] = the OR of col over x-drift .. x+drift in the frame;  votes[t,p,x] = the number of frames u with
 *    t-span <= u <= t+span, 0 <= u < L, scene[u] == scene[t] and coln[u,p,x];  avail[t] = the number of such frames u;
 *    keep[t,p,x] = col[t,p,x] and votes >= min(persist, avail), uint8 [L,2,W] of 0 / 1;  counts[t] = the sum of keep over p and x,
 *    int32 [L] (the paint entry clears all L first; integer atomics, exact).
 * 5. Paint.  P[t,b,x] = some kept column xx of either polarity with |xx - x| <= radius and b0[t,p,xx] <= b <= b1[t,p,xx];
 *    masks[t,y,x] = 255 P[t, min(y / rows, nb - 1), x], uint8 [L,H,W]: the remainder rows go with the last band.
 * e2fgvi_line_sums does 1, e2fgvi_line_columns 2 and 3, e2fgvi_line_paint 4 and 5 (col may hold any non-zero byte for 1).  The
 * sums entry reads every frame byte of a band once and the paint entry writes every mask byte once; every entry of every output is
 * written.  The same inputs give the same bits in every run; nothing is read on the host.  L, H, W >= 0, H * W < 2^31 - 256, rows
 * in [4, 64], tau in [0, 254], gap in [0, 4], side in [1, 8], drift in [0, 2], coverage in [1, 100], span in [0, 4], persist in
 * [1, 2 span + 1], radius in [0, 16] (E2FGVI_EINVAL otherwise, from the arguments alone); L == 0, H * W == 0 or nb == 0 returns 0
 * without a launch and without looking at the pointers (counts is then not cleared either); a null pointer with work, or an int32
 * array that is not 4-byte aligned, is E2FGVI_EINVAL.  Frames are launched in slabs of 65535. */
int e2fgvi_line_sums(const uint8_t* frames, int32_t L, int32_t H, int32_t W, int32_t rows, int32_t* S, void* stream);
int e2fgvi_line_columns(const int32_t* S, int32_t L, int32_t H, int32_t W, int32_t rows, int32_t tau, int32_t gap, int32_t side,
                        int32_t drift, int32_t coverage, uint8_t* cand, int32_t* cnt, uint8_t* col, int32_t* b0, int32_t* b1,
                        void* stream);
int e2fgvi_line_paint(const uint8_t* col, const int32_t* b0, const int32_t* b1, const int32_t* scene, int32_t L, int32_t H, int32_t W,
                      int32_t rows, int32_t drift, int32_t span, int32_t persist, int32_t radius, uint8_t* keep, int32_t* counts,
                      uint8_t* masks, void* stream);
/* Deflicker (video.deflicker): per frame one tone curve -- a shift per luma level -- that moves the frame's luma quantiles onto
 * their mean over the frames around it in its scene.  All arithmetic is integer; every division is a floor of non-negative numbers
 * and >> of a negative number is the arithmetic shift (a floor as well).
 *   frames uint8 [L,H,W,3];  N = H W, 1 <= N <= 2^26;  scene int32 [L] on the device: two frames are in one scene when their
 *   entries are equal.  Parameters span in [0, 8], max_shift in [1, 64].  K = 32.
 * 1. Luma.  Y = (77 R + 150 G + 29 B + 128) >> 8, the scene detector's and the line-scratch detector's.
 * 2. Histogram.  hist[t][v] = the number of pixels of frame t with Y == v, int32 [L][256];  C[t][v] = hist[t][0] + ... +
 *    hist[t][v], C[t][-1] = 0.
 * 3. Nodes, K quantiles per frame in 1/16 levels.  r_k = ((2k + 1) N) / (2K);  v = the smallest level with C[t][v] > r_k;
 *    Q[t][k] = 16 v + (16 (r_k - C[t][v-1])) / hist[t][v], int32 [L][32], in 0 .. 4095.
 * 4. Target.  W_t = {u : |u - t| <= span, 0 <= u < L, scene[u] == scene[t]}, n = |W_t| >= 1;
 *    T[t][k] = (2 (the sum of Q[u][k] over u in W_t) + n) / (2n);  s[t][k] = clamp(T[t][k] - Q[t][k], -16 max_shift, 16 max_shift).
 * 5. Curve.  For level y: c2 = 2 C[t][y-1] + hist[t][y];  phi = clamp((c2 K 128) / N - 128, 0, (K - 1) 256) (64-bit: c2 K 128
 *    reaches 2^39; the quotient is taken first, the subtraction may go below zero and is clamped);  k0 = phi >> 8, f = phi & 255,
 *    k1 = min(k0 + 1, K - 1);  d16 = (s[t][k0] (256 - f) + s[t][k1] f + 128) >> 8;  d[t][y] = (d16 + 8) >> 4, int16 [L][256].
 * 6. Apply.  out[t,i,j,c] = clamp(frames[t,i,j,c] + d[t][Y(frames[t,i,j])], 0, 255): one shift per pixel, the same for its three
 *    channels.  Because 77 + 150 + 29 = 256 the luma of the result is exactly Y + d wherever no channel clips.
 * e2fgvi_flicker_hist does 1 and 2: it clears all L 256 words on the stream and adds with integer atomics (exact, the same in
 * every run); every frame byte is read once.  e2fgvi_flicker_curves does 3 to 5 in one launch, a workgroup per frame that
 * recomputes the nodes of its window from hist; its contract is that every row of hist sums to N (a row that does not gives some
 * curve and no fault); it writes Q[t] and d[t] of every frame.  e2fgvi_flicker_apply does 6; every output byte is written once;
 * out may be frames itself (in place), any other overlap of the two ranges is E2FGVI_EINVAL.  Nothing is read on the host.
 * L, H, W, N >= 0, H W <= 2^26, N <= 2^26, span and max_shift in their ranges (E2FGVI_EINVAL otherwise, from the arguments alone);
 * L == 0, H W == 0 or N == 0 returns 0 without a launch and without looking at the pointers; a null pointer with work, an int32
 * array that is not 4-byte aligned or a d that is not 2-byte aligned is E2FGVI_EINVAL.  Frames are launched in slabs of 65535. */
int e2fgvi_flicker_hist(const uint8_t* frames, int32_t* hist, int32_t L, int32_t H, int32_t W, void* stream);
int e2fgvi_flicker_curves(const int32_t* hist, const int32_t* scene, int32_t* Q, int16_t* d, int32_t L, int32_t N, int32_t span,
                          int32_t max_shift, void* stream);
int e2fgvi_flicker_apply(const uint8_t* frames, const int16_t* d, uint8_t* out, int32_t L, int32_t H, int32_t W, void* stream);
/* Local deflicker (video.deflicker_local): the deflicker above cell by cell on a grid of gy x gx cells, the cells' curves blended
 * between the cell centres -- for flicker that varies over the frame.  All arithmetic is integer; every division is a floor of
 * non-negative numbers unless said otherwise and >> of a negative number is the arithmetic shift (a floor as well).
 *   frames uint8 [L,H,W,3];  1 <= gy, gx <= 8, H >= gy, W >= gx, H W <= 2^26;  scene, span, max_shift and K = 32 as above.
 * 0. Cells.  Cell (i, j) owns the rows [(i H) / gy, ((i + 1) H) / gy) and the columns [(j W) / gx, ((j + 1) W) / gx);  n_ij is
 *    its number of pixels, >= 1.
 * 1. Luma.  Y as above.
 * 2. Histograms.  hist[t][i][j][v] = the number of pixels of cell (i, j) of frame t with Y == v, int32 [L][gy][gx][256].
 * 3. Nodes.  Q[t][i][j][k] = the deflicker's node k (3 above) of the row hist[t][i][j] with N = n_ij, int32 [L][gy][gx][32].
 * 4. Shifts per node.  s[k] = the deflicker's (4 above) of the rows hist[u][i][j], u in W_t: the cell's own nodes, their rounded
 *    mean over the frames within span of t in t's scene, the difference clamped to +-16 max_shift.
 * 5. Shifts per level.  d16[t][i][j][y] = (s[k0] (256 - f) + s[k1] f + 128) >> 8 with phi, k0, k1 and f as in 5 above from the
 *    cell's own cumulative histogram and N = n_ij: the deflicker's shift in 1/16 levels, WITHOUT its last step (d16 + 8) >> 4.
 *    int16 [L][gy][gx][256], |d16| <= 16 max_shift <= 1024.
 * 6. Apply.  Positions are measured between the cell centres in 1/256 of a cell.  Row r:  v = clamp(((2r + 1) gy 128) / H - 128,
 *    0, (gy - 1) 256) (the quotient first, the difference may go below zero and is clamped);  i0 = v >> 8, fy = v & 255,
 *    i1 = min(i0 + 1, gy - 1).  Column x likewise with gx and W: u, j0, fx, j1.  For a pixel of luma Y, with a = d16[t][i0][j0][Y],
 *    b = d16[t][i0][j1][Y], c = d16[t][i1][j0][Y], e = d16[t][i1][j1][Y]:
 *      D = ((a (256 - fx) + b fx) (256 - fy) + (c (256 - fx) + e fx) fy + 32768) >> 16;   d = (D + 8) >> 4;
 *      out[t,r,x,ch] = clamp(frames[t,r,x,ch] + d, 0, 255), the same d for the three channels.
 *    |a (256 - fx) + b fx| <= 2^18 and the sum in front of the shift stays below 2^27: int32 holds everything.  A pixel in front of
 *    the first cell centre, or behind the last, has f = 0 on that axis and gets that cell's curve alone; gy = gx = 1 gives the
 *    deflicker's bytes (D = a, d its d).
 * e2fgvi_flicker_local_hist does 1 and 2: it clears all L gy gx 256 words on the stream and adds with integer atomics (exact,
 * the same in every run); every frame byte is read once.  e2fgvi_flicker_local_curves does 3 to 5 in one launch, a workgroup per
 * frame and cell that recomputes the nodes of its window from hist; its contract is that hist[t][i][j] sums to n_ij (a row that
 * does not gives some curve and no fault); it writes every entry of Q and d16.  e2fgvi_flicker_local_apply does 6; every output
 * byte is written once, by the thread that read the input byte: out may be frames itself (in place), any other overlap of the two
 * ranges is E2FGVI_EINVAL.  Nothing is read on the host.
 * L, H, W >= 0, H W <= 2^26, gy and gx in [1, 8], span and max_shift in their ranges (E2FGVI_EINVAL otherwise, from the arguments
 * alone);  L == 0 or H W == 0 returns 0 without a launch and without looking at the pointers;  with work, H < gy or W < gx, a null
 * pointer, an int32 array that is not 4-byte aligned or a d16 that is not 2-byte aligned is E2FGVI_EINVAL.  Frames are launched
 * in slabs of 65535. */
int e2fgvi_flicker_local_hist(const uint8_t* frames, int32_t* hist, int32_t L, int32_t H, int32_t W, int32_t gy, int32_t gx,
                              void* stream);
int e2fgvi_flicker_local_curves(const int32_t* hist, const int32_t* scene, int32_t* Q, int16_t* d16, int32_t L, int32_t H, int32_t W,
                                int32_t gy, int32_t gx, int32_t span, int32_t max_shift, void* stream);
int e2fgvi_flicker_local_apply(const uint8_t* frames, const int16_t* d16, uint8_t* out, int32_t L, int32_t H, int32_t W, int32_t gy,
                               int32_t gx, void* stream);
/* Colour restoration (video.restore_color, video.apply_color): per group of frames and channel one monotone byte table, from the
 * channel histograms pooled over the group and their quantile nodes.  All arithmetic is integer; // is the floor also for a
 * negative numerator and >> of a negative number is the arithmetic shift.  Values with a 16 in them are in 1/16 levels.  K = 32.
 *   frames uint8 [L,H,W,3], H W <= 2^26.
 * 1. Histograms.  hist[t][c][v] = the number of pixels of frame t whose channel c equals v, int32 [L][3][256].
 * 2. Pools.  A group g is a list of frames in CSR form: starts int32 [G+1], ids int32 [M]; group g owns ids[starts[g] :
 *    starts[g+1]].  P_g[c][v] = the sum of hist[t][c][v] over the group's ids, in 64 bits;  N = the sum of a row;  C[v] = P[0] +
 *    ... + P[v], C[-1] = 0.  An id outside [0, L) is skipped.  starts is read clamped to [0, M]; a group whose range is empty or
 *    reversed has N = 0.
 * 3. Nodes.  Q[g][c][0..33], int32 [G][3][34].  node(r): v = the smallest level with C[v] > r;  node(r) = 16 v + (16 (r -
 *    C[v-1])) // P[v].  Q[k] = node(((2k + 1) N) // 64) for k < 32;  the black point Q[32] = node((lo N) // 1000);  the white
 *    point Q[33] = node(N - 1 - (hi N) // 1000);  lo and hi in [0, 250], per mille.  N may reach 2^50: everything is 64-bit.  A
 *    group with N = 0 gets zeros.
 * 4. Table of group g, channel c, level v, uint8 [G][3][256].  x = 16 v;  mode int32 [G].
 *      mode 0 (keep), and any other value:  o = x.
 *      mode 1 (levels):  b = Q[g][c][32], w = Q[g][c][33];  channel c is usable when w - b >= 16 min_range.  With an automatic
 *        target (lo_t < 0) B is the smallest b and Wt the largest w over the usable channels of g (no usable channel: every
 *        table is the identity); otherwise B = 16 lo_t, Wt = 16 hi_t.  c not usable: o = x.  c usable: den = w - b,
 *        num = min(Wt - B, (max_gain den) >> 8) -- a gain above max_gain / 256 is cut, and the centre of the range stays on the
 *        centre of the target --, o = ((B + Wt) den + (2x - b - w) num + den) // (2 den).
 *      mode 2 (match):  q[k] = Q[g][c][k], t[k] = clamp(T[g][c][k], 0, 4095), k < 32, T laid out as Q.  x <= q[0]: o = x + t[0] -
 *        q[0].  Otherwise x >= q[31]: o = x + t[31] - q[31].  Otherwise k = the largest index with q[k] <= x, den = q[k+1] - q[k]
 *        (above zero by the choice of k, whatever q holds), o = t[k] + (2 (x - q[k]) (t[k+1] - t[k]) + den) // (2 den).
 *    o' = x + (((o - x) strength + 128) >> 8), strength in [0, 256];  lut[g][c][v] = clamp((o' + 8) >> 4, 0, 255).
 * 5. Apply.  out[t,i,j,c] = lut[group[t]][c][frames[t,i,j,c]], group int32 [L]; a frame with group[t] outside [0, G) is copied.
 * e2fgvi_color_hist does 1: it clears all L 768 words on the stream and adds with integer atomics (exact, the same in every run);
 * every frame byte is read once.  e2fgvi_color_nodes does 2 and 3, a workgroup per group and channel, and writes every entry of
 * Q.  e2fgvi_color_lut does 4 and writes every entry of lut; its Q is e2fgvi_color_nodes' (values in 0 .. 4095; others give some
 * table and no fault); T is never null when G > 0 (Q itself where nothing is matched).  e2fgvi_color_apply does 5; every output
 * byte is written once, by the thread that read the input byte: out may be frames itself (in place), any other overlap of the
 * two ranges is E2FGVI_EINVAL.  Nothing is read on the host.
 * L, H, W, G, M >= 0, H W <= 2^26, lo and hi in [0, 250], min_range in [1, 255], max_gain in [256, 4096], strength in [0, 256], the
 * target lo_t = hi_t = -1 or 0 <= lo_t < hi_t <= 255 (E2FGVI_EINVAL otherwise, from the arguments alone).  No work -- L == 0 or
 * H W == 0 for hist and apply, G == 0 for nodes and lut -- returns 0 without a launch and without looking at the pointers; with
 * work a null pointer (hist of no frame, ids of no id and lut of no group may be null) or an int32 array that is not 4-byte
 * aligned is E2FGVI_EINVAL.  Frames are launched in slabs of 65535. */
int e2fgvi_color_hist(const uint8_t* frames, int32_t* hist, int32_t L, int32_t H, int32_t W, void* stream);
int e2fgvi_color_nodes(const int32_t* hist, const int32_t* starts, const int32_t* ids, int32_t* Q, int32_t L, int32_t G, int32_t M,
                       int32_t lo, int32_t hi, void* stream);
int e2fgvi_color_lut(const int32_t* Q, const int32_t* T, const int32_t* mode, uint8_t* lut, int32_t G, int32_t lo_t, int32_t hi_t,
                     int32_t min_range, int32_t max_gain, int32_t strength, void* stream);
int e2fgvi_color_apply(const uint8_t* frames, const uint8_t* lut, const int32_t* group, uint8_t* out, int32_t L, int32_t H, int32_t W,
                       int32_t G, void* stream);
/* Weave stabiliser (video.stabilize): the translation of the picture from frame to frame -- gate weave, telecine jitter -- measured
 * from banded luma profiles, a path smoothed over a symmetric window, and the frames moved back onto it.  All arithmetic is
 * integer; "floor" is the floor for either sign, >> of a negative number is the arithmetic shift and & 15 its non-negative rest.
 *   frames uint8 [L,H,W,3];  scene int32 [L] on the device: two frames are in one scene when their entries are equal.
 *   NB = 8 bands per axis.  Parameters radius R in [1, 32], tex in [0, 65535], span in [0, 16], max_shift in [1, 64].
 * 1. Profiles of Y = (77 R + 150 G + 29 B + 128) >> 8.  col[t][b][x] = the sum of Y over the rows [bH/8, (b+1)H/8) of column x,
 *    int32 [L][8][W];  row[t][b][y] = the sum over the columns [bW/8, (b+1)W/8) of row y, int32 [L][8][H] (floor divisions; a band
 *    may be empty).  The gradient of a profile P of length n is g[i] = P[i+1] - P[i-1], 0 at i = 0 and i = n - 1.
 * 2. Motion of the pair (t-1, t), per axis (x: col, n = W, bands over the rows; y: row, n = H) and band.  The window is i in
 *    [R+1, n-R-1);  cost(s) = the sum over the window of |g_t[i+s] - g_{t-1}[i]|, s in [-R, R], 64-bit.  The best s has the smallest
 *    cost; ties go to the smallest |s|, then to the negative one.  With c-, c0, c+ the costs at s-1, s, s+1: den = c- - 2 c0 + c+,
 *    delta = floor((16 (c- - c+) + den) / (2 den)), and delta = 0 when c0 == 0.  The band is valid when it is not empty, the window
 *    has at least 2R elements, -R < s < R, den > 0 and the window's sum of |g_{t-1}| is at least tex times its length; its motion
 *    is 16 s + delta, in 1/16 px.  The pair's motion on the axis is the lower median of the valid bands' when at least NB/2 are
 *    valid (the pair is trusted), else 0.  Frame 0 and the first frame of a scene: motion 0, no valid band.
 *    motion int32 [L][4] = mx, my, nx, ny: the motion and the number of valid bands per axis.
 * 3. Path.  Frame t starts a segment on an axis when t == 0, scene[t] != scene[t-1] or n_axis[t] < NB/2.  p_t = the sum of the
 *    motion from the segment's second frame to t;  k_t = min(span, t - first, last - t);  q_t = floor((2 S + n) / (2n)), S the sum
 *    of p over [t-k_t, t+k_t], n = 2 k_t + 1, 64-bit;  c_t = clamp(q_t - p_t, -16 max_shift, 16 max_shift).  Without subpixel
 *    c_t = ((c_t + 8) >> 4) << 4.  shift int32 [L][2] = cx, cy in 1/16 px.
 * 4. Apply, C = 1 or 3 bytes a pixel.  cx, cy clamped to +-16 * 64.  X = 16 x - cx, x0 = X >> 4, fx = X & 15, likewise y; the taps
 *    a, b, c, d = (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), coordinates clamped to the frame;  out = ((16-fx)(16-fy) a +
 *    fx (16-fy) b + (16-fx) fy c + fx fy d + 128) >> 8 per channel;  mask[t][y][x] = 255 where a tap of non-zero weight lies
 *    outside the frame before clamping, else 0.  A whole-pixel shift copies bytes, a zero shift returns the input.
 * e2fgvi_weave_profiles does 1 in one pass (it clears col on the stream and adds with integer atomics; every word of col and row
 * is written, every frame byte read once); e2fgvi_weave_match does 2 in one launch, e2fgvi_weave_path 3, e2fgvi_weave_apply 4
 * (mask may be null; out and mask must not overlap frames or each other: E2FGVI_EINVAL).  Nothing is read on the host.  Sizes >=
 * 0; H, W <= 4096 for profiles and match, H W <= 2^26 for apply; parameters in their ranges, subpixel 0 or 1 (E2FGVI_EINVAL
 * otherwise, from the arguments alone); L, H or W == 0 returns 0 without a launch and without looking at the pointers; a null
 * pointer with work or an int32 array that is not 4-byte aligned is E2FGVI_EINVAL.  Frames are launched in slabs of 65535. */
int e2fgvi_weave_profiles(const uint8_t* frames, int32_t* col, int32_t* row, int32_t L, int32_t H, int32_t W, void* stream);
int e2fgvi_weave_match(const int32_t* col, const int32_t* row, const int32_t* scene, int32_t* motion, int32_t L, int32_t H,
                       int32_t W, int32_t radius, int32_t tex, void* stream);
int e2fgvi_weave_path(const int32_t* motion, const int32_t* scene, int32_t* shift, int32_t L, int32_t span, int32_t max_shift,
                      int32_t subpixel, void* stream);
int e2fgvi_weave_apply(const uint8_t* frames, const int32_t* shift, uint8_t* out, uint8_t* mask, int32_t L, int32_t H, int32_t W,
                       int32_t C, void* stream);
/* Deinterlacer (video.deinterlace, video.detect_interlace): an interlaced frame is two fields, half a frame period apart, on
 * alternating rows; each field becomes a picture of its own, and the field order is measured.  All arithmetic is integer and >> of
 * a negative number is the arithmetic shift.
 *   frames uint8 [L,H,W,3];  scene int32 [L] on the device: two frames are in one scene when their entries are equal.
 *   Y = (77 R + 150 G + 29 B + 128) >> 8, the luma of the other tools.  Row parity 0 is the top field;  tff in {0, 1}: the field
 *   shown first has parity first = tff ? 0 : 1.  A neighbour frame t-1 or t+1 that lies outside the video or in another scene is
 *   replaced by frame t itself.  Parameters mode in [0, 2], guard in {0, 1}, edges in [0, 2].
 * Deinterlace.  Frame t gives two pictures: O[2t] keeps the rows of parity first, O[2t+1] those of parity 1 - first; a kept row is
 * copied.  With P, C, N the frames t-1, t, t+1: for O[2t] A = P, B = C, for O[2t+1] A = C, B = N -- the two fields of the missing
 * parity nearest in time, one before and one after.  For a picture that keeps parity p, a missing row y (y & 1 != p) and column x:
 *   up = y-1 if y-1 >= 0, else y+1;  dn = y+1 if y+1 <= H-1, else y-1.  With H == 1 there is neither: out = (A[y] + B[y]) >> 1 per
 *   channel and nothing else applies.  Columns are clamped to [0, W-1] wherever x plus an offset is written.
 * 1. c = Y_C[up][x], e = Y_C[dn][x], dY = (Y_A[y][x] + Y_B[y][x]) >> 1.
 * 2. t0 = |Y_A[y][x] - Y_B[y][x]|;  t1 = (|Y_P[up][x] - c| + |Y_P[dn][x] - e|) >> 1;  t2 = (|Y_N[up][x] - c| + |Y_N[dn][x] - e|) >> 1;
 *    diff = max(t0 >> 1, t1, t2).
 * 3. Direction.  score(j) = the sum over k in {-1, 0, 1} of |Y_C[up][x+k+j] - Y_C[dn][x+k-j]|.  best = score(0) - 1, J = 0.  For
 *    sgn = -1, then sgn = +1: if edges >= 1 and score(sgn) < best, take it: best = score(sgn), J = sgn; only if it was taken, and
 *    edges >= 2, and score(2 sgn) < best: best = score(2 sgn), J = 2 sgn.  The + side compares against the best so far, the -
 *    side's result included.
 * 4. Guard, when guard == 1 and y-2 >= 0 and y+2 <= H-1 (otherwise it is skipped, not clamped).  b = (Y_A[y-2][x] + Y_B[y-2][x]) >> 1,
 *    f likewise at y+2;  mx = max(dY - e, dY - c, min(b - c, f - e));  mn = min(dY - e, dY - c, max(b - c, f - e));
 *    diff = max(diff, mn, -mx).
 * 5. Per channel: sp = (C[up][x+J] + C[dn][x-J]) >> 1;  d = (A[y][x] + B[y][x]) >> 1;  out = clamp(sp, d - diff, d + diff).  All
 *    decisions are taken on luma, so they are the same for a pixel's three channels.
 * mode 0: field rate, out [2L,H,W,3] = O;  mode 1: frame rate, first field kept, out[t] = O[2t];  mode 2: frame rate, second field
 * kept, out[t] = O[2t+1].  Every output byte is written once.
 * Scores.  m = (H - 2) / 2 (floor); the rows are y in [1, 2m]: as many even rows as odd ones, none when H < 4.  For t with t+1 in
 * the same scene D[t][q] = the sum, over the rows of parity q and all columns, of |2 Y_{t+1}[y][x] - Y_t[y-1][x] - Y_t[y+1][x]|;
 * D int64 [L][2], D[t] = 0 for the last frame of a scene.  D[t][0] sets the bottom field of t against the top field of t+1 -- half
 * a frame period apart under top-field-first, one and a half under bottom-field-first -- and D[t][1] is the mirror; on progressive
 * video the two are equal up to texture.
 * e2fgvi_interlace_scores clears D on the stream and adds with integer atomics (exact, the same in every run); every frame byte is
 * read at most twice.  e2fgvi_deinterlace is one launch; out must not overlap frames (E2FGVI_EINVAL).  Nothing is read on the host.
 * Sizes >= 0, H W <= 2^26, parameters in their ranges (E2FGVI_EINVAL otherwise, from the arguments alone); L, H or W == 0 returns 0
 * without a launch and without looking at the pointers; a null pointer with work, a scene that is not 4-byte aligned or a D that is
 * not 8-byte aligned is E2FGVI_EINVAL.  Frames are launched in slabs of 65535. */
int e2fgvi_interlace_scores(const uint8_t* frames, const int32_t* scene, int64_t* D, int32_t L, int32_t H, int32_t W, void* stream);
int e2fgvi_deinterlace(const uint8_t* frames, const int32_t* scene, uint8_t* out, int32_t L, int32_t H, int32_t W, int32_t tff,
                       int32_t mode, int32_t guard, int32_t edges, void* stream);
/* Inverse telecine (video.inverse_telecine, video.detect_telecine): video made from 24 fps film by 3:2 pulldown holds, in two of
 * every five frames, the fields of two different film frames; the scores say for every frame which neighbour its other field
 * fits, and the weave puts the fields back together.  All arithmetic is integer.
 *   frames uint8 [L,H,W,3];  scene int32 [L] on the device: two frames are in one scene when their entries are equal.
 *   Y = (77 R + 150 G + 29 B + 128) >> 8, the luma of the other tools.
 * Scores.  M int64 [L][2][3][16].  For frame t, row parity q -- the parity of the rows that would be taken from another frame -- and
 * candidate j in {0, 1, 2}, which stands for the source s = t-1, t, t+1; a source that lies outside the video or in another scene
 * is replaced by t itself.  m = (H - 2) / 2 (floor); the rows are y in [1, 2m] with (y & 1) == q, over all columns x: the rows of
 * the interlace scores, none when H < 4.  cell = ((4 y) / H) * 4 + (4 x) / W, the scene detector's 4 x 4 grid.
 *   M[t][q][j][cell] = the sum of |2 Y_s[y][x] - Y_t[y-1][x] - Y_t[y+1][x]|
 * -- how badly the field of parity q of frame s combs against the other field of frame t, cell by cell.  Wherever t has a successor
 * in its scene the sum over the cells of M[t][q][2] is D[t][q] of e2fgvi_interlace_scores; where a candidate was replaced by t,
 * M[t][q][j] == M[t][q][1].
 * e2fgvi_telecine_scores clears M on the stream and adds with integer atomics, one per (q, j, cell) and workgroup (exact, the same
 * in every run).  Frames are launched in slabs of 65535.
 * Weave.  jobs int32 [n][2] = (a, b) on the device, keep in {0, 1}, out uint8 [n,H,W,3]: the rows of parity keep of out[i] are the
 * rows of frames[a_i], the other rows those of frames[b_i].  One launch; every output byte is written once; ids are clamped to
 * [0, L-1], so none reads outside frames (the callers refuse them first); out must not overlap frames (E2FGVI_EINVAL).
 * Nothing is read on the host.  Sizes >= 0, H W <= 2^26, keep in {0, 1} (E2FGVI_EINVAL otherwise, from the arguments alone); L, H or
 * W == 0 (scores), n, H or W == 0 (weave) returns 0 without a launch and without looking at the pointers; a null pointer with work,
 * a scene or jobs that is not 4-byte aligned, an M that is not 8-byte aligned and jobs with L == 0 are E2FGVI_EINVAL. */
int e2fgvi_telecine_scores(const uint8_t* frames, const int32_t* scene, int64_t* M, int32_t L, int32_t H, int32_t W, void* stream);
int e2fgvi_field_weave(const uint8_t* frames, const int32_t* jobs, uint8_t* out, int32_t L, int32_t n, int32_t H, int32_t W,
                       int32_t keep, void* stream);
/* Temporal denoiser (video.denoise): a pixel becomes the weighted mean of itself and of the pixels its flows point at in the frame
 * before and the frame after, each weighted by how well the 3 x 3 luma patch around it matches the pixel's own.  All integers after
 * one floor; >> of a negative number is the arithmetic shift, / of integers the floor.
 *   frames uint8 [L,H,W,3];  fwd, bwd fp32 [L-1,H,W,2], 8-byte aligned, in e2fgvi_defect_candidates' convention;  scene int32 [L]:
 *   two frames are in one scene when their entries are equal.  Y = (77 R + 150 G + 29 B + 128) >> 8.
 *   Parameters h = strength in [1, 64], s = search in [0, 2], limit = max_change in [0, 255];  m = (65536 + (9 h) / 2) / (9 h).
 * For centre frame t and pixel p = (x, y) there are two neighbours: A is frame t-1 with g = bwd[t-1], B is frame t+1 with g = fwd[t],
 * both read on frame t's grid.  A neighbour outside the video or in another scene contributes nothing.  Per neighbour N that exists:
 * 1. q = (x + g_x(p), y + g_y(p)) in fp64;  inside = g(p) finite and 0 <= q_x <= W-1 and 0 <= q_y <= H-1, decided in floating
 *    point before any conversion;  r = floor(q + 0.5).  A pixel that is not inside takes nothing from N.
 * 2. The candidates are c = r + (i, j), -s <= i, j <= s, whose centre lies in the frame (one that does not is dropped, not clamped).
 * 3. SAD(c) = the sum over u, v in {-1, 0, 1} of |Y_t(clamp(p + (u, v))) - Y_N(clamp(c + (u, v)))|, taps clamped to the frame on
 *    both sides.
 * 4. w(c) = max(0, 256 - ((SAD(c) m) >> 8)).
 * Wsum = 256 + the sum of w(c) over both neighbours' candidates;  per channel k: acc_k = 256 C_k(p) + the sum of w(c) N_k(c);
 * o_k = (acc_k + (Wsum >> 1)) / Wsum;  out_k = clamp(o_k, C_k(p) - limit, C_k(p) + limit).  All decisions are on luma, so a
 * pixel's three channels share their weights.  Every output byte is written once; out must not overlap frames (E2FGVI_EINVAL).
 * All intermediates fit int32: SAD m < 2^25, Wsum <= 13056, acc < 2^22.
 * work: a device buffer of at least L (H + 8) (((W + 11) & ~3) + 4) bytes, 4-byte aligned, that overlaps neither frames nor out:
 * the entry writes the luma of every frame into it first (one launch) and the filter reads it (one launch); its contents
 * afterwards are not part of the contract.  work_bytes is its size.  Nothing is read on the host.
 * Sizes >= 0, H W < 2^31 - 256, parameters in their ranges (E2FGVI_EINVAL otherwise, from the arguments alone); L, H or W == 0
 * returns 0 without a launch and without looking at the pointers; a null or misaligned pointer with work, or a work buffer that
 * is too small, is E2FGVI_EINVAL.  L == 1 has no neighbour: out = frames, and fwd, bwd and work are not looked at.  Frames are
 * launched in slabs of 65535. */
int e2fgvi_denoise(const uint8_t* frames, const float* fwd, const float* bwd, const int32_t* scene, uint8_t* out, uint8_t* work,
                   int64_t work_bytes, int32_t L, int32_t H, int32_t W, int32_t strength, int32_t search, int32_t max_change,
                   void* stream);
/* Frames between frames (video.retime, video.replace_frames): the picture at the time k / d between two frames, gathered along the
 * two flows between them.  No atomics: the same inputs give the same bytes.
 *   frames uint8 [L,H,W,3];  fwd, bwd fp32 [P,H,W,2], 8-byte aligned, P flow pairs in e2fgvi_warp_error's convention (pixels,
 *   channel 0 = x);  jobs int32 [n,5] on the device, one row (ia, ib, fi, k, d) per output frame: A = frames[ia], B = frames[ib],
 *   f = fwd[fi] the motion A -> B on A's grid, g = bwd[fi] the motion B -> A on B's grid;  out uint8 [n,H,W,3];  source uint8
 *   [n,H,W] or NULL.  Parameters iterations in [0, 8], tol = tolerance in [0, 255] (1/16 px), match in [0, 765].
 * A job with ia or ib outside [0, L), fi outside [0, P), d outside [1, 64] or k outside [0, d] writes nothing.
 * k == 0: out = A, source = 5.  k == d: out = B, source = 5.  Otherwise tau = (double)k / (double)d, sigma = (double)(d - k) /
 * (double)d, and every output pixel p = (x, y) gets two candidate trajectories through it: side A = side(S = A, E = B, h = f,
 * lambda = tau) and side B = side(S = B, E = A, h = g, lambda = sigma).  All coordinate arithmetic is fp64 on the fp32 inputs, in
 * the order written, one rounding per operation (no fused multiply-add).  side(S, E, h, lambda):
 * 1. inside(q): q finite and 0 <= q_x <= W-1 and 0 <= q_y <= H-1, decided in floating point before any conversion to an integer.
 * 2. bil(h, q), for inside(q): with (x0, y0) = floor(q), w1 = q - (x0, y0), w0 = 1 - w1 per axis, the corners' weights w00 = wy0 wx0,
 *    w01 = wy0 wx1, w10 = wy1 wx0, w11 = wy1 wx1 (01 is the corner to the right, 10 the one below); the sample is w00 h00, + w01 h01,
 *    + w10 h10, + w11 h11 in that order, a corner outside the image left out (e2fgvi_mask_track_step's sample).
 * 3. h0 = h(p);  q = (x - lambda h0_x, y - lambda h0_y), the product first.
 * 4. `iterations` times: the side fails unless inside(q);  hq = bil(h, q);  the side fails unless hq is finite;
 *    q = (x - lambda hq_x, y - lambda hq_y).
 * 5. The side fails unless inside(q) and hq = bil(h, q) is finite.  r = ((q_x + lambda hq_x) - x, (q_y + lambda hq_y) - y);
 *    landed = r_x r_x + r_y r_y <= (double)(tol tol) / 256.0.
 * 6. e = (q_x + hq_x, q_y + hq_y);  two_ended = landed and inside(e).
 * 7. Integers from here on.  tap16(T, q): Q = floor(q 16 + 0.5) per component, xi = Q_x >> 4, fx = Q_x & 15, likewise y; the right
 *    and lower corner indices are clamped to W-1 and H-1 (their weight is 0 there); per channel
 *    ((16 - fy) ((16 - fx) c00 + fx c01) + fy ((16 - fx) c10 + fx c11) + 128) >> 8.  s = tap16(S, q), and t = tap16(E, e) when two_ended.
 * 8. cost = the sum over the channels of |s - t|;  matched = two_ended and cost <= match.
 * 9. The matched colour: side A ((d - k) s + k t + d / 2) / d, side B ((d - k) t + k s + d / 2) / d, integer divisions.
 * Per pixel: A matched and (B not matched or cost_A <= cost_B): A's matched colour, source 1.  Otherwise B matched: B's matched
 * colour, source 2.  Neither matched: A landed and (B not landed or 2 k <= d): s_A alone, source 3; otherwise B landed: s_B alone,
 * source 4 (3 and 4: a place seen in one frame only, at an occlusion or a frame border); nothing landed: the cross-fade
 * ((d - k) A(p) + k B(p) + d / 2) / d per channel, source 0.  A non-finite flow only ever fails a side, by select.
 * One launch per 65535 jobs (the job is the grid's y axis); offsets are 64-bit; every byte of an in-range job's frame is written
 * once; out and source must overlap neither frames, fwd, bwd or jobs nor each other (E2FGVI_EINVAL).  Nothing is read on the host.  Sizes >= 0, H W < 2^31 - 256, parameters in
 * their ranges (E2FGVI_EINVAL otherwise, from the arguments alone); n, H or W == 0 returns 0 without a launch and without looking
 * at the pointers; a null pointer with work (frames with L > 0, fwd and bwd with P > 0, jobs, out), flows that are not 8-byte
 * aligned or jobs that are not 4-byte aligned are E2FGVI_EINVAL. */
int e2fgvi_interpolate(const uint8_t* frames, const float* fwd, const float* bwd, const int32_t* jobs, uint8_t* out, uint8_t* source,
                       int32_t n, int32_t L, int32_t P, int32_t H, int32_t W, int32_t iterations, int32_t tolerance, int32_t match,
                       void* stream);

/* conv_offset post-processing of SecondOrderDeformableAlignment (feat_prop.py:38-53) fused into the conv that produces
 * it: `residual` must point to the per-pixel flows [P,4] = (u1,v1,u2,v2) with res_ld = 4, `slope` = max_residue:
 * offset channels -> slope*tanh(v) + flow.flip, mask channels (last third) -> sigmoid(v) */
#define E2FGVI_ACT_DCNPOST 4

#define E2FGVI_MAX_SRC 4

/* element types of the tensors of the 16-bit data path (see the end of this header) */
#define E2FGVI_F32 0
#define E2FGVI_BF16 1
#define E2FGVI_BF16X3 2      /* not a storage type: fp32 sources and results, the MFMA operands as three bf16 pieces each, six exact terms
                              * per product (mfma_dtype of the deformable conv, mode of e2fgvi_conv2d_x and of the weight packers) */
#define E2FGVI_F16 3         /* IEEE half: accepted wherever E2FGVI_BF16 names a storage type (dst / res / src / mfma / tail / helper
                              * dtypes, e2fgvi_cast); fp32 -> fp16 rounds to nearest even, +-inf past 65504, subnormals kept */

const char* e2fgvi_last_error(void);
/* 9.  Version 9 consolidated the per-type entry points of versions 2-8 (suffixes _x, _xs, _bf16, _f16, _f32x, _f32x3, _taps): one
 * entry point per operation, the element type an E2FGVI_* argument. */
int e2fgvi_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Operands are slices.  Every float entry point below takes its operands as slices of larger tensors: a pixel stride (*_ld), a
 * first channel (*_coff), a channel count (cpg, Cout, src_c, channels), a row range.  For all of them:
 *   - a kernel's result depends on no byte outside the declared slices of its operands: a channel, pixel or row next to a slice
 *     may hold anything, Inf and NaN included (nothing outside a slice is loaded and then multiplied by 0);
 *   - a kernel changes no byte outside the declared slice of its destinations (second outputs and planes included);
 *   - pad channels inside a declared slice (the fourth / last five channels of NHWC4 / NHWC8 frames, channels 4..7 of flows8) are
 *     the producer's to zero: the kernels that write such tensors write the zeros, a consumer may multiply them by weights.
 * tests/test_gpu_slices.py holds every entry point to it, in NaN-poisoned arenas, at the tiles of its own tests.
 * ---------------------------------------------------------------------------------------------- */

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear layer on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces torch.nn.functional.conv2d / linear at: encoder model/e2fgvi.py:75-109, decoder
 * :143-150, SPyNet 7x7 stacks model/modules/flow_comp.py:180-215, conv_offset / backbone / fusion
 * model/modules/feat_prop.py:20-28,73-79, SoftSplit unfold+linear tfocal_transformer.py:40-45
 * (= 7x7 stride-3 conv), qkv/proj :221,398, FFN linears :80-81, SoftComp linear :68.
 *
 * The input is the *virtual channel concat* of up to 4 NHWC sources (so torch.cat copies at
 * e2fgvi.py:101-107, feat_prop.py:36,126-136 never exist).  With `groups` > 1, group g reads
 * channels [coff[s] + g*cpg[s], +cpg[s]) of every source s, in source order.
 * Weights must be pre-packed with e2fgvi_pack_conv_weight using the same cpg[] / bk.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const float* src[E2FGVI_MAX_SRC];
    int32_t src_ld[E2FGVI_MAX_SRC];    /* pixel stride of each source, floats (multiple of 4)      */
    int32_t src_coff[E2FGVI_MAX_SRC];  /* first channel used by group 0 (multiple of 4)            */
    int32_t src_cpg[E2FGVI_MAX_SRC];   /* channels per group taken from this source (mult. of 4)   */
    int32_t nsrc;
    int32_t N, H, W;                   /* input batch / height / width                             */
    int32_t Ho, Wo;                    /* output height / width                                    */
    int32_t KH, KW, stride, pad;
    int32_t groups;
    int32_t Cout;                      /* total output channels                                    */
    int32_t bk;                        /* K-chunk the weights were packed for: 8, 16 or 32         */
    const float* wpacked;
    const float* bias;                 /* [Cout] or NULL                                           */
    const float* residual;             /* NHWC [N,Ho,Wo,*] added before the activation, or NULL    */
    int32_t res_ld, res_coff;
    float* dst;
    int32_t dst_ld, dst_coff;
    int32_t dst_nchw;                  /* 1: dst is plain NCHW [N,Cout,Ho,Wo] (ld/coff ignored)     */
    int32_t act;
    float slope;
    int32_t tile;                      /* 0 = auto; otherwise force a tile config (tests/bench)    */
} e2fgvi_conv_desc;

int e2fgvi_conv2d_nhwc(const e2fgvi_conv_desc* d, void* stream);
/* The same operator from a build without packed-fp32 VALU instructions (v_pk_{mul,add,fma}_f32): for launches that run
 * on a side stream concurrently with bf16 MFMA kernels -- SPyNet next to the encoder.  Identical results. */
int e2fgvi_conv2d_nhwc_nopk(const e2fgvi_conv_desc* d, void* stream);

/* number of floats of the packed weight buffer for the given geometry */
int64_t e2fgvi_packed_conv_weight_size(int32_t Cout, int32_t groups, int32_t KH, int32_t KW,
                                       int32_t nsrc, const int32_t* src_cpg, int32_t bk);
/* w: reference layout [Cout, sum(cpg), KH, KW] (torch OIHW; Linear = [Cout, Cin, 1, 1]) */
int e2fgvi_pack_conv_weight(const float* w, float* wpacked, int32_t Cout, int32_t groups,
                            int32_t KH, int32_t KW, int32_t nsrc, const int32_t* src_cpg,
                            int32_t bk, void* stream);

/* Winograd F(2x2,3x3) form of the same operator for 3x3 / stride 1 / pad 1 layers with even H, W (the encoder's
 * stride-1 layers e2fgvi.py:77-93, the decoder convs :112-150, SoftComp's HQ bias conv e2fgvi_hq tfocal :67-79): fp32
 * arithmetic on the fp32 MFMA pipe, 16 instead of 36 multiplies per 2x2 outputs.  Also the propagation convs
 * (feat_prop.py:20-28,73-79) incl. the ACT_DCNPOST epilogue.  Same descriptor; restrictions: every src_cpg a multiple
 * of 4, NHWC output, bk ignored; tile = 0 (auto), 32 / 64 (couts per workgroup, 16x16-pixel blocks) or 132 / 164
 * (8x16-pixel blocks).  Weights: [group][8-channel chunk][16 positions][2][Npad][4] holding G g G^T. */
int64_t e2fgvi_packed_winograd_weight_size(int32_t Cout, int32_t groups, int32_t nsrc, const int32_t* src_cpg); /* floats */
int e2fgvi_pack_winograd_weight(const float* w, float* wpacked, int32_t Cout, int32_t groups, int32_t nsrc,
                                const int32_t* src_cpg, void* stream);
int e2fgvi_conv3x3_winograd(const e2fgvi_conv_desc* d, void* stream);

/* Wide-tile Winograd forms of the same operator (csrc/conv_wino4.hip): F(fy x 4, 3x3) with fy = 2 (24 transform positions
 * per 2x4 outputs: 3 multiplies per output and input channel) or fy = 4 (36 per 4x4: 2.25), against 4 for F(2x2,3x3) and
 * 9 for the direct convolution the reference runs (F.conv2d at e2fgvi.py:77-93,112-150, feat_prop.py:20-28,73-79).
 * Same descriptor and restrictions as e2fgvi_conv3x3_winograd, plus H % fy == 0 and W % 4 == 0; tile = 0 (auto), 32 or
 * 64 couts per workgroup (fy = 4: 32).  Weights: [group][8-channel chunk][(fy+2)*6 positions][2][Npad][4] holding
 * G_y g G_x^T.  fp32 throughout; rounding relative to the output rms on 512 input channels: 6.5e-6 (fy = 2), 1.9e-5
 * (fy = 4) -- the direct fp32 convolution sits at 7.7e-6. */
int64_t e2fgvi_packed_winograd4_weight_size(int32_t Cout, int32_t groups, int32_t nsrc, const int32_t* src_cpg, int32_t fy);
int e2fgvi_pack_winograd4_weight(const float* w, float* wpacked, int32_t Cout, int32_t groups, int32_t nsrc,
                                 const int32_t* src_cpg, int32_t fy, void* stream);
int e2fgvi_conv3x3_winograd4(const e2fgvi_conv_desc* d, int32_t fy, void* stream);

/* The decoder's last layer (csrc/conv_tail.hip): nn.Conv2d(64, 3, kernel_size=3, stride=1, padding=1) + torch.tanh
 * (model/e2fgvi.py:99-103,261 / model/e2fgvi_hq.py:99-103,263).  With 3 output channels the nine taps move to the N side of
 * ONE [pixels x 64] x [64 x 27] GEMM (every input pixel read once, 9x fewer matrix instructions than the implicit GEMM),
 * followed by the shifted 9-term sum in LDS.  src: NHWC [N,H,W,src_ld >= 64] of src_dtype (E2FGVI_F32: exact fp32 MFMA;
 * E2FGVI_BF16 / E2FGVI_F16: bf16 / fp16 MFMA, fp32 accumulation), 16-byte aligned rows; wpacked: 64 x 32 elements of src_dtype from
 * e2fgvi_pack_tail_weight (w: fp32 OIHW [3,64,3,3]); bias fp32 [3] or NULL; dst fp32 NCHW [N,3,H,W]; act: E2FGVI_ACT_*.
 * Only Cin = 64, Cout = 3 is built (E2FGVI_EUNSUP otherwise). */
int64_t e2fgvi_packed_tail_weight_size(int32_t Cout, int32_t Cin);
int e2fgvi_pack_tail_weight(const float* w, void* wpacked, int32_t Cout, int32_t Cin, int32_t dtype, void* stream);
int e2fgvi_conv3x3_tail(const void* src, int32_t src_dtype, int32_t src_ld, const void* wpacked, const float* bias, float* dst,
                        int32_t N, int32_t H, int32_t W, int32_t act, float slope, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Modulated deformable convolution (DCNv2), im2col-free: bilinear gather straight into LDS + MFMA.
 * Replaces mmcv.ops.modulated_deform_conv2d (mmcv-full 1.4.8) called at
 * model/modules/feat_prop.py:55-58.  x is the virtual concat of two NHWC sources (feat_prop |
 * feat_n2, feat_prop.py:127).  offset: [P, dg*2*K] with (dy,dx) interleaved per tap, mask:
 * [P, dg*K] (both pixel-major, the NHWC image of mmcv's NCHW tensors).
 * If `flows` != NULL the kernel also applies SecondOrderDeformableAlignment's post-processing
 * (feat_prop.py:38-53) on the fly: offset/mask are then the raw conv_offset output (o1|o2|mask),
 * offset = max_residue * tanh(raw) + flow.flip (flow_1 for the first dg/2 groups, flow_2 for the
 * rest), mask = sigmoid(raw); flows is [P,4] = (u1,v1,u2,v2).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const void* src[2];                /* fp32 NHWC (bf16 NHWC with src_dtype = E2FGVI_BF16)       */
    int32_t src_ld[2];
    int32_t src_c[2];                  /* channels of each source; C = sum; C/dg multiple of 16    */
    int32_t nsrc;
    int32_t N, H, W, Ho, Wo;
    int32_t KH, KW, stride, pad, dil;
    int32_t deform_groups;
    int32_t Cout;
    const float* offset; int32_t off_ld;
    const float* mask;   int32_t mask_ld;
    const float* flows;                /* optional [P,4]                                           */
    float max_residue;
    const float* wpacked;              /* e2fgvi_pack_dcn_weight for mfma_dtype (of its type)      */
    const float* bias;
    float* dst; int32_t dst_ld, dst_coff;
    int32_t tile;
    int32_t dst_dtype;                 /* E2FGVI_F32 (0, default) or E2FGVI_BF16 / E2FGVI_F16: dst is a 16-bit NHWC tensor */
    int32_t mfma_dtype;                /* the type wpacked was packed for.  E2FGVI_F32 (0, default): fp32 MFMA;
                                          E2FGVI_BF16 / E2FGVI_F16: the sampled slab is rounded to 16 bits and multiplied on
                                          bf16 / fp16 MFMA (fp32 gather / blend / accumulation; E2FGVI_F16 needs src_dtype =
                                          E2FGVI_F16 and dst_dtype E2FGVI_F32 or E2FGVI_F16); E2FGVI_BF16X3: fp32 sources and
                                          results, blended values and weights as three bf16 pieces, six exact terms per product */
    int32_t src_dtype;                 /* E2FGVI_F32 (0, default); E2FGVI_BF16 / E2FGVI_F16 (with the same mfma_dtype): the
                                          sources are 16-bit NHWC (src_ld multiple of 8): half the gather fetches           */
    int32_t src_planar;                /* 1 (16-bit sources, 16 channels per deform group): source s is laid out
                                          [src_c[s] / 16 groups][N*H*W pixels][16 channels] (e2fgvi_nhwc_to_planar16) instead
                                          of NHWC -- the 32-byte runs of neighbouring pixels of one group are then adjacent in
                                          memory, so the corner fetches of neighbouring output pixels share cache lines       */
} e2fgvi_mdcn_desc;

int e2fgvi_mdcn_nhwc(const e2fgvi_mdcn_desc* d, void* stream);
/* elements of the packing for mfma_dtype: one per weight slot (4 bytes for E2FGVI_F32, 2 for E2FGVI_BF16 / E2FGVI_F16, the same
 * count for all three), three bf16 planes whose sum is the fp32 weight for E2FGVI_BF16X3 (3 x that count) */
int64_t e2fgvi_packed_dcn_weight_size(int32_t mfma_dtype, int32_t Cout, int32_t C, int32_t KH, int32_t KW);
/* w: fp32 [Cout, C, KH, KW] */
int e2fgvi_pack_dcn_weight(const float* w, void* wpacked, int32_t mfma_dtype, int32_t Cout, int32_t C, int32_t KH, int32_t KW,
                           int32_t deform_groups, void* stream);

/* 16-bit NHWC [P pixels][C] (C a multiple of 16) -> [C / 16][P][16]: the deformable conv's planar source layout (src_planar) */
int e2fgvi_nhwc_to_planar16(const void* src, void* dst, int64_t P, int32_t C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Temporal focal window attention, fused (flash-style, fp32 MFMA, online softmax).
 * Replaces WindowAttention.forward's roll/partition/cat/bmm/softmax/bmm chain,
 * model/modules/tfocal_transformer.py:226-396 (window 5x9, 4 heads of 128).
 *   qkv    [B*T*fh*fw, 1536]  rows in (b,t,y,x) order, columns q|k|v (tfocal_transformer.py:221-223)
 *   kv_pool[B*T*nWin, 1536]   qkv Linear applied to the pooled window tokens (:319), rows (b,t,win)
 *   key_tab[nWin, tab_ld]     per window: `nkeys[win]` key references per frame:
 *                             v >= 0 : token y*fw+x of the same frame (own window + rolled ring,
 *                                      duplicates included, :235-283);  v < 0 : pooled window -(v+1)
 *   nkeys  [nWin]             valid references per frame; the remaining (210 - nkeys) pooled slots
 *                             are the zero-padded ones that score exactly -100 (:301-316,378-380)
 *   out    [B*T*fh*fw, 512]   attention output in token order (window_reverse :132 is implicit)
 * ---------------------------------------------------------------------------------------------- */
int e2fgvi_focal_attention(const float* qkv, const float* kv_pool, const int32_t* key_tab,
                           int32_t tab_ld, const int32_t* nkeys, float* out, int32_t B, int32_t T,
                           int32_t fh, int32_t fw, int32_t waves, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Small HBM-bound kernels
 * ---------------------------------------------------------------------------------------------- */
/* Tensors marked `void*` are fp32, bf16 or fp16 as the dtype argument beside them says; all arithmetic is fp32. */
/* fp32 [N,C,H,W] -> NHWC of dst_dtype with pixel stride ld (channels C..ld-1 zero-filled); y = x*scale + shift */
int e2fgvi_nchw_to_nhwc(const float* src, void* dst, int32_t dst_dtype, int32_t N, int32_t C, int32_t H, int32_t W,
                        int32_t ld, float scale, float shift, void* stream);
int e2fgvi_nhwc_to_nchw(const float* src, int32_t ld, float* dst, int32_t N, int32_t C, int32_t H,
                        int32_t W, void* stream);

/* Bilinear resize (torch F.interpolate semantics, align_corners 0/1), NHWC or NCHW source ->
 * NHWC destination, followed by a per-channel affine y = v*scale[c] + shift[c] (scale/shift may be
 * NULL).  Replaces e2fgvi.py:214-219 (1/4 downsample), flow_comp.py:150-167 (SPyNet resizes and
 * flow rescale), :121-124 (flow x2) and e2fgvi.py:126-129 (decoder x2).  src and dst are of dtype; the 16-bit types take
 * NHWC sources with channels and strides in multiples of 8 and no affine (E2FGVI_EUNSUP with src_nchw, scale or shift). */
int e2fgvi_resize_bilinear(const void* src, int32_t dtype, int32_t src_nchw, int32_t src_ld, void* dst,
                           int32_t dst_ld, int32_t N, int32_t C, int32_t H, int32_t W, int32_t Ho,
                           int32_t Wo, int32_t align_corners, const float* scale,
                           const float* shift, void* stream);

/* 2x2 mean pooling, NHWC (flow_comp.py:101-111) */
int e2fgvi_avgpool2_nhwc(const float* src, float* dst, int32_t N, int32_t H, int32_t W, int32_t C,
                         void* stream);

/* SPyNet level input (flow_comp.py:117-132): for pair n, out[n,y,x,0:8] =
 * [ref(3), warp_border(supp, flow_up)(3), flow_up(2)], flow_up = 2 * up2x_align_corners(flow_prev)
 * (zeros when flow_prev == NULL).  pyr: [F,h,w,4] per-frame pyramid level; ref_idx/supp_idx: [Np]
 * frame indices; flow_prev: [Np,h/2,w/2,2].  out16 (optional, NULL = none): the 8 channels again as [Np,h,w,8] of out16_dtype
 * (E2FGVI_BF16 / E2FGVI_F16), the source of the level's 16-bit conv stack. */
int e2fgvi_spynet_level_input(const float* pyr, const int32_t* ref_idx, const int32_t* supp_idx,
                              const float* flow_prev, float* out, void* out16, int32_t out16_dtype, int32_t Np,
                              int32_t h, int32_t w, void* stream);

/* Propagation step conditions (feat_prop.py:110-123): given feat_prop, feat_n2 [N,H,W,C] and the
 * flow fields flow_a (=flows[:,i-1]) and flow_b (=flows[:,i-2] or NULL), all NHWC, writes
 *   cond  [N,H,W,2C] = warp0(feat_prop, flow_n1) | warp0(feat_n2, flow_n2)   (zeros padding)
 *   flows [N,H,W,4]  = flow_n1 | flow_n2,  flow_n2 = flow_n1 + warp0(flow_b, flow_n1) (0 if NULL)
 * Each of the N images has its own flow image: flow_x + n*flow_img_stride.
 * The warp sources are of src_dtype: E2FGVI_F32 (cond of any cond_dtype) or E2FGVI_BF16 / E2FGVI_F16 (16-bit NHWC features, a cond
 * of the same type: half the gather bytes).  flows8_bf16 (optional): the [P,4] flows again as a 16-bit [P,8] conv source
 * (channels 4..7 zero) of the cond's type (bf16 beside an fp32 cond). */
int e2fgvi_prop_cond(const void* feat_prop, int32_t fp_ld, const void* feat_n2, int32_t f2_ld, int32_t src_dtype,
                     const float* flow_a, const float* flow_b, int64_t flow_img_stride, void* cond, int32_t cond_dtype,
                     float* flows, void* flows8_bf16, int32_t N, int32_t H, int32_t W, int32_t C, void* stream);

/* LayerNorm over the last dim (C = 256, 512, 768 or 1024, eps 1e-5, biased variance) of fp32 rows, y of y_dtype;
 * tfocal_transformer.py:452,463,470,533 */
int e2fgvi_layernorm(const float* x, const float* gamma, const float* beta, void* y, int32_t y_dtype, int64_t rows,
                     int32_t C, void* stream);

/* Window pooling Linear(45->1) (tfocal_transformer.py:508-516): x [B*T,fh,fw,C] tokens ->
 * pooled [B*T, fh/5, fw/9, C], both of dtype */
int e2fgvi_window_pool(const void* x, int32_t dtype, const float* w45, const float* bias1, void* pooled,
                       int32_t BT, int32_t fh, int32_t fw, int32_t C, void* stream);

/* FusionFeedForward middle (tfocal_transformer.py:82,92-97), all tensors of dtype: hid [F*fh*fw, C*49] ->
 * fold(7,3,3) / overlap count -> folded [F,H,W,C];  then unfold -> [F*fh*fw, C*49].  `gelu` says which of the two applies the
 * exact GELU: e2fgvi_ffn_fold(gelu = 0) + e2fgvi_ffn_unfold(gelu = 1) is the reference's order; fold(gelu = 1) + unfold(gelu = 0)
 * puts the GELU in front of the unfold (a gather with zero padding commutes with GELU, GELU(0) = 0): 5.4x fewer erf evaluations.
 * fp32: bit-identical either way; 16-bit: with the second order GELU sees the unrounded fold. */
int e2fgvi_ffn_fold(const void* hid, void* folded, int32_t dtype, int32_t gelu, int32_t F, int32_t fh, int32_t fw, int32_t H,
                    int32_t W, int32_t C, void* stream);
int e2fgvi_ffn_unfold(const void* folded, void* out, int32_t dtype, int32_t gelu, int32_t F, int32_t fh, int32_t fw,
                      int32_t H, int32_t W, int32_t C, void* stream);

/* SoftComp fold (tfocal_transformer.py:70-71): emb [F*fh*fw, C*49] -> overlap-ADD fold ->
 * [F,H,W,C] + bias_hwc[H,W,C] (optional, fp32) + residual (optional, NHWC ld = C); emb, residual and dst of dtype */
int e2fgvi_softcomp_fold(const void* emb, const float* bias_hwc, const void* residual,
                         void* dst, int32_t dtype, int32_t F, int32_t fh, int32_t fw, int32_t H, int32_t W,
                         int32_t C, void* stream);
/* element-wise fp32 <-> bf16 / fp16 conversion (round to nearest even; fp16: the bits of torch's .half(), overflow to +-inf,
 * subnormals kept), n a multiple of 4 */
int e2fgvi_cast(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LDS-DMA implicit-GEMM convolution / linear layer (csrc/conv_bf16x.hip): the 16-bit data paths (BASELINE.json configs 4 / 5:
 * e2fgvi_hq at 720p / 1080p, "bf16 MFMA") and the fp32 path's GEMM-shaped layers.  Same operators and call sites as
 * e2fgvi_conv2d_nhwc.  Activations are NHWC (element (n,y,x,c) at ((n*H+y)*W+x)*ld + c, ld in ELEMENTS); bias / residual /
 * activation are applied in fp32 and the result is stored as 16-bit and / or fp32.  `mode` of e2fgvi_conv2d_x and of the
 * packers names the operands:
 *   E2FGVI_BF16   bf16 sources (channels per source in multiples of 8), bf16 packed weights, v_mfma_f32_32x32x16_bf16, fp32
 *                 accumulation; 16-bit residual / dst / dst2 are bf16;
 *   E2FGVI_F16    the same with fp16 everywhere (v_mfma_f32_32x32x16_f16: same rate and layouts; tile codes 1-8, 11-18):
 *                 res_dtype / dst_dtype take E2FGVI_F32 or E2FGVI_F16, no split planes;
 *   E2FGVI_F32    fp32 sources (channels in multiples of 4), fp32 packed weights, v_mfma_f32_32x32x2_f32 (exact fp32, a K-step =
 *                 32 channels): the token Linears and SoftSplit / SoftComp, where it beats e2fgvi_conv2d_nhwc's register-staged
 *                 pipeline;
 *   E2FGVI_BF16X3 fp32 sources; every weight is stored as three bf16 numbers whose sum is the fp32 weight bit for bit (hi / mid /
 *                 lo, 8 significand bits each), every activation is split the same way in registers, and of the nine bf16
 *                 products of a*b the six largest are accumulated by v_mfma_f32_32x32x16_bf16 in fp32 (the three dropped ones
 *                 are < 2^-22 |a*b| together): fp32-level rounding at 2.7x the fp32 MFMA rate.  Tile codes 1..8 and 107 / 108
 *                 (the 256x256 / 256x192 tiles with the two halves of the workgroup one K-half-step apart: same bits as 7 / 8,
 *                 not for tap-packed weights), and 51 / 52: 7x7 stride-1 pad-3 layers from an LDS halo patch (16x16- / 8x16-pixel
 *                 tiles, the patch split once per 16-channel block instead of once per tap; sums in (block, tap) order): one source
 *                 of a multiple of 16 channels, groups = 1, Cout <= 64, plain packing, fp32 NHWC dst and residual, no
 *                 ACT_DCNPOST / dst2 / out_grid -- E2FGVI_EUNSUP otherwise.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const void* src[E2FGVI_MAX_SRC];   /* NHWC sources of the virtual concat, of the mode's source type         */
    int32_t src_ld[E2FGVI_MAX_SRC];    /* pixel stride, elements (multiple of 8)                           */
    int32_t src_coff[E2FGVI_MAX_SRC];  /* first channel used by group 0 (multiple of 8)                    */
    int32_t src_cpg[E2FGVI_MAX_SRC];   /* channels per group taken from this source (multiple of 8)        */
    int32_t nsrc;
    int32_t N, H, W, Ho, Wo;
    int32_t KH, KW, stride, pad;
    int32_t groups;
    int32_t Cout;
    const void* wpacked;               /* e2fgvi_pack_conv_weight_x with the same mode and tap_packed       */
    const float* bias;                 /* fp32 [Cout] or NULL                                               */
    const void* residual;              /* NHWC [N,Ho,Wo,*] of res_dtype, or the fp32 [P,4] flows of ACT_DCNPOST */
    int32_t res_ld, res_coff, res_dtype;
    void* dst;                         /* NHWC [N,Ho,Wo,dst_ld] of dst_dtype                                */
    int32_t dst_ld, dst_coff, dst_dtype;
    void* dst2;                        /* optional second copy of the result as 16-bit NHWC, or NULL        */
    int32_t dst2_ld, dst2_coff;
    int32_t act;
    float slope;
    int32_t tile;                      /* 0 = auto; rows x columns per workgroup: 1 = 128x128, 2 = 128x64, 3 = 128x32,
                                        * 4 = 64x128, 5 = 64x64, 6 = 256x128, 7 = 256x256, 8 = 256x192; + 10 (11-14, 16-18):
                                        * 3x3 stride-1 layers with one A stage per kernel row (bf16 operands only)      */
    int32_t dst_nchw;                  /* 1: dst is plain fp32 NCHW [N,Cout,Ho,Wo] (dst_ld / dst_coff ignored)  */
    int32_t tap_packed;                /* 1: wpacked was packed with tap_packed = 1; the row-shift tile codes do not apply */
    /* out_grid = 1 (zero: plain padding): Ho x Wo are taken as given, `pad` rows lie above and
     * `pad_left` columns left of the image and whatever else the KH x KW kernel reaches reads as zeros; with out_sy / out_sx > 0
     * output pixel (n, oy, ox) is stored -- and the residual read -- at pixel (oy*out_sy + out_py, ox*out_sx + out_px) of image n
     * of an [N, out_H, out_W] tensor.  res_bcast = 1: `residual` is ONE image ([out_H*out_W] or [Ho*Wo] rows) added to every
     * image of the batch.  Together: SoftComp in gather form -- nn.Fold(7x7, stride 3, pad 3) of Linear(512 -> 49*128)
     * (tfocal_transformer.py:49-72, tfocal_transformer_hq.py:49-79) as nine phase convolutions over the token grid, phase
     * (py, px) owning the pixels (3 ty + py, 3 tx + px): no [tokens, 6272] tensor (813 MB at 720p T=10 in bf16). */
    int32_t out_grid, pad_left;
    int32_t out_sy, out_sx, out_py, out_px, out_H, out_W;
    int32_t res_bcast;
    /* dst2_plane_stride > 0 (zero: dst2 is a plain copy; fp32 dst, groups = 1, no NCHW / scatter, not E2FGVI_F16):
     * output channels co >= dst2_split_from are NOT stored to dst; their EXACT three-way bf16 split (hi + mid + lo == the fp32
     * result, csrc/common.h e2_split2) goes to dst2 instead -- plane pl (0 = hi, 1 = mid, 2 = lo) of row m, channel co at
     * dst2[pl * dst2_plane_stride + m * dst2_ld + dst2_coff + co - dst2_split_from] (elements) -- and channels below
     * dst2_split_from go to dst only.  The qkv Linear of a transformer block writes the K / V operand planes of the
     * split-operand attention (e2fgvi_focal_attention_x3) this way: no separate e2fgvi_split3_kv pass over the rows
     * (tfocal_transformer.py:221-223: q = columns 0-511, k = 512-1023, v = 1024-1535). */
    int32_t dst2_split_from;
    int64_t dst2_plane_stride;
} e2fgvi_convx_desc;

int e2fgvi_conv2d_x(const e2fgvi_convx_desc* d, int32_t mode, void* stream);
/* Number of elements of the packed weight buffer for `mode`: 16-bit ones for E2FGVI_BF16 / E2FGVI_F16 (one layout, one count), fp32
 * ones for E2FGVI_F32, bf16 ones for E2FGVI_BF16X3 (3 x the E2FGVI_F32 count); negative for a geometry or a mode it rejects.
 * tap_packed = 0: [group][K-step][8 k-octets][Npad][8] (fp32: [4]; split: [K-step][plane][4 k-octets][Npad][8]), a K-step = 64
 * (fp32 sources: 32) input channels of one (tap, source), sources padded to a K-step, Npad = Cout/groups rounded up to 32.
 * tap_packed = 1, for narrow layers (groups == 1, nsrc == 1, src_cpg[0] = 8 ... 56 channels -- from 4 with fp32 sources --, KW >= 2:
 * SPyNet's 7x7 stacks model/modules/flow_comp.py:180-215, the encoder's first layer e2fgvi.py:76, the FFN's second Linear read as a
 * 7x7 stride-3 convolution of the folded tensor tfocal_transformer.py:81,95-97): the (tap, 8-channel chunk) pairs form one stream
 * cut into K-steps of 8 chunks -- 49 taps of 8 / 16 / 32 / 40 channels in 7 / 13 / 25 / 31 steps instead of 49 zero-padded ones
 * (fp32 sources: chunks of 4 channels, K-steps of 32: 40 channels = 10 chunks per tap, 62 steps instead of 98). */
int64_t e2fgvi_packed_conv_weight_x_size(int32_t mode, int32_t tap_packed, int32_t Cout, int32_t groups, int32_t KH, int32_t KW,
                                         int32_t nsrc, const int32_t* src_cpg);
/* w: fp32 [Cout, sum(cpg), KH, KW] (torch OIHW) */
int e2fgvi_pack_conv_weight_x(const float* w, void* wpacked, int32_t mode, int32_t tap_packed, int32_t Cout, int32_t groups,
                              int32_t KH, int32_t KW, int32_t nsrc, const int32_t* src_cpg, void* stream);

/* The Winograd F(2x2,3x3) kernel with split operands like E2FGVI_BF16X3 above (csrc/conv_wino.hip, X3 build): the transformed input and the
 * transformed weights are split exactly into three bf16 pieces each, six bf16 MFMA terms per product.  Same descriptor and
 * epilogues as e2fgvi_conv3x3_winograd; tile 0 (auto), 32, 132, 164; wpacked holds
 * e2fgvi_packed_winograd_weight_x3_size() bf16 elements ([group][16-channel stage][16 positions][plane][h][Npad][8]). */
int e2fgvi_conv3x3_winograd_x3(const e2fgvi_conv_desc* d, void* stream);
int64_t e2fgvi_packed_winograd_weight_x3_size(int32_t Cout, int32_t groups, int32_t nsrc, const int32_t* src_cpg);
int e2fgvi_pack_winograd_weight_x3(const float* w, void* wpacked, int32_t Cout, int32_t groups, int32_t nsrc,
                                   const int32_t* src_cpg, void* stream);

/* e2fgvi_focal_attention (fp32 in, fp32 softmax, fp32 out; tfocal_transformer.py:226-396) with both matrix
 * products on the bf16 matrix pipe as six exact bf16 terms of three-way split operands (csrc/attention_x3.hip).
 * e2fgvi_split3_kv: the k / v columns (512 .. 1535) of `rows` consecutive fp32 qkv rows -- the B*T*fh*fw token rows FOLLOWED by
 * the B*T*nWin pooled rows -- as three bf16 planes planes[3][rows][1024] whose sum is the fp32 value bit for bit.
 * e2fgvi_focal_attention_x3: qkv = the token rows (read for Q), planes = that buffer; waves: 0 (auto), 2, 4, 8 = waves of 32
 * queries per workgroup, 14 = four waves x two key groups (small grids: fewer than two query blocks per SIMD). */
int e2fgvi_split3_kv(const float* qkv_rows, void* planes, int64_t rows, void* stream);
int e2fgvi_focal_attention_x3(const float* qkv, const void* planes, const int32_t* key_tab, int32_t tab_ld, const int32_t* nkeys,
                              float* out, int32_t B, int32_t T, int32_t fh, int32_t fw, int32_t waves, void* stream);

/* Fused temporal focal window attention on 16-bit MFMA: qkv / kv_pool / out are of dtype (E2FGVI_BF16 or E2FGVI_F16; fp16: P
 * rounded to fp16 for the PV product) with the layouts of e2fgvi_focal_attention; scores, softmax statistics and accumulation
 * are fp32.  qkv and kv_pool must lie within one 4 GiB window (the engine allocates them back to back). */
int e2fgvi_focal_attention_16(const void* qkv, const void* kv_pool, const int32_t* key_tab, int32_t tab_ld,
                              const int32_t* nkeys, void* out, int32_t dtype, int32_t B, int32_t T, int32_t fh, int32_t fw,
                              void* stream);
/* Kernel variant of e2fgvi_focal_attention_16 for the following calls of this process (A/B measurements and the tests of
 * every instantiation): 0 = automatic, 1 = the register-staged kernel, 10 * QB + NW = the LDS-DMA kernel with NW
 * (2 / 4 / 8) waves of QB (1 / 2) x 32 queries per workgroup.  Returns the previous setting.  Same operator and results up to
 * fp32 summation order in every variant. */
int e2fgvi_focal_attention_16_variant(int variant);

#ifdef __cplusplus
}
#endif
#endif /* E2FGVI_HIP_H */
