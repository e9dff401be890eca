// What the input pipeline's kernels share (lf_pipeline.hip: resize_bilinear_kernel; lf_frame_stem.hip: frame_stem_kernel, the
// resize fused in front of the inference stem): the plan, the device table layout, Pillow's clip and the staging of a source window
// in LDS with its guard against the end of the frames buffer -- lf_stage_window for packed RGB frames, lf_stage_window_format for the
// other frame formats (BGR, NV12, YUYV), which leaves the SAME RGB triples in the same rows, so nothing behind the staging knows a format.
#pragma once
#include <stdint.h>

#include <vector>

#include "lf_common.h"
#include "lf_surface.h"      // lf_yuv_coef, lf_yuv_pixel; the surface layout and the staging group that knows it

#define PIL_PRECISION_BITS 22

struct lf_pipeline_plan {
    int format = LF_FRAME_RGB;           // LF_FRAME_*: what the frames buffer holds (lf_pipeline_plan_set_format)
    lf_yuv_coef coef = {65536, 0, 91881, 22554, 46802, 116130};
    int Hin, Win, crop_top, crop_h, out_h, out_w;
    int ksx, ksy;
    std::vector<int> bx, kx, by, ky;     // bilinear: bounds (first, count) and fixed-point weights
    std::vector<int> ntx, nty;           // nearest source index tables
    int tile_h, tile_w;                  // output tile per workgroup (shrunk until its input window fits the LDS budget)
    int max_rows, max_cols;              // largest input window of an output tile
    size_t lds_bytes;
    int in_stride;                       // LDS bytes per staged input row (dword aligned, + shift + tap over-read pad)
    long table_ints;
    // frame_stem_kernel (lf_frame_stem.hip): tile of STEM output pixels per workgroup, the largest source window of such a tile
    // (it covers the (2 th + 1) x (2 tw + 1) resized pixels the tile's 3x3 stride-2 patches read), its LDS bytes; fs_ok = 0: the
    // geometry does not fit (odd output size, or no tile whose window stays inside the LDS budget)
    int fs_ok, fs_th, fs_tw, fs_max_rows, fs_max_cols, fs_in_stride;
    size_t fs_lds_bytes;
    // lf_pipeline_plan_set_layout: the plan reads decoder surfaces (pitch, plane offsets, frame stride, plane pointers) and runs the
    // surface kernels (resize_surface_kernel, frame_surface_stem_kernel); false: tight frames, the kernels they always ran
    bool has_layout = false;
    lf_surface surf = {};
};

// fills the fs_* fields (lf_frame_stem.hip); called by lf_pipeline_plan_create
void lf_frame_stem_plan(lf_pipeline_plan* P);
// frames (N, Hin, Win, 3) uint8 -> cat (N, out_h / 2, out_w / 2, 16) NHWC fp32 / bf16: lf_pipeline_image + lf_stem_fwd_infer (Cin = 3)
// in one launch, the same bits.  Fails without launching where fs_ok is 0.
int lf_frame_stem_fwd_infer(const lf_pipeline_plan* P, const uint8_t* frames, int N, const void* tables_dev, const float* w, const float* b,
                            const float* sc, const float* sh, float* cat, int s16, hipStream_t st);

// bytes of one frame in the plan's format (pitch = width): the kernels' guard is pool_frames x this; on a layout plan the frame
// stride (the guard there: (pool_frames - 1) x stride + surf.frame_span)
inline size_t lf_plan_frame_bytes(const lf_pipeline_plan* P) {
    if (P->has_layout) return (size_t)P->surf.stride;
    const size_t px = (size_t)P->Hin * P->Win;
    return P->format == LF_FRAME_NV12 ? px / 2 * 3 : (P->format == LF_FRAME_YUYV ? px * 2 : px * 3);
}

// staged rows hold [shift <= 3][window][over-read of up to ksx taps], rounded to dwords
inline int lf_pipeline_in_stride(int max_cols, int ksx) { return (max_cols * 3 + 3 + ksx * 3 + 3) / 4 * 4; }

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> PIL_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// device table block layout (ints): bx[2*ow] kx[ow*ksx] by[2*oh] ky[oh*ksy] ntx[ow] nty[oh]
struct Tables {
    const int *bx, *kx, *by, *ky, *ntx, *nty;
};
__host__ __device__ inline Tables table_ptrs(const int* t, int oh, int ow, int ksx, int ksy) {
    Tables r;
    r.bx = t; r.kx = r.bx + 2 * ow; r.by = r.kx + (long)ow * ksx; r.ky = r.by + 2 * oh;
    r.ntx = r.ky + (long)oh * ksy; r.nty = r.ntx + ow;
    return r;
}

// Rows [row0, row0 + nr) x source columns [c0, c0 + ncb / 3) of frame `frame` -> s_in[r][in_stride], by aligned dword loads with a
// per-row byte shift (s_shift[r]): wave `wave` of four takes rows wave, wave + 4, ...  A dword that would reach past the end of the
// frames buffer (total_bytes) is put together from its bytes inside it.
__device__ __forceinline__ void lf_stage_window(const uint8_t* __restrict__ frames, size_t total_bytes, long frame, int Hin, int Win, int row0,
                                                int c0, int nr, int ncb, uint8_t* s_in, int in_stride, int* s_shift, int lane, int wave) {
    for (int r = wave; r < nr; r += 4) {
        const size_t g0 = (((size_t)frame * Hin + row0 + r) * Win + c0) * 3;
        const int sh = (int)(g0 & 3);
        const size_t a0 = g0 - sh;
        const int nd = (sh + ncb + 3) >> 2;
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_in + (size_t)r * in_stride);
        for (int d = lane; d < nd; d += 64) {
            const size_t byte = a0 + 4 * (size_t)d;
            uint32_t v;
            if (byte + 4 <= total_bytes) {
                v = *reinterpret_cast<const uint32_t*>(frames + byte);
            } else {
                v = 0;
                for (int e = 0; e < 4; ++e)
                    if (byte + e < total_bytes) v |= (uint32_t)frames[byte + e] << (8 * e);
            }
            dst[d] = v;
        }
        if (lane == 0) s_shift[r] = sh;
    }
}

// ---- the other frame formats ---------------------------------------------------------------------------------------------------
// An aligned dword of the frames buffer under lf_stage_window's guard: one that would reach past total_bytes is put together from
// its bytes inside the buffer (zero for the rest).  `byte` is a multiple of 4.
__device__ __forceinline__ uint32_t lf_frame_dword(const uint8_t* __restrict__ frames, size_t total_bytes, size_t byte) {
    if (byte + 4 <= total_bytes) return *reinterpret_cast<const uint32_t*>(frames + byte);
    uint32_t v = 0;
    for (int e = 0; e < 4; ++e)
        if (byte + e < total_bytes) v |= (uint32_t)frames[byte + e] << (8 * e);
    return v;
}
// the 8 bytes from the aligned dword at or below `byte` on, as one little-endian word
__device__ __forceinline__ uint64_t lf_frame_qword(const uint8_t* __restrict__ frames, size_t total_bytes, size_t byte) {
    const size_t a = byte & ~(size_t)3;
    return (uint64_t)lf_frame_dword(frames, total_bytes, a) | ((uint64_t)lf_frame_dword(frames, total_bytes, a + 4) << 32);
}

// (lf_clamp8 and lf_yuv_pixel: lf_surface.h, shared with the surface staging and its host check)

// lf_stage_window for FMT = LF_FRAME_BGR / _NV12 / _YUYV: the same rows x columns of frame `frame`, converted to RGB triples in
// registers and written to s_in[r] with shift 0 -- what lf_stage_window leaves for the converted frame, up to the shift.  A lane
// takes four consecutive pixels of the window (12 bytes, three dwords of the LDS row) and reads their source bytes as aligned
// dwords: three or four of the BGR row; two of the Y row and two of the interleaved CbCr row (chroma row y >> 1 of the FULL frame,
// pair x >> 1: replicated, a window may start inside a pair); the two or three Y0 Cb Y1 Cr dwords of YUYV.
// Bounds.  Loads: every one goes through lf_frame_dword, so none reaches past total_bytes = pool_frames x lf_plan_frame_bytes,
// whatever the lane's pixels are -- the last group of a row may hold up to three pixels beyond the window, whose bytes then come
// from the next row, plane or frame, or are zero past the end; they land in the row's over-read pad, which only zero weights meet.
// Stores: (ncb / 3 + 3) / 4 * 12 <= ncb + 9 <= max_cols * 3 + 3 + ksx * 3 <= in_stride bytes of row r, as ksx >= 3 for every plan
// (Pillow's ksize = 2 ceil(support) + 1, support >= 1) -- inside the row lf_pipeline_in_stride sized, next to no other wave's.
template <int FMT>
__device__ __forceinline__ void lf_stage_window_format(const uint8_t* __restrict__ frames, size_t total_bytes, long frame, int Hin, int Win,
                                                       int row0, int c0, int nr, int ncb, uint8_t* s_in, int in_stride, int* s_shift, int lane,
                                                       int wave, const lf_yuv_coef cf) {
    static_assert(FMT == LF_FRAME_BGR || FMT == LF_FRAME_NV12 || FMT == LF_FRAME_YUYV, "packed RGB frames go through lf_stage_window");
    const int ng = (ncb / 3 + 3) >> 2;
    const size_t plane = (size_t)Hin * Win;
    for (int r = wave; r < nr; r += 4) {
        const int y = row0 + r;
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_in + (size_t)r * in_stride);
        for (int g = lane; g < ng; g += 64) {
            const int x0 = c0 + 4 * g;
            uint32_t px[4];
            if (FMT == LF_FRAME_BGR) {
                const size_t g0 = (((size_t)frame * Hin + y) * Win + x0) * 3;
                const int sh = 8 * (int)(g0 & 3);
                const size_t a0 = g0 & ~(size_t)3;
                const uint64_t d0 = lf_frame_dword(frames, total_bytes, a0), d1 = lf_frame_dword(frames, total_bytes, a0 + 4);
                const uint64_t d2 = lf_frame_dword(frames, total_bytes, a0 + 8), d3 = sh ? lf_frame_dword(frames, total_bytes, a0 + 12) : 0;
                const uint32_t w0 = (uint32_t)((d0 | (d1 << 32)) >> sh), w1 = (uint32_t)((d1 | (d2 << 32)) >> sh);
                const uint32_t w2 = (uint32_t)((d2 | (d3 << 32)) >> sh);
                const uint32_t p[4] = {w0 & 0xffffffu, (w0 >> 24) | ((w1 & 0xffffu) << 8), (w1 >> 16) | ((w2 & 0xffu) << 16), w2 >> 8};
#pragma unroll
                for (int i = 0; i < 4; ++i) px[i] = ((p[i] & 0xffu) << 16) | (p[i] & 0xff00u) | (p[i] >> 16);      // B G R -> R G B
            } else if (FMT == LF_FRAME_NV12) {
                const size_t fb = (size_t)frame * (plane / 2 * 3);
                const size_t ya = fb + (size_t)y * Win + x0, ca = fb + plane + (size_t)(y >> 1) * Win + (x0 & ~1);
                const uint64_t qy = lf_frame_qword(frames, total_bytes, ya) >> (8 * (int)(ya & 3));
                const uint64_t qc = lf_frame_qword(frames, total_bytes, ca) >> (8 * (int)(ca & 3));      // ca is even: 0 or 2 bytes
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int pair = 8 * (((x0 & 1) + i) & ~1);                   // 0, 2 or 4 bytes behind the first pair: <= 6 + 1 < 8
                    px[i] = lf_yuv_pixel((int)((qy >> (8 * i)) & 255), (int)((qc >> pair) & 255), (int)((qc >> (pair + 8)) & 255), cf);
                }
            } else {
                // Win even: every Y0 Cb Y1 Cr group is an aligned dword
                const size_t pa = ((size_t)frame * plane + (size_t)y * Win + (x0 & ~1)) * 2;
                const uint32_t d0 = lf_frame_dword(frames, total_bytes, pa), d1 = lf_frame_dword(frames, total_bytes, pa + 4);
                const uint32_t d2 = (x0 & 1) ? lf_frame_dword(frames, total_bytes, pa + 8) : 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = (x0 & 1) + i;                                   // 0 .. 4: pixel k of the three groups
                    const uint32_t d = k < 2 ? d0 : (k < 4 ? d1 : d2);
                    px[i] = lf_yuv_pixel((int)((d >> (16 * (k & 1))) & 255), (int)((d >> 8) & 255), (int)(d >> 24), cf);
                }
            }
            dst[3 * g] = px[0] | (px[1] << 24);
            dst[3 * g + 1] = (px[1] >> 8) | (px[2] << 16);
            dst[3 * g + 2] = (px[2] >> 16) | (px[3] << 8);
        }
        if (lane == 0) s_shift[r] = 0;
    }
}

// ---- decoder surfaces ------------------------------------------------------------------------------------------------------------
// lf_stage_window_format for a plan with a layout (lf_pipeline_plan_set_layout), FMT = any LF_FRAME_*: the same rows x columns of
// frame `frame`, from planes with their own pitch and offset, or from the plane pointers of row `frame` of a pointer table; the
// same RGB triples in the same LDS rows, shift 0.  A lane takes four consecutive pixels (lf_surface_group, lf_surface.h -- the code
// the host check runs over exact-size heap buffers); pitch, offsets, stride and the mode are runtime values of S.
// Bounds.  Loads: every one is an aligned dword through `ld`, which knows how many bytes are left behind its address and touches
// none beyond.  Contiguous mode: left counts to total_bytes = (pool_frames - 1) x stride + frame_span behind `frames`, whatever the
// lane's pixels are; rounding an address down stays at or behind `frames` (4-byte aligned).  Pointer mode: left counts to span_p =
// (rows_p - 1) pitch_p + row bytes_p behind the plane's pointer, so the last group of a plane's last row reads inside the plane or
// takes zeros.  A 4-byte aligned pointer makes rounding down stay inside the plane.  The NV12 CbCr pointer may be 2-byte aligned:
// its first fetch then loads the aligned dword 2 bytes IN FRONT of the plane -- the dword that also holds the plane's bytes 0 and 1,
// so the load touches no granule the plane does not touch and cannot fault; the two foreign bytes are shifted out before use and
// reach no result (tests: a CbCr base at + 2 on the host and on the device).  That one read is outside "inside the plane or zero".
// A pitch is below 2^31.  In both
// modes the up to three pixels of a row's last group beyond the window take padding bytes, bytes of the next row, or zeros; they
// land in the row's over-read pad, which only zero weights meet -- no padding byte reaches a result.  frame < pool_frames (the
// callers clamp an index outside the pool to 0) and rows stay below Hin, so the largest address of plane p is that of its last row.
// Stores: as lf_stage_window_format, (ncb / 3 + 3) / 4 * 12 <= in_stride bytes of row r.
template <int FMT>
__device__ __forceinline__ void lf_stage_surface(const uint8_t* __restrict__ frames, size_t total_bytes, const lf_surface& S, long frame, int row0,
                                                 int c0, int nr, int ncb, uint8_t* s_in, int in_stride, int* s_shift, int lane, int wave,
                                                 const lf_yuv_coef cf) {
    const int ng = (ncb / 3 + 3) >> 2;
    lf_plane pl[3];
    lf_surface_planes_of(S, frames, total_bytes, frame, pl);
    // lf_frame_dword with the buffer's end `left` bytes behind the dword: whole inside, or put together from its bytes inside
    const auto ld = [](const uint8_t* a, long left) { return left <= 0 ? 0u : lf_frame_dword(a, (size_t)left, 0); };
    for (int r = wave; r < nr; r += 4) {
        const int y = row0 + r;
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_in + (size_t)r * in_stride);
        for (int g = lane; g < ng; g += 64) {
            uint32_t o[3];
            lf_surface_group<FMT>(ld, pl, y, c0 + 4 * g, cf, o);
            dst[3 * g] = o[0];
            dst[3 * g + 1] = o[1];
            dst[3 * g + 2] = o[2];
        }
        if (lane == 0) s_shift[r] = 0;
    }
}
