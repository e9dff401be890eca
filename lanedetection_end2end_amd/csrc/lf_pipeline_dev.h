// What the input pipeline's kernels share (lf_pipeline.hip: resize_bilinear_kernel; lf_frame_stem.hip: frame_stem_kernel, the
// resize fused in front of the inference stem): the plan, the device table layout, Pillow's clip and the staging of a source window
// in LDS with its guard against the end of the frames buffer.
#pragma once
#include <stdint.h>

#include <vector>

#include "lf_common.h"

#define PIL_PRECISION_BITS 22

struct lf_pipeline_plan {
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
};

// fills the fs_* fields (lf_frame_stem.hip); called by lf_pipeline_plan_create
void lf_frame_stem_plan(lf_pipeline_plan* P);
// frames (N, Hin, Win, 3) uint8 -> cat (N, out_h / 2, out_w / 2, 16) NHWC fp32 / bf16: lf_pipeline_image + lf_stem_fwd_infer (Cin = 3)
// in one launch, the same bits.  Fails without launching where fs_ok is 0.
int lf_frame_stem_fwd_infer(const lf_pipeline_plan* P, const uint8_t* frames, int N, const void* tables_dev, const float* w, const float* b,
                            const float* sc, const float* sh, float* cat, int s16, hipStream_t st);

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
