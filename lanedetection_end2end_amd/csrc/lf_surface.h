// Decoder surfaces (include/lanefit.h, "additions since 5 -- surfaces"): the frame layout of a pipeline plan resolved to numbers, and
// the part of the surface staging that knows it -- which bytes of which plane the four pixels of a staging group are, and the RGB
// triples they become.  Everything here compiles for the device AND for a plain host compiler (no HIP header, no HIP type): the
// kernels (lf_pipeline_dev.h: lf_stage_surface) and the stand-alone host check (tests/surface_stage_host.cpp) run the SAME
// lf_surface_group, the kernels through aligned dword loads under the end-of-buffer guard, the host check through a loader that
// asserts the extent of every load against an allocation of exactly the bytes the contract grants.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LF_HD __host__ __device__ __forceinline__
#define LF_UNROLL _Pragma("unroll")
#else
#define LF_HD inline
#define LF_UNROLL
#endif

// format codes of include/lanefit.h, restated so that this header stands without it (lf_pipeline.hip static_asserts the match)
enum { LF_SURF_RGB = 0, LF_SURF_BGR = 1, LF_SURF_NV12 = 2, LF_SURF_YUYV = 3, LF_SURF_I420 = 4, LF_SURF_RGBX = 5, LF_SURF_BGRX = 6 };

// YCbCr -> RGB in Q16 (include/lanefit.h, "additions since 5 -- frame formats"); passed to the kernels by value
struct lf_yuv_coef {
    int c_y, y_off, c_rv, c_gu, c_gv, c_bu;
};

LF_HD int lf_clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// one pixel as R | G << 8 | B << 16: the Q16 definition of include/lanefit.h, arithmetic shift (floor), int32 throughout
LF_HD uint32_t lf_yuv_pixel(int Y, int Cb, int Cr, const lf_yuv_coef& k) {
    const int yy = k.c_y * (Y - k.y_off) + 32768, u = Cb - 128, v = Cr - 128;
    const int R = lf_clamp8((yy + k.c_rv * v) >> 16);
    const int G = lf_clamp8((yy - k.c_gu * u - k.c_gv * v) >> 16);
    const int B = lf_clamp8((yy + k.c_bu * u) >> 16);
    return (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
}

// lf_yuv_pixel for the surface staging, behind a barrier the optimiser cannot see through, then cut to its three bytes.  Why it is
// here: without it the YCbCr surface kernels gave wrong bytes on the device (single bytes of the staged row -- a pixel's blue, the
// next pixel's red -- came out OR-ed with other bits) while this very code was right on the host.  The cause was NOT established.
// What is known: without the barrier the compiler forms R | G << 8 with gfx950's packed shift-and-saturate (v_ashr_pk_u8_i32), with
// it no surface kernel contains that instruction, and with it every bit-exact GPU test passes.  The tight NV12 kernels contain the
// instruction and pass their bit-exact tests, so the instruction alone does not explain it.  The barrier stays because the tests
// pass with it; it costs no instruction, the mask at most one v_and per pixel.
LF_HD uint32_t lf_surface_pixel(int Y, int Cb, int Cr, const lf_yuv_coef& k) {
    uint32_t p = lf_yuv_pixel(Y, Cb, Cr, k);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(p));
#endif
    return p & 0xffffffu;
}

// A layout with every default resolved (no zero left): what lf_pipeline_plan_set_layout stores and the kernels take by value.
struct lf_surface {
    long pitch[3];       // bytes between rows of plane p
    long off[3];         // bytes from a frame's base to plane p (contiguous mode)
    long span[3];        // (rows_p - 1) pitch_p + row bytes_p: what a plane pointer grants (pointer mode)
    long stride;         // bytes between frames (contiguous mode)
    long frame_span;     // the furthest byte of one frame: max over p of off_p + span_p
    int planes, ptrs;    // 1..3; 1 = `frames` is a device array (N, planes) of plane base pointers
};

LF_HD int lf_surface_planes(int fmt) { return fmt == LF_SURF_I420 ? 3 : (fmt == LF_SURF_NV12 ? 2 : 1); }
LF_HD long lf_surface_rows(int fmt, int p, int H) { return p == 0 ? H : H / 2; }
LF_HD long lf_surface_row_bytes(int fmt, int p, int W) {
    if (p > 0) return fmt == LF_SURF_NV12 ? W : W / 2;
    return fmt == LF_SURF_RGB || fmt == LF_SURF_BGR ? 3L * W : (fmt == LF_SURF_YUYV ? 2L * W : (fmt >= LF_SURF_RGBX ? 4L * W : W));
}

// Resolves a layout (pitch / plane_offset / frame_stride as the caller gave them, 0 = default) for Hin x Win frames of format fmt.
// Returns NULL and fills *S, or the reason it is refused.  The alignment rules are what lf_surface_group relies on:
//   YUYV, RGBX, BGRX  pitch, frame stride multiples of 4: every Y0 Cb Y1 Cr group / every pixel is ONE aligned dword;
//   NV12              chroma pitch, chroma offset AND the frame stride even: a Cb Cr pair never straddles the 8 bytes a lane fetches
//                     (the stride moves the chroma plane of every frame behind the first, so it is held to the same rule).
// Pointer mode (ptrs) reads neither plane_offset nor frame_stride: they are not looked at, whatever they hold, and the resolved
// offsets and stride are those of the defaults (lf_pipeline_frame_bytes still answers).  Values of planes the format lacks are
// not looked at in either mode.
inline const char* lf_surface_resolve(int fmt, int Hin, int Win, const long pitch[3], const long plane_offset[3], long frame_stride, int ptrs,
                                      lf_surface* S) {
    if (fmt < LF_SURF_RGB || fmt > LF_SURF_BGRX) return "unknown format";
    if ((fmt == LF_SURF_NV12 || fmt == LF_SURF_I420) && ((Hin | Win) & 1)) return "NV12 / I420 frames need an even height and width";
    if (fmt == LF_SURF_YUYV && (Win & 1)) return "YUYV frames need an even width";
    const long no_offsets[3] = {0, 0, 0};
    if (ptrs) {
        plane_offset = no_offsets;
        frame_stride = 0;
    }
    if (frame_stride < 0) return "negative frame stride";
    if (plane_offset[0] != 0) return "plane_offset[0] must be 0";
    lf_surface R = {};
    R.planes = lf_surface_planes(fmt);
    R.ptrs = ptrs ? 1 : 0;
    const bool dword = fmt == LF_SURF_YUYV || fmt >= LF_SURF_RGBX;
    long tight_end = 0;
    for (int p = 0; p < R.planes; ++p) {
        const long rows = lf_surface_rows(fmt, p, Hin), rb = lf_surface_row_bytes(fmt, p, Win);
        if (pitch[p] < 0 || plane_offset[p] < 0) return "negative pitch or plane offset";
        if (pitch[p] != 0 && pitch[p] < rb) return "pitch below the bytes of a row";
        if (pitch[p] > 0x7fffffffL) return "pitch of 2^31 bytes or more";
        R.pitch[p] = pitch[p] ? pitch[p] : rb;
        R.off[p] = p == 0 ? 0 : (plane_offset[p] ? plane_offset[p] : R.off[p - 1] + lf_surface_rows(fmt, p - 1, Hin) * R.pitch[p - 1]);
        R.span[p] = (rows - 1) * R.pitch[p] + rb;
        const long po = ptrs ? R.pitch[p] : (R.pitch[p] | R.off[p]);      // pointer mode: the pointer's alignment is the caller's contract
        if (dword && (po & 3)) return "YUYV / RGBX / BGRX surfaces need pitch and plane offset in multiples of 4";
        if (fmt == LF_SURF_NV12 && p == 1 && (po & 1)) return "the NV12 chroma plane needs an even pitch and offset";
        if (R.off[p] + R.span[p] > R.frame_span) R.frame_span = R.off[p] + R.span[p];
        if (R.off[p] + rows * R.pitch[p] > tight_end) tight_end = R.off[p] + rows * R.pitch[p];
    }
    R.stride = frame_stride ? frame_stride : tight_end;
    if (!ptrs && dword && (R.stride & 3)) return "YUYV / RGBX / BGRX surfaces need a frame stride in multiples of 4";
    if (!ptrs && fmt == LF_SURF_NV12 && (R.stride & 1)) return "NV12 surfaces need an even frame stride (it moves the chroma plane)";
    *S = R;
    return nullptr;
}

// One plane of one frame as the staging sees it: p = its first byte, left = the bytes the contract grants from p on, pitch.
// Contiguous mode: p = frames + frame x stride + off_p, left = the end of the whole batch - that.  Pointer mode: p = the plane's
// pointer, left = span_p.  Three values per plane: the scalar registers of the three-plane kernels are few.
struct lf_plane {
    const uint8_t* p;
    long left;
    int pitch;
};

// The aligned dword at byte `off` of the plane (p + off a multiple of 4; off may be -1 .. -3 where p itself is not aligned: in
// contiguous mode that lies inside the batch, whose base is aligned; in pointer mode only the NV12 CbCr pointer may be 2-byte
// aligned, and the dword two bytes in front of it is the aligned dword that also holds the plane's first two bytes).  LD is the loader: ld(a, left) -> the dword at a, with
// zeros for the bytes at or beyond a + left (left may be <= 0: nothing is read).
template <class LD>
LF_HD uint32_t lf_plane_dword(const LD& ld, const lf_plane& P, long off) { return ld(P.p + off, P.left - off); }

// `need` <= 8 - shift bytes from byte `off` of the plane on, little-endian, by one aligned dword load or two.
template <class LD>
LF_HD uint64_t lf_surface_fetch(const LD& ld, const lf_plane& P, long off, int need) {
    const int sh = (int)((uintptr_t)(P.p + off) & 3);
    uint64_t q = lf_plane_dword(ld, P, off - sh);
    if (sh + need > 4) q |= (uint64_t)lf_plane_dword(ld, P, off - sh + 4) << 32;
    return q >> (8 * sh);
}

// The four pixels x0 .. x0 + 3 of row y -> the three dwords (R G B R | G B R G | B R G B) lf_stage_window leaves in LDS for them.
// Pixels at or beyond the row's end take whatever follows inside the guard (padding, the next row) or zero: the caller lets them
// land in the over-read pad of the staged row only.
//   RGB / BGR   12 bytes from byte 3 x0 of the row, any alignment: three or four dwords;
//   RGBX / BGRX four aligned dwords, the fourth byte dropped;
//   YUYV        the two or three aligned Y0 Cb Y1 Cr dwords that hold the pixels;
//   NV12        4 Y bytes; the 4 or 6 bytes of the two or three Cb Cr pairs (chroma row y >> 1, pair x >> 1), an even address;
//   I420        4 Y bytes; 2 or 3 bytes of each chroma plane (row y >> 1, sample x >> 1), any alignment -- a lane's two chroma
//               bytes come out of the aligned dword that holds them (and its neighbour where they straddle), never a byte load.
template <int FMT, class LD>
LF_HD void lf_surface_group(const LD& ld, const lf_plane* pl, int y, int x0, const lf_yuv_coef& cf, uint32_t out[3]) {
    uint32_t px[4];
    const long row = (long)y * pl[0].pitch;
    if (FMT == LF_SURF_RGB || FMT == LF_SURF_BGR) {
        const long g0 = row + (long)x0 * 3;
        const int bs = (int)((uintptr_t)(pl[0].p + g0) & 3), sh = 8 * bs;
        const long a0 = g0 - bs;
        const uint64_t d0 = lf_plane_dword(ld, pl[0], a0), d1 = lf_plane_dword(ld, pl[0], a0 + 4);
        const uint64_t d2 = lf_plane_dword(ld, pl[0], a0 + 8), d3 = sh ? lf_plane_dword(ld, pl[0], a0 + 12) : 0;
        const uint32_t w0 = (uint32_t)((d0 | (d1 << 32)) >> sh), w1 = (uint32_t)((d1 | (d2 << 32)) >> sh);
        const uint32_t w2 = (uint32_t)((d2 | (d3 << 32)) >> sh);
        if (FMT == LF_SURF_RGB) {
            out[0] = w0; out[1] = w1; out[2] = w2;
            return;
        }
        const uint32_t p[4] = {w0 & 0xffffffu, (w0 >> 24) | ((w1 & 0xffffu) << 8), (w1 >> 16) | ((w2 & 0xffu) << 16), w2 >> 8};
        LF_UNROLL
        for (int i = 0; i < 4; ++i) px[i] = ((p[i] & 0xffu) << 16) | (p[i] & 0xff00u) | (p[i] >> 16);      // B G R -> R G B
    } else if (FMT == LF_SURF_RGBX || FMT == LF_SURF_BGRX) {
        const long a = row + (long)x0 * 4;                                // an aligned address (lf_surface_resolve)
        LF_UNROLL
        for (int i = 0; i < 4; ++i) {
            const uint32_t d = lf_plane_dword(ld, pl[0], a + 4 * i);
            px[i] = FMT == LF_SURF_RGBX ? d & 0xffffffu : ((d & 0xffu) << 16) | (d & 0xff00u) | ((d >> 16) & 0xffu);
        }
    } else if (FMT == LF_SURF_YUYV) {
        const long pa = row + (long)(x0 & ~1) * 2;                        // an aligned address
        const uint32_t d0 = lf_plane_dword(ld, pl[0], pa), d1 = lf_plane_dword(ld, pl[0], pa + 4);
        const uint32_t d2 = (x0 & 1) ? lf_plane_dword(ld, pl[0], pa + 8) : 0;
        LF_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int k = (x0 & 1) + i;                                   // 0 .. 4: pixel k of the three groups
            const uint32_t d = k < 2 ? d0 : (k < 4 ? d1 : d2);
            px[i] = lf_surface_pixel((int)((d >> (16 * (k & 1))) & 255), (int)((d >> 8) & 255), (int)(d >> 24), cf);
        }
    } else if (FMT == LF_SURF_NV12) {
        const uint64_t qy = lf_surface_fetch(ld, pl[0], row + x0, 4);
        // the address is even (lf_surface_resolve; the pointer contract): shift 0 or 2, so the 4 or 6 bytes fit the two dwords
        const uint64_t qc = lf_surface_fetch(ld, pl[1], (long)(y >> 1) * pl[1].pitch + (x0 & ~1), 4 + 2 * (x0 & 1));
        LF_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int pair = 8 * (((x0 & 1) + i) & ~1);                   // 0, 2 or 4 bytes behind the first pair
            px[i] = lf_surface_pixel((int)((qy >> (8 * i)) & 255), (int)((qc >> pair) & 255), (int)((qc >> (pair + 8)) & 255), cf);
        }
    } else {
        const uint64_t qy = lf_surface_fetch(ld, pl[0], row + x0, 4);
        const uint64_t qu = lf_surface_fetch(ld, pl[1], (long)(y >> 1) * pl[1].pitch + (x0 >> 1), 2 + (x0 & 1));
        const uint64_t qv = lf_surface_fetch(ld, pl[2], (long)(y >> 1) * pl[2].pitch + (x0 >> 1), 2 + (x0 & 1));
        LF_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int s = 8 * (((x0 & 1) + i) >> 1);                      // sample 0, 1 or 2 behind the first
            px[i] = lf_surface_pixel((int)((qy >> (8 * i)) & 255), (int)((qu >> s) & 255), (int)((qv >> s) & 255), cf);
        }
    }
    out[0] = px[0] | (px[1] << 24);
    out[1] = (px[1] >> 8) | (px[2] << 16);
    out[2] = (px[2] >> 16) | (px[3] << 8);
}

// The planes of frame `frame`: contiguous mode from the layout's numbers, pointer mode from row `frame` of the pointer table.
LF_HD void lf_surface_planes_of(const lf_surface& S, const uint8_t* frames, size_t total_bytes, long frame, lf_plane pl[3]) {
    for (int p = 0; p < 3; ++p) {
        if (p >= S.planes) { pl[p] = pl[0]; continue; }
        if (S.ptrs) {
            pl[p].p = reinterpret_cast<const uint8_t* const*>(frames)[frame * S.planes + p];
            pl[p].left = S.span[p];
        } else {
            const long org = frame * S.stride + S.off[p];
            pl[p].p = frames + org;
            pl[p].left = (long)total_bytes - org;
        }
        pl[p].pitch = (int)S.pitch[p];
    }
}
