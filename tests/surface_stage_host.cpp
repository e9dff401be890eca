// Stand-alone host check of the surface staging's address arithmetic (csrc/lf_surface.h: lf_surface_resolve, lf_surface_planes_of,
// lf_surface_group -- the code the kernels run).  Built and run by tests/test_surfaces_cpu.py, with the address and undefined-behaviour
// sanitizers where the host compiler has them; the asserts below are the check either way.
//   - every format, the kernel-level geometries and the four layouts of tests/test_surfaces_gpu.py (padded pitches; + gaps before the
//     later planes; + a frame stride with a gap; plane pointers), N = 3;
//   - the surface lives in heap buffers of EXACTLY batch_bytes / span(p) bytes, and every load goes through a loader that asserts
//     the dword is aligned and that each byte it touches lies inside one of them;
//   - the staged rows (every window start 0 .. 4 and the five-pixel window that ends at the row's end, every row of the crop) are compared with
//     a plain per-pixel loop over the same buffers.
#include <assert.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "lf_surface.h"

struct Alloc { const uint8_t* p; size_t n; };
static std::vector<Alloc> g_allocs;
static long g_loads = 0, g_partial = 0;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); abort(); } \
    } while (0)

struct CheckedLoad {
    uint32_t operator()(const uint8_t* a, long left) const {
        CHECK(((uintptr_t)a & 3) == 0);
        ++g_loads;
        if (left <= 0) return 0;
        const size_t n = left >= 4 ? 4 : (size_t)left;
        if (n < 4) ++g_partial;
        bool inside = false;
        for (const Alloc& A : g_allocs) inside = inside || (a >= A.p && a + n <= A.p + A.n);
        CHECK(inside);
        uint32_t v = 0;
        for (size_t e = 0; e < n; ++e) v |= (uint32_t)a[e] << (8 * e);
        return v;
    }
};

static uint32_t g_seed = 12345;
static uint8_t rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (uint8_t)(g_seed >> 24); }

// the definition, one pixel at a time, straight from the planes
static void pixel(int fmt, const lf_plane* pl, int y, int x, const lf_yuv_coef& cf, uint8_t rgb[3]) {
    const uint8_t* r0 = pl[0].p + (long)y * pl[0].pitch;
    if (fmt == LF_SURF_RGB || fmt == LF_SURF_BGR || fmt == LF_SURF_RGBX || fmt == LF_SURF_BGRX) {
        const int bpp = fmt >= LF_SURF_RGBX ? 4 : 3;
        const bool swap = fmt == LF_SURF_BGR || fmt == LF_SURF_BGRX;
        for (int c = 0; c < 3; ++c) rgb[c] = r0[x * bpp + (swap ? 2 - c : c)];
        return;
    }
    int Y, Cb, Cr;
    if (fmt == LF_SURF_YUYV) {
        Y = r0[2 * x]; Cb = r0[4 * (x >> 1) + 1]; Cr = r0[4 * (x >> 1) + 3];
    } else if (fmt == LF_SURF_NV12) {
        const uint8_t* c = pl[1].p + (long)(y >> 1) * pl[1].pitch + 2 * (x >> 1);
        Y = r0[x]; Cb = c[0]; Cr = c[1];
    } else {
        Y = r0[x];
        Cb = pl[1].p[(long)(y >> 1) * pl[1].pitch + (x >> 1)];
        Cr = pl[2].p[(long)(y >> 1) * pl[2].pitch + (x >> 1)];
    }
    const long long yy = (long long)cf.c_y * (Y - cf.y_off) + 32768, u = Cb - 128, v = Cr - 128;
    const long long s[3] = {yy + cf.c_rv * v, yy - cf.c_gu * u - cf.c_gv * v, yy + cf.c_bu * u};
    for (int c = 0; c < 3; ++c) {
        long long t = s[c] >> 16;
        rgb[c] = (uint8_t)(t < 0 ? 0 : (t > 255 ? 255 : t));
    }
}

// layout 5: layout 4 (plane pointers) with every NV12 CbCr plane at + 2 of its allocation -- the contract lets that pointer be 2-byte
// aligned, and the staging then loads the aligned dword that starts 2 bytes in front of the plane (lf_pipeline_dev.h, Bounds); the
// allocation is the plane's span + those 2 bytes, so the asserts still hold every load to memory the program owns
template <int FMT>
static long run(int H, int W, int top, int ch, int layout, const lf_yuv_coef& cf) {
    const int front = layout == 5 ? 2 : 0;
    if (layout == 5) layout = 4;
    const int N = 3, planes = lf_surface_planes(FMT);
    // the padded pitches of tests/test_surfaces_gpu.py, odd where legal
    static const int pad[7][3] = {{5, 0, 0}, {5, 0, 0}, {6, 10, 0}, {12, 0, 0}, {3, 1, 1}, {12, 0, 0}, {12, 0, 0}};
    long pitch[3] = {0, 0, 0}, off[3] = {0, 0, 0}, stride = 0;
    for (int p = 0; p < planes; ++p) pitch[p] = lf_surface_row_bytes(FMT, p, W) + pad[FMT][p];
    if (layout >= 2 && layout <= 3)
        for (int p = 1; p < planes; ++p) off[p] = off[p - 1] + (lf_surface_rows(FMT, p - 1, H) + 3) * pitch[p - 1] + (p == 2 ? 2 * pitch[p] : 0);
    if (FMT == LF_SURF_NV12 && (off[1] & 1)) off[1] += 1;
    lf_surface S;
    const char* why = lf_surface_resolve(FMT, H, W, pitch, off, 0, layout == 4, &S);
    CHECK(!why);
    if (layout == 3) {
        stride = S.stride + 3 * S.pitch[0] + 8;
        why = lf_surface_resolve(FMT, H, W, pitch, off, stride, 0, &S);
        CHECK(!why);
    }
    // exact-size heap buffers, every byte (padding included) random
    g_allocs.clear();
    std::vector<uint8_t*> bufs;
    std::vector<const uint8_t*> table;
    const uint8_t* frames;
    size_t total = 0;
    if (S.ptrs) {
        for (int n = 0; n < N; ++n)
            for (int p = 0; p < planes; ++p) {
                const size_t lead = p == 1 ? front : 0, bytes = (size_t)S.span[p] + lead;
                uint8_t* b = (uint8_t*)malloc(bytes);
                CHECK(b && ((uintptr_t)b & 3) == 0);
                for (size_t i = 0; i < bytes; ++i) b[i] = rnd();
                bufs.push_back(b);
                g_allocs.push_back({b, bytes});
                table.push_back(b + lead);
            }
        frames = reinterpret_cast<const uint8_t*>(table.data());
    } else {
        total = (size_t)(N - 1) * S.stride + S.frame_span;
        uint8_t* b = (uint8_t*)malloc(total);
        CHECK(b);
        for (size_t i = 0; i < total; ++i) b[i] = rnd();
        bufs.push_back(b);
        g_allocs.push_back({b, total});
        frames = b;
    }
    long pixels = 0;
    const CheckedLoad ld;
    for (int n = 0; n < N; ++n) {
        lf_plane pl[3];
        lf_surface_planes_of(S, frames, total, n, pl);
        for (int c0 = 0; c0 <= 5 && c0 < W; ++c0) {
            // window [c0, W) -- it ends at the row's end, the last group reaches up to three pixels beyond it -- or, for c0 = 5, [W - 5, W)
            const int start = c0 == 5 ? (W > 5 ? W - 5 : 0) : c0;
            const int ncols = W - start, ng = (ncols + 3) >> 2;
            std::vector<uint32_t> row((size_t)3 * ng);
            for (int y = top; y < top + ch; ++y) {
                for (int g = 0; g < ng; ++g) lf_surface_group<FMT>(ld, pl, y, start + 4 * g, cf, &row[3 * g]);
                const uint8_t* got = reinterpret_cast<const uint8_t*>(row.data());
                for (int x = 0; x < ncols; ++x) {
                    uint8_t want[3];
                    pixel(FMT, pl, y, start + x, cf, want);
                    if (memcmp(got + 3 * x, want, 3)) {
                        fprintf(stderr, "format %d layout %d %dx%d frame %d row %d column %d: staged %d %d %d, definition %d %d %d\n", FMT, layout, H, W,
                                n, y, start + x, got[3 * x], got[3 * x + 1], got[3 * x + 2], want[0], want[1], want[2]);
                        abort();
                    }
                    ++pixels;
                }
            }
        }
    }
    for (uint8_t* b : bufs) free(b);
    return pixels;
}

int main() {
    static const int geoms[][4] = {{98, 334, 33, 64}, {30, 50, 6, 24}, {8, 8, 0, 8}, {180, 320, 20, 160}};
    static const lf_yuv_coef presets[2] = {{65536, 0, 91881, 22554, 46802, 116130}, {76309, 16, 117489, 13975, 34925, 138438}};
    long pixels = 0;
    for (const auto& g : geoms)
        for (int layout = 1; layout <= 4; ++layout)
            for (const lf_yuv_coef& cf : presets) {
                pixels += run<LF_SURF_RGB>(g[0], g[1], g[2], g[3], layout, cf);
                pixels += run<LF_SURF_BGR>(g[0], g[1], g[2], g[3], layout, cf);
                pixels += run<LF_SURF_NV12>(g[0], g[1], g[2], g[3], layout, cf);
                pixels += run<LF_SURF_YUYV>(g[0], g[1], g[2], g[3], layout, cf);
                pixels += run<LF_SURF_I420>(g[0], g[1], g[2], g[3], layout, cf);
                pixels += run<LF_SURF_RGBX>(g[0], g[1], g[2], g[3], layout, cf);
                pixels += run<LF_SURF_BGRX>(g[0], g[1], g[2], g[3], layout, cf);
            }
    for (const auto& g : geoms)
        for (const lf_yuv_coef& cf : presets) pixels += run<LF_SURF_NV12>(g[0], g[1], g[2], g[3], 5, cf);
    CHECK(g_partial > 0);      // the end-of-buffer path was taken
    printf("surface staging: %ld pixels equal the definition, %ld loads inside their allocations (%ld of them cut at the end)\n", pixels, g_loads,
           g_partial);
    return 0;
}
