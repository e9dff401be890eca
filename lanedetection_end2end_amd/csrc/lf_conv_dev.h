// Device helpers and launch state shared by the convolution kernel files lf_conv.hip and lf_conv_bf16.hip (tap-GEMM forward / data
// gradient on fp32 and on bf16 tensors), lf_conv_pair.hip (the fused 3x1 -> 1x3 forward pairs), lf_wgrad.hip (weight gradients) and
// lf_bwd16.hip (both gradients of the 16-channel layers): the vector types, buffer-addressed loads and stores,
// the DPP row sums, the tile constants, the per-(device, kernel) LDS attribute and occupancy cache with the launch that uses them,
// the epilogue-set dispatchers and the dynamic-LDS symbol.  Internal: included by those five files (and by lf_conv_stream.h, the
// stream tile body of the first and the third) only, everything in an anonymous namespace.  (lf_wgrad_ro.hip and lf_stem.hip keep private copies of zero4 and the typedefs.)
#pragma once
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <utility>

#include <hip/hip_ext.h>

#include "lf_conv.h"
#include "lf_ldsdma.h"
#include "lf_types.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int MT = 4;                 // 16-pixel tiles per wave
constexpr int WG_WAVES = 4;
constexpr int PIX_PER_WG = WG_WAVES * MT * 16;

__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// Buffer-addressed 16-byte load: SGPR resource + 32-bit VGPR byte offset + scalar byte offset.  Beside a dense MFMA stream a
// global_load whose 64-bit VGPR address was just computed costs the SIMD ~200 ns of matrix issue, this form ~6 ns
// (tools/vmem_cost.hip, profiles/r2_vmem_cost.txt); an offset >= num_records reads as 0.0f (the conv's zero padding).
typedef unsigned u32x4v __attribute__((vector_size(16)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
__device__ __forceinline__ f32x4 ldb4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
// (LF_OOB, the byte offset beyond every tensor the launcher admits, lives in lf_ldsdma.h)
__device__ __forceinline__ f32x4 zero4() { f32x4 z = {0.f, 0.f, 0.f, 0.f}; return z; }
// ReLU as a signed-integer maximum of the bit patterns (negative floats are negative integers): ONE v_max_i32 per element;
// fmaxf compiles to a canonicalising v_max_f32 v, v, v followed by the v_max_f32 with 0 -- twice the VALU work in the BN+ReLU
// operand prologue, where every VALU instruction issues beside the partner wave's MFMA stream
typedef int i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 max0(f32x4 v) {
    i32x4 b = __builtin_bit_cast(i32x4, v);
    b.x = b.x > 0 ? b.x : 0; b.y = b.y > 0 ? b.y : 0; b.z = b.z > 0 ? b.z : 0; b.w = b.w > 0 ? b.w : 0;
    return __builtin_bit_cast(f32x4, b);
}
// ReLU of LF_TAPGEMM_EPILOGUE on bf16 tensors (the streaming, ring and lean bf16 kernels), where a NaN stays a NaN: the matrix
// cores return NaN with its sign bit set (0 * Inf, Inf - Inf), which max0 stores as 0 -- so a non-finite value in a window showed
// in the output without ReLU and vanished with it (tests/test_bf16_stride2_kernels_gpu.py plants them).  v <= 0 is false for a
// NaN (v_cmp + v_cndmask, two VALU instructions per element); on every other input the result has max0's bits (-0 and -Inf
// included).  NOT changed, and not tested with non-finite values: the whole-line and wave-private bf16 kernels' own epilogues,
// the fp32 kernels and every BN+ReLU operand prologue keep max0 and store 0 for a sign-set NaN.
__device__ __forceinline__ f32x4 relu_keep_nan(f32x4 v) {
    v.x = v.x <= 0.f ? 0.f : v.x; v.y = v.y <= 0.f ? 0.f : v.y; v.z = v.z <= 0.f ? 0.f : v.z; v.w = v.w <= 0.f ? 0.f : v.w;
    return v;
}
__device__ __forceinline__ f32x4 keep_pos(f32x4 v, f32x4 m) {
    v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f; v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
    return v;
}
// storage-typed access of the epilogue operands / result (S16: the tensors hold bf16 elements, see lf_types.h)
// (buffer-addressed like the operand loads: the epilogue of one wave runs beside its partner's MFMA stream, where 64-bit
// address arithmetic and VGPR-pair addressed memory instructions are what made it take 9 us instead of 4)
typedef unsigned u32x2v __attribute__((vector_size(8)));
template <bool S16>
__device__ __forceinline__ f32x4 epi_ld(__amdgpu_buffer_rsrc_t r, unsigned off, unsigned soff = 0u) {   // element offsets
    if constexpr (S16) {
        const u32x2v q = __builtin_amdgcn_raw_buffer_load_b64(r, (int)(off * 2u), (int)(soff * 2u), 0);
        f32x4 v;
        v.x = __uint_as_float(q[0] << 16); v.y = __uint_as_float(q[0] & 0xffff0000u);
        v.z = __uint_as_float(q[1] << 16); v.w = __uint_as_float(q[1] & 0xffff0000u);
        return v;
    } else return ldb4(r, off * 4u, soff * 4u);
}
template <bool S16>
__device__ __forceinline__ void epi_st(__amdgpu_buffer_rsrc_t r, unsigned off, f32x4 v) {
    if constexpr (S16) {
        lf_bf16x4 b;
        b[0] = (lf_bf16)v.x; b[1] = (lf_bf16)v.y; b[2] = (lf_bf16)v.z; b[3] = (lf_bf16)v.w;
        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2v, b), r, (int)(off * 2u), 0, 0);
    } else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4v, v), r, (int)(off * 4u), 0, 0);   // (nt and sc0 sc1 hints measured: both -1.2 %)
}
__device__ __forceinline__ f32x4 round_bf16(f32x4 v) {
    v.x = (float)(lf_bf16)v.x; v.y = (float)(lf_bf16)v.y; v.z = (float)(lf_bf16)v.z; v.w = (float)(lf_bf16)v.w;
    return v;
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// one pair of fp32 values -> their packed bf16 roundings (v_cvt_pk_bf16_f32); v becomes the exact residuals
__device__ __forceinline__ unsigned split_pair(f32x2& v) {
    const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    v.x -= __uint_as_float(u << 16);             // exact: the residual of a round-to-nearest fits fp32
    v.y -= __uint_as_float(u & 0xffff0000u);
    return u;
}
// sum over the 16 lanes that share l>>4 (one DPP row): lane pairs, quads (quad_perm), then the four quad totals by row
// rotations of 4 and 8 -- every lane ends with the row total (associated differently per quad; the caller reads lane 0 of the
// row).  DPP adds need neither the lane id nor the LDS crossbar that __shfl_xor (ds_bpermute) goes through.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
// lane 0 of every 16-lane DPP row broadcast to its row (row_share:0 / row_newbcast:0)
__device__ __forceinline__ f32x4 bcast16(f32x4 v) {
    f32x4 r;
    r.x = dpp_mov<0x150>(v.x); r.y = dpp_mov<0x150>(v.y); r.z = dpp_mov<0x150>(v.z); r.w = dpp_mov<0x150>(v.w);
    return r;
}
__device__ __forceinline__ float sum16(float v) {
    v += dpp_mov<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_mov<0x124>(v);     // row_ror:4
    v += dpp_mov<0x128>(v);     // row_ror:8
    return v;
}

// Index arithmetic the tap-GEMM kernels share.  Each is used only where the kernel's instruction text stays what the inline
// form gave (tools/kernel_asm_diff.py); the kernels it would have changed keep their own lines: tapgemm_kernel, tapgemm_lean_kernel,
// tapgemm_bf16_ring_kernel, tappair128_kernel.  Scalar inputs are taken by const reference on purpose: by value, the callee is
// simplified before it is inlined and most callers' register allocation moves.  (The clamped source-offset block -- sy, sx, in,
// syc, sxc, offset -- has no helper: as a function it changed every kernel it was tried in.)
// Workgroup b runs on XCD b % 8 (observed dispatch order): the block index remapped so that every XCD owns a CONTIGUOUS range of
// tiles -- the halo rows neighbouring tiles share meet in one L2
__device__ __forceinline__ unsigned xcd_swizzle(const unsigned& b) {
    unsigned bx = b;
    if ((gridDim.x & 7u) == 0) bx = (bx & 7u) * (gridDim.x >> 3) + (bx >> 3);
    return bx;
}
// ... and for a workgroup that walks several units (first, first + stride, ... < end): the walk stays inside its XCD's range
struct XcdRange { unsigned first, stride, end; };
__device__ __forceinline__ XcdRange xcd_range(const unsigned& nunits) {
    XcdRange r = {blockIdx.x, gridDim.x, nunits};
    if ((gridDim.x & 7u) == 0 && (nunits & 7u) == 0) {
        const unsigned per = nunits >> 3;
        r.first = (blockIdx.x & 7u) * per + (blockIdx.x >> 3); r.stride = gridDim.x >> 3; r.end = (blockIdx.x & 7u) * per + per;
    }
    return r;
}
// (image, row, first column) of a wave whose 64 pixels from logical pixel q on lie in one image row (Wl % 64 == 0, q wave-uniform):
// two divisions, the results in scalar registers
__device__ __forceinline__ void row1_coords(const LfTapGeom& g, const unsigned& q, int& n0, int& i0, int& j0) {
    const unsigned r = q / (unsigned)g.Wl;
    j0 = __builtin_amdgcn_readfirstlane((int)(q - r * (unsigned)g.Wl));
    n0 = __builtin_amdgcn_readfirstlane((int)(r / (unsigned)g.Hl));
    i0 = __builtin_amdgcn_readfirstlane((int)r) - n0 * g.Hl;
}

// Per-(device, kernel) launch state shared by the host threads of a process (one process may drive several GPUs): the "dynamic
// LDS beyond 64 KB allowed" attribute of the LDS-ring kernels (allow_big_lds) and the occupancy cache (resident_workgroups), both
// below.  This header's anonymous namespace gives each including file ONE COPY OF ITS OWN of the mutex and of both maps.  That is
// correct because every map is keyed by kernel address and no kernel belongs to two files: a file's copies hold exactly the
// entries of that file's kernels, and each is only ever locked with that file's mutex.
std::mutex g_launch_state_mutex;
int current_device() {
    int dev = 0;
    return hipGetDevice(&dev) == hipSuccess ? dev : -1;
}
// hipFuncAttributeMaxDynamicSharedMemorySize once per (device, kernel); false when the runtime refuses (the caller launches a
// kernel that needs less LDS instead of failing at launch)
bool allow_big_lds(const void* kernel, int bytes) {
    static std::map<std::pair<int, const void*>, bool> done;
    const std::pair<int, const void*> key(current_device(), kernel);
    std::lock_guard<std::mutex> lock(g_launch_state_mutex);
    auto it = done.find(key);
    if (it != done.end()) return it->second;
    return done[key] = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
}
// Workgroups of `kernel` the whole chip holds at once (occupancy x CUs), cached per (device, kernel, dynamic LDS bytes).
template <typename K>
int resident_workgroups(K kernel, size_t lds, int block = 256) {
    static std::map<std::tuple<int, const void*, size_t>, int> cache;
    const int dev = current_device();
    const std::tuple<int, const void*, size_t> key(dev, reinterpret_cast<const void*>(kernel), lds);
    std::lock_guard<std::mutex> lock(g_launch_state_mutex);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int cus = 0, nb = 0;
    if (dev < 0 || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, lds) != hipSuccess || nb < 1 || cus < 1)
        return cache[key] = 1 << 30;                 // unknown: one tile per workgroup
    return cache[key] = nb * cus;
}
// The launch of every kernel that walks its tiles / items with stride gridDim.x: no more workgroups than are resident at once (a
// multiple of 8 per XCD dealing: XCD-contiguous item ranges), so that the work beyond the first round is spread one per CU by
// construction; then no more than max_wgs, where that is > 0.
// lds_attr > 0: the kernel needs that hipFuncAttributeMaxDynamicSharedMemorySize -- false when the runtime refuses it on this device
// (nothing launched: the caller takes a kernel that needs less LDS).  flags: g_launch_flags (lf_conv.hip) where the kernel honours it, else 0.
template <typename K, typename... Args>
bool launch_resident(K kernel, dim3 grid, unsigned block, size_t lds, int lds_attr, unsigned max_wgs, unsigned flags, hipStream_t st, const Args&... args) {
    if (lds_attr > 0 && !allow_big_lds(reinterpret_cast<const void*>(kernel), lds_attr)) return false;
    const unsigned res = (unsigned)resident_workgroups(kernel, lds, (int)block) / grid.y;
    if (grid.x > res && res >= 8) grid.x = res & ~7u;
    if (max_wgs > 0 && grid.x > max_wgs) grid.x = max_wgs;
    if (flags) hipExtLaunchKernelGGL(kernel, grid, dim3(block), (unsigned)lds, st, nullptr, nullptr, flags, args...);
    else hipLaunchKernelGGL(kernel, grid, dim3(block), lds, st, args...);
    return true;
}
constexpr int BIG_LDS = 160 * 1024 - 4096;      // the LDS attribute of the whole-line, wave-private and weight-resident kernels
// The compiled-in data-gradient epilogues (mask / residual / BN-backward sums) carry no bias vector (NOBIAS): a launch that
// combines one of them with a bias takes the run-time-flag kernel -- except the inference engine's residual tail (bias + ADD +
// ReLU: BRES, compiled into the kernels the forward convolutions route to; the split, ring and streaming-fast kernels keep the
// run-time form)
constexpr int BRES = LF_EPI_ADD | LF_EPI_RELU | LF_EPI_BIAS;
template <int V> using IntC = std::integral_constant<int, V>;
// The one place that turns the run-time epilogue set into a template argument: f(IntC<E>{}) with E the compiled-in set equal to
// epis, or -1 (the run-time-flag form) for every other.  WITH_BRES = false: the kernel family has no compiled-in BRES form.
template <bool WITH_BRES, typename F>
auto with_epi(int epis, F&& f) {
    switch (epis) {
        case 0: return f(IntC<0>{});
        case LF_EPI_RELU: return f(IntC<LF_EPI_RELU>{});
        case LF_EPI_MASK: return f(IntC<LF_EPI_MASK>{});
        case LF_EPI_ADD: return f(IntC<LF_EPI_ADD>{});
        case LF_EPI_STATS_SQ: return f(IntC<LF_EPI_STATS_SQ>{});
        case LF_EPI_MASK | LF_EPI_STATS_XHAT: return f(IntC<LF_EPI_MASK | LF_EPI_STATS_XHAT>{});
        case LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT: return f(IntC<LF_EPI_ADD | LF_EPI_MASK | LF_EPI_STATS_XHAT>{});
        case LF_EPI_MASKBN | LF_EPI_STATS_XHAT: return f(IntC<LF_EPI_MASKBN | LF_EPI_STATS_XHAT>{});
        case BRES: return f(IntC<WITH_BRES ? BRES : -1>{});
        default: return f(IntC<-1>{});
    }
}
// ... and for the kernels that compile the BN+ReLU operand prologue beside the epilogue, f(IntC<PRO>{}, IntC<E>{}): a prologue launch
// has the compiled-in ReLU epilogue or the run-time flags, only prologue-free launches dispatch on epis
template <bool WITH_BRES, typename F>
void with_pro_epi(int pro, int epi, int epis, F&& f) {
    if (pro == LF_PRO_BNRELU && epi == LF_EPI_RELU) f(IntC<1>{}, IntC<LF_EPI_RELU>{});
    else if (pro == LF_PRO_BNRELU) f(IntC<1>{}, IntC<-1>{});
    else with_epi<WITH_BRES>(epis, [&](auto e) { f(IntC<0>{}, e); });
}

extern __shared__ __attribute__((aligned(16))) unsigned char lf_tap_lds[];      // tap tables of tapgemm_kernel

}  // namespace
