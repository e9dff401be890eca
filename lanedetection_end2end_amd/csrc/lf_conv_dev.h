// Device helpers and launch state shared by the convolution kernel files lf_conv.hip (tap-GEMM forward / data gradient) and
// lf_wgrad.hip (weight gradients): the vector types, buffer-addressed loads and stores, the DPP row sums, the tile constants, the
// per-(device, kernel) LDS attribute and the dynamic-LDS symbol.  Internal: included by those two files only, everything in an
// anonymous namespace.  (lf_wgrad_ro.hip and lf_stem.hip keep private copies of zero4 and the typedefs.)
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

// (This header's anonymous namespace gives each including file ONE COPY OF ITS OWN of the mutex and of allow_big_lds' map.  That is
// correct because the map is keyed by kernel address and no kernel belongs to two files; the occupancy cache meant by "below" is
// resident_workgroups in lf_conv.hip, which locks that file's copy.)
// Per-(device, kernel) launch state shared by the host threads of a process (one process may drive several GPUs): the occupancy
// cache below and the "dynamic LDS beyond 64 KB allowed" attribute of the LDS-ring kernels.
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

extern __shared__ __attribute__((aligned(16))) unsigned char lf_tap_lds[];      // tap tables of tapgemm_kernel

}  // namespace
