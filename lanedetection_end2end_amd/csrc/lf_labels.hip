// The label half of LaneDataset.__getitem__ for a whole batch in one launch (the pixel half is lf_pipeline.hip):
// the parsed label tables of a RESIDENT dataset stay in HBM, a batch is the rows sel[n] of them, flipped where flip[n] says so --
// no per-sample host loop and no host -> device copy of label data per step.
//   lf_label_batch_bp  : BP/Dataloader/Load_Data_new.py:133-197
//   lf_label_batch_bev : BEV/Dataloader/Load_Data_new.py:74,86-111
// Everything here is exact or ONE correctly rounded fp64 operation (x / 2.5, h / 2.5, ... - 32, (2R - 1) - x, 1 + (-c)): no
// product feeds a sum, so nothing can be contracted into an fma and the results are bit-equal to numpy's.
// One block of four waves per sample: wave = lane row, lane of the wave = column (56 of 64 in use); at most 4 x 56 elements per
// sample, so there is nothing to tune.
#include "lf_common.h"

#define LB_LANES 4
#define LB_POINTS 56        // BP :99 self.num_points
#define LB_LINES 10         // length of a label_new.json "lines" list
#define LB_THREADS 256

namespace {

struct Row {
    long row;
    bool flip;
};

// sel[n] -> table row and the effective flip.  An index outside the pool is COUNTED for the host (IndexError, one call late) and
// row 0 is read in its place, as lf_pipeline_*_indexed do.  Flip: `if idx not in self.valid_idx and hflip_input` (BP :168, BEV :88).
__device__ __forceinline__ Row select_row(const int64_t* __restrict__ sel, const uint8_t* __restrict__ flip,
                                          const uint8_t* __restrict__ is_valid, long M, int n, int* __restrict__ bad) {
    Row r;
    r.row = sel[n];
    if (r.row < 0 || r.row >= M) {
        if (bad && threadIdx.x == 0) atomicAdd(bad, 1);
        r.row = 0;
    }
    r.flip = flip && flip[n] && !is_valid[r.row];
    return r;
}

// mirror_list (BP :200-207, BEV :120-127) of a 10-entry list is the list reversed; [3:7] of it is entries 6, 5, 4, 3.
__device__ __forceinline__ int line_entry(const int8_t* __restrict__ lines, long row, bool flip, int k) {
    return lines[row * LB_LINES + (flip ? 6 - k : 3 + k)];
}

__global__ __launch_bounds__(LB_THREADS) void label_batch_bp_kernel(
    const int32_t* __restrict__ lanes, const double* __restrict__ h_samples, const int32_t* __restrict__ h_count,
    const int8_t* __restrict__ lines, const int64_t* __restrict__ file_idx, const uint8_t* __restrict__ is_valid,
    const int32_t* __restrict__ valid_pos, long M, const int64_t* __restrict__ sel, const uint8_t* __restrict__ flip, int resize,
    double* __restrict__ valid_points, double* __restrict__ lanes_out, float* __restrict__ horizon, float* __restrict__ gt_line,
    int64_t* __restrict__ idx, int64_t* __restrict__ index, uint8_t* __restrict__ flipped, int* __restrict__ bad) {
    __shared__ double s_min[LB_LANES];
    const int n = blockIdx.x, l = threadIdx.x >> 6, c = threadIdx.x & 63;
    const Row r = select_row(sel, flip, is_valid, M, n, bad);
    int count = h_count[r.row];
    count = count < 0 ? 0 : (count > LB_POINTS ? LB_POINTS : count);
    double y = (double)resize;                                   // :152 `or [self.resize]`
    if (c < LB_POINTS) {
        const size_t o = ((size_t)n * LB_LANES + l) * LB_POINTS + c;
        // own lane row l, unflipped: valid_points (:140-141, never permuted) and the horizon candidate
        const int x = lanes[((size_t)r.row * LB_LANES + l) * LB_POINTS + c];
        valid_points[o] = (x > 0 && c >= 8) ? 1.0 : 0.0;
        double v = (double)x / 2.5;                              // :144
        if (v < 0.0) v = -2.0;                                   // :145,147
        // :146,152 zip(lane, h_samples): column i of the PADDED lane pairs with height i of the label's own list
        if (c < count && v != -2.0) y = h_samples[(size_t)r.row * LB_POINTS + c] / 2.5 - 32.0;
        // output row l: the flip takes rows [1, 0, 3, 2] (:176-178)
        if (r.flip) {
            const int xs = lanes[((size_t)r.row * LB_LANES + (l ^ 1)) * LB_POINTS + c];
            const double vs = (double)xs / 2.5;
            v = vs < 0.0 ? -2.0 : (double)(2 * resize - 1) - vs;
        }
        lanes_out[o] = v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) y = fmin(y, __shfl_xor(y, o, 64));
    if (c == 0) s_min[l] = y;
    __syncthreads();
    const double y_val = fmin(fmin(s_min[0], s_min[1]), fmin(s_min[2], s_min[3]));      // :153
    // :154-155 horizon[0:int(np.floor(y_val))] = 1 -- Python's slice: a negative stop counts from the end, both ends clamp
    const double f = floor(y_val);
    long stop = f >= (double)resize ? resize : (f <= -(double)resize ? -(long)resize : (long)f);
    if (stop < 0) stop += resize;
    for (int j = threadIdx.x; j < resize; j += LB_THREADS) horizon[(size_t)n * resize + j] = j < stop ? 1.f : 0.f;
    if (threadIdx.x < 4) {                                       // :187-188 clamp(lines[3:7] + 1, 0, 1).float()
        const int v = line_entry(lines, r.row, r.flip, threadIdx.x) + 1;
        gt_line[(size_t)n * 4 + threadIdx.x] = v < 0 ? 0.f : (v > 1 ? 1.f : (float)v);
    }
    if (threadIdx.x == 64) {
        idx[n] = file_idx[r.row];                                // :122
        index[n] = valid_pos[r.row];                             // :195
        flipped[n] = r.flip ? 1 : 0;
    }
}

__global__ __launch_bounds__(64) void label_batch_bev_kernel(
    const double* __restrict__ params, const int8_t* __restrict__ lines, const int64_t* __restrict__ file_idx,
    const uint8_t* __restrict__ is_valid, const int32_t* __restrict__ valid_pos, long M, const int64_t* __restrict__ sel,
    const uint8_t* __restrict__ flip, float* __restrict__ params_out, int64_t* __restrict__ gt_line, int64_t* __restrict__ idx,
    int64_t* __restrict__ index, uint8_t* __restrict__ flipped, int* __restrict__ bad) {
    const int n = blockIdx.x, t = threadIdx.x;
    const Row r = select_row(sel, flip, is_valid, M, n, bad);
    if (t < 12) {
        const int l = t / 3, k = t - l * 3;
        double v;
        if (r.flip) {                                            // :96-99 rows [1, 0, 3, 2], negated, 1 + the last coefficient
            v = -params[((size_t)r.row * 4 + (l ^ 1)) * 3 + k];  // (an absent lane becomes (-0, -0, 1), as in the reference)
            if (k == 2) v = 1.0 + v;
        } else {
            v = params[((size_t)r.row * 4 + l) * 3 + k];
        }
        params_out[(size_t)n * 12 + t] = (float)v;               // :103
    } else if (t < 16) {
        gt_line[(size_t)n * 4 + (t - 12)] = line_entry(lines, r.row, r.flip, t - 12) + 1;      // :109-111
    } else if (t == 16) {
        idx[n] = file_idx[r.row];                                // :73
        index[n] = valid_pos[r.row];                             // :115
        flipped[n] = r.flip ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int lf_label_batch_bp(const int32_t* lanes, const double* h_samples, const int32_t* h_count, const int8_t* lines,
                      const int64_t* file_idx, const uint8_t* is_valid, const int32_t* valid_pos, long M, const int64_t* sel,
                      const uint8_t* flip, int N, int resize, double* valid_points, double* lanes_out, float* horizon,
                      float* gt_line, int64_t* idx, int64_t* index, uint8_t* flipped, int* bad, void* stream) {
    LF_REQUIRE(lanes && h_samples && h_count && lines && file_idx && is_valid && valid_pos && sel && valid_points && lanes_out &&
                   horizon && gt_line && idx && index && flipped,
               "lf_label_batch_bp: null pointer");
    LF_REQUIRE(M > 0 && N > 0 && resize > 0 && resize <= (1 << 20), "lf_label_batch_bp: bad sizes M=%ld N=%d resize=%d", M, N, resize);
    hipLaunchKernelGGL(label_batch_bp_kernel, dim3(N), dim3(LB_THREADS), 0, (hipStream_t)stream, lanes, h_samples, h_count, lines,
                       file_idx, is_valid, valid_pos, M, sel, flip, resize, valid_points, lanes_out, horizon, gt_line, idx, index,
                       flipped, bad);
    LF_CHECK_LAUNCH("lf_label_batch_bp");
    return 0;
}

int lf_label_batch_bev(const double* params, const int8_t* lines, const int64_t* file_idx, const uint8_t* is_valid,
                       const int32_t* valid_pos, long M, const int64_t* sel, const uint8_t* flip, int N, float* params_out,
                       int64_t* gt_line, int64_t* idx, int64_t* index, uint8_t* flipped, int* bad, void* stream) {
    LF_REQUIRE(params && lines && file_idx && is_valid && valid_pos && sel && params_out && gt_line && idx && index && flipped,
               "lf_label_batch_bev: null pointer");
    LF_REQUIRE(M > 0 && N > 0, "lf_label_batch_bev: bad sizes M=%ld N=%d", M, N);
    hipLaunchKernelGGL(label_batch_bev_kernel, dim3(N), dim3(64), 0, (hipStream_t)stream, params, lines, file_idx, is_valid, valid_pos,
                       M, sel, flip, params_out, gt_line, idx, index, flipped, bad);
    LF_CHECK_LAUNCH("lf_label_batch_bev");
    return 0;
}

}  // extern "C"
