// Balanced age evaluation (imdb-wiki-dir/train.py:286-391 `validate` + `shot_metrics`) as ONE streaming pass per batch: per kept
// sample the five terms behind MSE / L1 / G-Mean / NUM, summed per integer label into a [num_labels + 1][5] float64 table (the last
// row collects every label that is no training label: fractional, negative, NaN, >= num_labels).  The reference keeps every
// prediction, copies them to the host and rescans the training labels once per distinct validation label; here nothing per sample
// is written and the host reads (num_labels + 1) * 5 numbers once per validation pass.
//
// Reduction, bit-reproducible (no float atomics anywhere); quad grid, wave-private tables and fold are those of dir_reduce_shared.h:
//   thread   one quad of the grid anchored at `label` per step, e = |pred - label| and e * e in float32 as the reference forms
//            them, ln e as log((double)e)
//   wave     labels are not spatially smooth (a shuffled validation set: ~64 distinct rows among 64 lanes), so there is no butterfly
//            per distinct row: the samples go to the wave's PRIVATE LDS table one after the other, in lane order; a row's slot is
//            only ever touched by the lane that owns it (row mod 64), which receives the sample's terms by readlane
//   block    the four wave tables added in wave order -> one [rows][5] float64 partial in the workspace
//   fold     a second launch adds the partials in block order onto the caller's table
// The zero-error count and NUM are counts: uint32 in LDS, exact in float64.
#include "dir_reduce_shared.h"
#include <math.h>

#define AGE_MAX_ROWS 256                      // LDS: 4 waves x rows x 32 B <= 32 KB
#define AGE_MAX_BLOCKS 1024
#define AGE_COLS 5

typedef DirSlot<3, 2> AgeSlot;                // one label row of a wave's LDS table: e*e, e, ln e (e > 0) and the counts e == 0, NUM
static_assert(AGE_COLS == 3 + 2, "table columns = the slot's sums and counts");

// (int)label for an integral label in [0, num_labels), the "other" row num_labels for everything else (NaN fails every comparison)
__device__ __forceinline__ int age_row(float l, int num_labels) {
    return (l >= 0.0f && l < (float)num_labels && l == truncf(l)) ? (int)l : num_labels;
}

// one value of lane `k` (uniform) to every lane
__device__ __forceinline__ float age_readlane(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ double age_readlane(double v, int k) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

__global__ void __launch_bounds__(DIR_TPB)
age_eval_kernel(const float* __restrict__ pred, const float* __restrict__ label, const uint8_t* __restrict__ valid,
                long long n, int off, int num_labels, bool pred_vec, bool valid_vec, double* __restrict__ partials) {
    extern __shared__ __align__(16) unsigned char age_smem[];
    AgeSlot* tabs = reinterpret_cast<AgeSlot*>(age_smem);                         // [4 waves][rows]
    const int rows = num_labels + 1;
    dir_slots_zero(tabs, rows);
    __syncthreads();
    const int lane = threadIdx.x & (DIR_WAVE - 1);
    AgeSlot* tab = tabs + (threadIdx.x / DIR_WAVE) * rows;

    const long long quads = (n + off + 3) / 4;
    const long long stride = (long long)gridDim.x * DIR_TPB;
    const long long rounds = (quads + stride - 1) / stride;                       // whole waves stay in the loop (ballot)
    for (long long it = 0; it < rounds; ++it) {
        const long long q = it * stride + (long long)blockIdx.x * DIR_TPB + threadIdx.x;
        const DirQuad<long long> d = dir_quad<long long>(q, quads, off, n);
        float l[4], p[4];
        bool in[4], keep[4];
        dir_quad_in(d, n, in);
        dir_quad_load(label, d, true, in, 0.0f, l);
        dir_quad_keep(valid, d, valid_vec, in, keep);
        dir_quad_load(pred, d, pred_vec, in, 0.0f, p);
        float e[4];
        double ln[4];
        int row[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                             // all lanes at once: the serial part below only moves numbers
            e[j] = fabsf(p[j] - l[j]);
            ln[j] = (keep[j] && e[j] > 0.0f) ? log((double)e[j]) : 0.0;
            row[j] = keep[j] ? age_row(l[j], num_labels) : -1;
        }
        // lane order: the samples of one lane after the other go to every lane (readlane), and the lane that OWNS the row (row mod 64)
        // adds them to its slot: every row's sum has one fixed order and no LDS address is shared between lanes
        unsigned long long todo = __ballot(keep[0] || keep[1] || keep[2] || keep[3]);
        while (todo) {
            const int k = __ffsll((long long)todo) - 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rk = __builtin_amdgcn_readlane(row[j], k);
                if (rk < 0) continue;                                             // uniform
                const float ek = age_readlane(e[j], k);
                const double lk = age_readlane(ln[j], k);
                if (lane == (rk & (DIR_WAVE - 1))) {
                    AgeSlot& s = tab[rk];
                    s.s[0] += (double)(ek * ek);
                    s.s[1] += (double)ek;
                    if (ek > 0.0f) s.s[2] += lk;
                    if (ek == 0.0f) s.c[0] += 1u;
                    s.c[1] += 1u;
                }
            }
            todo &= todo - 1;
        }
    }
    __syncthreads();
    dir_slots_write(tabs, rows, partials + (size_t)blockIdx.x * rows * AGE_COLS);
}

extern "C" size_t dir_age_eval_workspace(long long n, int num_labels) {
    if (n <= 0 || num_labels <= 0 || num_labels + 1 > AGE_MAX_ROWS) return 0;
    return (size_t)dir_quad_grid(n, AGE_MAX_BLOCKS) * (num_labels + 1) * AGE_COLS * sizeof(double);
}

extern "C" int dir_age_eval_accumulate(const float* pred, const float* label, const uint8_t* valid, long long n, int num_labels,
                                       double* table, void* workspace, size_t workspace_bytes, dir_stream_t stream) {
    DIR_RETURN_IF(n < 0 || num_labels <= 0, DIR_EINVAL);
    DIR_RETURN_IF(num_labels + 1 > AGE_MAX_ROWS, DIR_EUNSUPPORTED);
    if (n == 0) return DIR_OK;
    DIR_RETURN_IF(!pred || !label || !table || !workspace, DIR_EINVAL);
    DIR_RETURN_IF(dir_misaligned(pred, 4) || dir_misaligned(label, 4) || dir_misaligned(table, 8) || dir_misaligned(workspace, 8), DIR_EINVAL);
    DIR_RETURN_IF(workspace_bytes < dir_age_eval_workspace(n, num_labels), DIR_EWORKSPACE);
    const int grid = dir_quad_grid(n, AGE_MAX_BLOCKS);
    const int off = dir_quad_offset(label);
    const bool pred_vec = dir_quad_same_offset(pred, off), valid_vec = dir_quad_mask_aligned(valid, off);
    const int rows = num_labels + 1;
    const size_t lds = (size_t)4 * rows * sizeof(AgeSlot);
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(age_eval_kernel, dim3(grid), dim3(DIR_TPB), lds, dir_s(stream), pred, label, valid, n, off, num_labels,
                       pred_vec, valid_vec, partials);
    DIR_LAUNCH_CHECK();
    return dir_table_fold(partials, grid, rows * AGE_COLS, table, stream);
}
