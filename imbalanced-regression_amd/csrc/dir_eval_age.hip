// Balanced age evaluation (imdb-wiki-dir/train.py:286-391 `validate` + `shot_metrics`) as ONE streaming pass per batch: per kept
// sample the five terms behind MSE / L1 / G-Mean / NUM, summed per integer label into a [num_labels + 1][5] float64 table (the last
// row collects every label that is no training label: fractional, negative, NaN, >= num_labels).  The reference keeps every
// prediction, copies them to the host and rescans the training labels once per distinct validation label; here nothing per sample
// is written and the host reads (num_labels + 1) * 5 numbers once per validation pass.
//
// Reduction, bit-reproducible (no float atomics anywhere), the scheme of dir_eval.hip:
//   thread   one aligned 16-byte quad of `label` per step (edge quads element-wise), e = |pred - label| and e * e in float32 as the
//            reference forms them, ln e as log((double)e)
//   wave     labels are not spatially smooth (a shuffled validation set: ~64 distinct rows among 64 lanes), so there is no butterfly
//            per distinct row: the samples go to the wave's PRIVATE LDS table one after the other, in lane order; a row's slot is
//            only ever touched by the lane that owns it (row mod 64), which receives the sample's terms by readlane
//   block    the four wave tables added in wave order -> one [rows][5] float64 partial in the workspace
//   fold     a second launch adds the partials in block order onto the caller's table
// The zero-error count and NUM are counts: uint32 in LDS, exact in float64.
#include "dir_common.h"
#include <math.h>

#define AGE_MAX_ROWS 256                      // LDS: 4 waves x rows x 32 B <= 32 KB
#define AGE_MAX_BLOCKS 1024
#define AGE_COLS 5

struct AgeSlot {                              // one label row of a wave's LDS table
    double s[3];                              // e*e, e, ln e (e > 0)
    uint32_t c[2];                            // e == 0, NUM
};

static int age_grid(long long n) {
    const long long quads = (n + 3 + 3) / 4;  // the quad grid is anchored at the 16-byte boundary below `label`: up to 3 slots of lead-in
    long long g = (quads + DIR_TPB - 1) / DIR_TPB;
    if (g > AGE_MAX_BLOCKS) g = AGE_MAX_BLOCKS;
    return g < 1 ? 1 : (int)g;
}

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
    for (int i = threadIdx.x; i < 4 * rows * (int)(sizeof(AgeSlot) / 4); i += DIR_TPB) reinterpret_cast<uint32_t*>(age_smem)[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & (DIR_WAVE - 1);
    AgeSlot* tab = tabs + (threadIdx.x / DIR_WAVE) * rows;

    const long long quads = (n + off + 3) / 4;
    const long long stride = (long long)gridDim.x * DIR_TPB;
    const long long rounds = (quads + stride - 1) / stride;                       // whole waves stay in the loop (ballot)
    for (long long it = 0; it < rounds; ++it) {
        const long long q = it * stride + (long long)blockIdx.x * DIR_TPB + threadIdx.x;
        const long long i0 = 4 * q - off;                                         // may be < 0 (lead-in) or reach past n (tail)
        float l[4], p[4];
        bool keep[4];
        const bool inside = q < quads;
        const bool full = inside && i0 >= 0 && i0 + 3 < n;
        if (full) {
            const float4 lv = *reinterpret_cast<const float4*>(label + i0);       // 16-byte aligned by construction of the quad grid
            l[0] = lv.x; l[1] = lv.y; l[2] = lv.z; l[3] = lv.w;
            if (valid) {
                if (valid_vec) {
                    const uint32_t mv = *reinterpret_cast<const uint32_t*>(valid + i0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) keep[j] = ((mv >> (8 * j)) & 0xffu) != 0;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) keep[j] = valid[i0 + j] != 0;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) keep[j] = true;
            }
            if (pred_vec) {
                const float4 pv = *reinterpret_cast<const float4*>(pred + i0);
                p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) p[j] = pred[i0 + j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long i = i0 + j;
                const bool in = inside && i >= 0 && i < n;
                keep[j] = in && (!valid || valid[i] != 0);
                l[j] = in ? label[i] : 0.0f;
                p[j] = in ? pred[i] : 0.0f;
            }
        }
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
    double* out = partials + (size_t)blockIdx.x * rows * AGE_COLS;
    for (int i = threadIdx.x; i < rows * AGE_COLS; i += DIR_TPB) {
        const int r = i / AGE_COLS, col = i - r * AGE_COLS;
        double v = 0.0;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {                                          // wave order
            const AgeSlot& s = tabs[wv * rows + r];
            v += col < 3 ? s.s[col] : (double)s.c[col - 3];
        }
        out[i] = v;
    }
}

__global__ void __launch_bounds__(DIR_TPB)
age_eval_fold_kernel(const double* __restrict__ partials, int blocks, int entries, double* __restrict__ table) {
    const int i = blockIdx.x * DIR_TPB + threadIdx.x;
    if (i >= entries) return;
    double v = 0.0;
#pragma unroll 8
    for (int g = 0; g < blocks; ++g) v += partials[(size_t)g * entries + i];       // block order
    table[i] += v;
}

extern "C" size_t dir_age_eval_workspace(long long n, int num_labels) {
    if (n <= 0 || num_labels <= 0 || num_labels + 1 > AGE_MAX_ROWS) return 0;
    return (size_t)age_grid(n) * (num_labels + 1) * AGE_COLS * sizeof(double);
}

extern "C" int dir_age_eval_accumulate(const float* pred, const float* label, const uint8_t* valid, long long n, int num_labels,
                                       double* table, void* workspace, size_t workspace_bytes, dir_stream_t stream) {
    DIR_RETURN_IF(n < 0 || num_labels <= 0, DIR_EINVAL);
    DIR_RETURN_IF(num_labels + 1 > AGE_MAX_ROWS, DIR_EUNSUPPORTED);
    if (n == 0) return DIR_OK;
    DIR_RETURN_IF(!pred || !label || !table || !workspace, DIR_EINVAL);
    DIR_RETURN_IF((reinterpret_cast<uintptr_t>(pred) & 3u) || (reinterpret_cast<uintptr_t>(label) & 3u) ||
                  (reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(workspace) & 7u), DIR_EINVAL);
    DIR_RETURN_IF(workspace_bytes < dir_age_eval_workspace(n, num_labels), DIR_EWORKSPACE);
    const int grid = age_grid(n);
    const int off = (int)((reinterpret_cast<uintptr_t>(label) >> 2) & 3u);        // elements between the 16-byte boundary below and label[0]
    const bool pred_vec = ((reinterpret_cast<uintptr_t>(pred) >> 2) & 3u) == (unsigned)off;
    const bool valid_vec = valid && ((reinterpret_cast<uintptr_t>(valid) - (uintptr_t)off) & 3u) == 0;
    const int rows = num_labels + 1;
    const size_t lds = (size_t)4 * rows * sizeof(AgeSlot);
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(age_eval_kernel, dim3(grid), dim3(DIR_TPB), lds, dir_s(stream), pred, label, valid, n, off, num_labels,
                       pred_vec, valid_vec, partials);
    DIR_LAUNCH_CHECK();
    const int entries = rows * AGE_COLS;
    hipLaunchKernelGGL(age_eval_fold_kernel, dim3(dir_cdiv(entries, DIR_TPB)), dim3(DIR_TPB), 0, dir_s(stream), partials, grid, entries, table);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}
