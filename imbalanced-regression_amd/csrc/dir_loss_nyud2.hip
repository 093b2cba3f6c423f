// NYUD2-DIR training loss (nyud2-dir/train.py:200, `loss = torch.mean(((output - depth) ** 2) * weight)`) with the per-pixel LDS weight
// of nyud2-dir/loaddata.py:57-69 (`bucket_weights[min(int(d * 10), 99)]`) looked up in the same pass: value and gradient in ONE
// streaming launch plus a one-workgroup fold.  The reference builds the weight map on the host with a Python `map` over every pixel;
// here the bucket table sits in LDS and the weight map is never written.
//
// Per pixel, float32, one rounding per operation (-ffp-contract=off):
//   b  = clamp(int(depth * mult), 0, bucket_num - 1)        float32 product, truncated: dir_scaled_bucket of dir_common.h from 0
//   w  = table[b]   (1 when there is no table, and 1 for a NaN depth)
//   d  = pred - depth;   t = (d * d) * w;   dx = ((1 / n) * w) * (2 * d)      torch's autograd order: mean, mul, pow backward
// A negative depth goes to bucket 0 (as PixelWeights does); the reference's Python list would wrap a negative index.  NaN propagates.
//
// Reduction, bit-reproducible (no float atomics anywhere):
//   thread   float64 running sum over its pixels in index order (one quad of the grid anchored at `depth` per step, dir_reduce_shared.h)
//   wave     64-lane butterfly in float64
//   block    the four wave sums added in wave order -> one float64 partial in the workspace
//   fold     a second launch of one workgroup adds the partials in workgroup order, divides by n in float64, rounds to float32
#include "dir_reduce_shared.h"

#define DLOSS_MAX_BUCKETS 256                 // LDS: one float per bucket
#define DLOSS_MAX_BLOCKS 256                  // one per CU; bounds the partial buffer (2 KB) and the serial fold

// one pixel: the term (d * d) * w and the unit gradient ((1 / n) * w) * (2 * d)
__device__ __forceinline__ void dloss_pixel(float p, float z, const float* tab, float mult, int bucket_num, float inv_n, float& t, float& g) {
    float w = 1.0f;
    if (tab && z == z) w = tab[dir_scaled_bucket(z, mult, 0, bucket_num - 1)];
    const float d = p - z;
    t = (d * d) * w;
    g = (inv_n * w) * (2.0f * d);
}

__global__ void __launch_bounds__(DIR_TPB)
depth_loss_kernel(const float* __restrict__ pred, const float* __restrict__ depth, int n, int off, bool vec, float mult,
                  const float* __restrict__ table, int bucket_num, float* __restrict__ dx, double* __restrict__ partials) {
    __shared__ float tab_lds[DLOSS_MAX_BUCKETS];
    __shared__ double sh[DIR_TPB / DIR_WAVE];
    if (table) {
        for (int i = threadIdx.x; i < bucket_num; i += DIR_TPB) tab_lds[i] = table[i];
        __syncthreads();
    }
    const float* tab = table ? tab_lds : nullptr;
    const float inv_n = 1.0f / (float)n;
    const int quads = (n + off + 3) / 4;
    double acc = 0.0;
    for (int q = (int)blockIdx.x * DIR_TPB + (int)threadIdx.x; q < quads; q += (int)gridDim.x * DIR_TPB) {
        const DirQuad<long long> d = dir_quad<long long>(q, quads, off, n);
        if (d.full && vec) {                                                      // two 16-byte loads issued together, one 16-byte store
            const bool all[4] = {true, true, true, true};                         // a full quad: every element exists
            float z[4], p[4], t[4], g[4];
            dir_quad_load(depth, d, true, all, 0.0f, z);
            dir_quad_load(pred, d, true, all, 0.0f, p);
#pragma unroll
            for (int j = 0; j < 4; ++j) dloss_pixel(p[j], z[j], tab, mult, bucket_num, inv_n, t[j], g[j]);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)t[j];                      // index order
            if (dx) *reinterpret_cast<float4*>(dx + d.i0) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
            for (int j = 0; j < 4; ++j) {
                const long long i = d.i0 + j;
                if (i < 0 || i >= n) continue;                                    // an element outside [0, n) is skipped
                float t, g;
                dloss_pixel(pred[i], depth[i], tab, mult, bucket_num, inv_n, t, g);
                acc += (double)t;
                if (dx) dx[i] = g;
            }
        }
    }
    const double tot = dir_block_sum(acc, sh);                                    // wave order
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

static_assert(DLOSS_MAX_BLOCKS <= DIR_TPB, "the fold stages one partial per thread");

__global__ void __launch_bounds__(DIR_TPB)
depth_loss_fold_kernel(const double* __restrict__ partials, int blocks, int n, float* __restrict__ loss) {
    __shared__ double sh[DLOSS_MAX_BLOCKS];
    sh[threadIdx.x] = (int)threadIdx.x < blocks ? partials[threadIdx.x] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int g = 0; g < blocks; ++g) tot += sh[g];                            // workgroup order
        loss[0] = (float)(tot / (double)n);
    }
}

extern "C" size_t dir_depth_loss_workspace(long long n) {
    if (n <= 0) return 0;
    return dir_align_up(sizeof(double) * (size_t)dir_quad_grid(n, DLOSS_MAX_BLOCKS), 256);
}

extern "C" int dir_depth_loss(const float* pred, const float* depth, long long n, float mult, const float* table, int bucket_num,
                              float* loss, float* dx_unit, void* workspace, size_t workspace_bytes, dir_stream_t stream) {
    DIR_RETURN_IF(!pred || !depth || !loss || n <= 0, DIR_EINVAL);
    DIR_RETURN_IF(table && bucket_num <= 0, DIR_EINVAL);
    DIR_RETURN_IF(bucket_num > DLOSS_MAX_BUCKETS || n > 2100000000LL, DIR_EUNSUPPORTED);   // 32-bit pixel indices: split the batch
    DIR_RETURN_IF(dir_misaligned(pred, 4) || dir_misaligned(depth, 4) || dir_misaligned(dx_unit, 4) || dir_misaligned(workspace, 8), DIR_EINVAL);
    DIR_RETURN_IF(!workspace || workspace_bytes < dir_depth_loss_workspace(n), DIR_EINVAL);
    const int grid = dir_quad_grid(n, DLOSS_MAX_BLOCKS);
    // 16-byte accesses to pred and dx_unit when both sit at depth's offset (all three 16-byte aligned is offset 0), element-wise otherwise
    const int off = dir_quad_offset(depth);
    const bool vec = dir_quad_same_offset(pred, off) && (!dx_unit || dir_quad_same_offset(dx_unit, off));
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(depth_loss_kernel, dim3(grid), dim3(DIR_TPB), 0, dir_s(stream), pred, depth, (int)n, off, vec, mult,
                       table, bucket_num, dx_unit, partials);
    DIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(depth_loss_fold_kernel, dim3(1), dim3(DIR_TPB), 0, dir_s(stream), partials, grid, (int)n, loss);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}
