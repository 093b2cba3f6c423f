// NYUD2-DIR balanced depth evaluation (nyud2-dir/util.py:35-133 `Evaluator`, nyud2-dir/test.py:39-59) as ONE streaming pass:
// per kept pixel the eight terms of RMSE / MAE / ABS_REL / LG10 / delta1-3 / NUM, summed per 0.1 m depth bucket into a
// [bucket_num][8] float64 table.  The reference upsamples the prediction (F.interpolate bilinear, align_corners=True), boolean-
// indexes, copies everything to the host and maps a Python function over every pixel; here the upsampled value is formed in
// registers and nothing per pixel is ever written.
//
// Reduction, bit-reproducible (no float atomics anywhere):
//   thread   one quad of the grid anchored at `depth` per step (dir_reduce_shared.h), terms in float32 as the reference forms them
//   wave     per distinct bucket among the lanes (depth is spatially smooth: usually 1-3), a 64-lane butterfly sum in float64;
//            lane 0 adds it to the wave's PRIVATE LDS table (program order, no atomics)
//   block    the four wave tables added in wave order -> one [bucket_num][8] float64 partial in the workspace (dir_slots_write)
//   fold     a second launch adds the partials in block order onto the caller's table (dir_table_fold)
// The three delta columns and NUM are counts: packed 4 x 16 bit through the butterfly, uint32 in LDS, exact in float64.
#include "dir_reduce_shared.h"

#define EVAL_MAX_BUCKETS 256                  // LDS: 4 waves x bucket_num x 48 B <= 48 KB
#define EVAL_MAX_BLOCKS 1024
#define EVAL_LN10 2.30258509299404568402f     // (float)math.log(10)

typedef DirSlot<4, 4> EvalSlot;               // one bucket row of a wave's LDS table: d*d, d, d/depth, |lg10 pred - lg10 depth| and
                                              // the counts delta1, delta2, delta3, NUM

struct EvalTerms {
    double s[4];
    unsigned long long c;                     // 4 x 16-bit counts: delta1 | delta2 << 16 | delta3 << 32 | NUM << 48
    int b;                                    // bucket, -1 = nothing to add
};

// one pixel's terms; its bucket is Evaluator.get_bin_idx = dir_scaled_bucket from 0, -1 for a dropped pixel (a NaN depth is dropped)
__device__ __forceinline__ void eval_pixel(float p, float z, bool keep, float mult, int bucket_num, float t[4], unsigned long long& c, int& b) {
    b = keep ? dir_scaled_bucket(z, mult, 0, bucket_num - 1) : -1;
    const float d = fabsf(p - z);
    t[0] = d * d;
    t[1] = d;
    t[2] = d / z;
    t[3] = fabsf(logf(p) / EVAL_LN10 - logf(z) / EVAL_LN10);
    const float yz = p / z, zy = z / p;
    const float r = (yz < zy) ? zy : yz;      // maxOfTwo: a NaN ratio stays NaN and passes no threshold
    c = (r <= 1.25f ? 1ull : 0ull) | (r <= 1.5625f ? 1ull << 16 : 0ull) | (r <= 1.953125f ? 1ull << 32 : 0ull) | (1ull << 48);
}

// bilinear, align_corners=True, float32 steps:  s = i * ((in - 1) / (out - 1)),  i0 = min(int(s), in - 1),  l = s - i0,  hgh = 1 - l,
// value = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11)
__device__ __forceinline__ float eval_bilinear(const float* __restrict__ img, int h, int w, int Y, int X, float sy, float sx) {
    const float fy = (float)Y * sy, fx = (float)X * sx;
    int y0 = (int)fy; if (y0 > h - 1) y0 = h - 1;
    int x0 = (int)fx; if (x0 > w - 1) x0 = w - 1;
    const int y1 = y0 < h - 1 ? y0 + 1 : y0, x1 = x0 < w - 1 ? x0 + 1 : x0;
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    const float v00 = img[y0 * w + x0], v01 = img[y0 * w + x1], v10 = img[y1 * w + x0], v11 = img[y1 * w + x1];
    return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}

// every lane's terms into the wave's table: one butterfly per distinct bucket, lanes of other buckets contribute +0.0
__device__ __forceinline__ void eval_wave_add(EvalSlot* __restrict__ tab, const EvalTerms& t, int lane) {
    unsigned long long todo = __ballot(t.b >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int bb = __shfl(t.b, leader, DIR_WAVE);
        const bool m = t.b == bb;
        double v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = dir_wave_sum(m ? t.s[k] : 0.0);
        const unsigned long long cs = dir_wave_sum_u64(m ? t.c : 0ull);        // <= 64 lanes x 4 pixels per field
        if (lane == 0) {
            EvalSlot& e = tab[bb];
#pragma unroll
            for (int k = 0; k < 4; ++k) { e.s[k] += v[k]; e.c[k] += (uint32_t)((cs >> (16 * k)) & 0xffffu); }
        }
        todo &= ~__ballot(m);
    }
}

template <bool UPSAMPLE>
__global__ void __launch_bounds__(DIR_TPB)
depth_eval_kernel(const float* __restrict__ pred, const float* __restrict__ depth, const uint8_t* __restrict__ mask,
                  int n, int off, int h, int w, int H, int W, float sy, float sx, float mult, int bucket_num,
                  bool pred_vec, bool mask_vec, double* __restrict__ partials) {
    extern __shared__ __align__(16) unsigned char eval_smem[];
    EvalSlot* tabs = reinterpret_cast<EvalSlot*>(eval_smem);                      // [4 waves][bucket_num]
    dir_slots_zero(tabs, bucket_num);
    __syncthreads();
    const int lane = threadIdx.x & (DIR_WAVE - 1);
    EvalSlot* tab = tabs + (threadIdx.x / DIR_WAVE) * bucket_num;

    const int quads = (n + off + 3) / 4;
    const int rounds = (quads + (int)gridDim.x * DIR_TPB - 1) / ((int)gridDim.x * DIR_TPB);       // whole waves stay in the loop (shuffles)
    for (int it = 0; it < rounds; ++it) {
        const int q = (it * (int)gridDim.x + (int)blockIdx.x) * DIR_TPB + (int)threadIdx.x;
        const DirQuad<int> d = dir_quad<int>(q, quads, off, n);
        const int i0 = d.i0;
        float z[4], p[4];
        bool in[4], keep[4];
        dir_quad_in(d, n, in);
        dir_quad_load(depth, d, true, in, 0.0f, z);
        dir_quad_keep(mask, d, mask_vec, in, keep);
#pragma unroll
        for (int j = 0; j < 4; ++j) keep[j] = keep[j] && (z[j] == z[j]);          // setNanToZero: a NaN depth is in no sum and not in NUM
        if (UPSAMPLE) {
            const int ic = i0 < 0 ? 0 : i0;
            unsigned row = (unsigned)ic / (unsigned)W;
            int X = ic - (int)row * W - (ic - i0);                                // column of element i0 (negative in the lead-in)
            unsigned im = row / (unsigned)H;
            int Y = (int)(row - im * (unsigned)H);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                p[j] = keep[j] ? eval_bilinear(pred + (size_t)im * h * w, h, w, Y, X, sy, sx) : 1.0f;
                if (++X == W) { X = 0; if (++Y == H) { Y = 0; ++im; } }
            }
        } else {
            dir_quad_load(pred, d, pred_vec, keep, 1.0f, p);                      // a dropped prediction is 1: logf stays defined
        }

        float t[4][4];
        unsigned long long c[4];
        int b[4];
        int b_first = -1;
        bool one_bucket = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            eval_pixel(p[j], z[j], keep[j], mult, bucket_num, t[j], c[j], b[j]);
            if (!keep[j]) continue;
            if (b_first < 0) b_first = b[j];
            else one_bucket = one_bucket && b[j] == b_first;
        }
        EvalTerms e;
        if (__all(one_bucket)) {                                                  // usual case: the thread's kept pixels share a bucket
            e.b = b_first; e.c = 0ull;
#pragma unroll
            for (int k = 0; k < 4; ++k) e.s[k] = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (keep[j]) {
                    e.c += c[j];
#pragma unroll
                    for (int k = 0; k < 4; ++k) e.s[k] += (double)t[j][k];
                }
            }
            eval_wave_add(tab, e, lane);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                e.b = b[j]; e.c = c[j];
#pragma unroll
                for (int k = 0; k < 4; ++k) e.s[k] = (double)t[j][k];
                eval_wave_add(tab, e, lane);
            }
        }
    }
    __syncthreads();
    dir_slots_write(tabs, bucket_num, partials + (size_t)blockIdx.x * bucket_num * 8);
}

extern "C" size_t dir_depth_eval_workspace(long long n, int bucket_num) {
    if (n <= 0 || bucket_num <= 0 || bucket_num > EVAL_MAX_BUCKETS) return 0;
    return (size_t)dir_quad_grid(n, EVAL_MAX_BLOCKS) * bucket_num * 8 * sizeof(double);
}

extern "C" int dir_depth_eval_accumulate(const float* pred, const float* depth, const uint8_t* mask, int N, int h, int w, int H, int W,
                                         float mult, int bucket_num, double* table, void* workspace, size_t workspace_bytes,
                                         dir_stream_t stream) {
    DIR_RETURN_IF(N < 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || bucket_num <= 0 || !(mult > 0.0f), DIR_EINVAL);
    DIR_RETURN_IF(bucket_num > EVAL_MAX_BUCKETS, DIR_EUNSUPPORTED);
    if (N == 0) return DIR_OK;
    DIR_RETURN_IF(!pred || !depth || !table || !workspace, DIR_EINVAL);
    DIR_RETURN_IF(dir_misaligned(pred, 4) || dir_misaligned(depth, 4) || dir_misaligned(table, 8) || dir_misaligned(workspace, 8), DIR_EINVAL);
    const long long n = (long long)N * H * W, np = (long long)N * h * w;
    DIR_RETURN_IF(n > 2100000000LL || np > 2100000000LL, DIR_EUNSUPPORTED);       // 32-bit pixel indices (4 * quad of the last round included): split the batch
    DIR_RETURN_IF(workspace_bytes < dir_depth_eval_workspace(n, bucket_num), DIR_EWORKSPACE);
    const int grid = dir_quad_grid(n, EVAL_MAX_BLOCKS);
    const int off = dir_quad_offset(depth);
    const bool up = h != H || w != W;
    const bool pred_vec = !up && dir_quad_same_offset(pred, off);
    const bool mask_vec = dir_quad_mask_aligned(mask, off);
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.0f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.0f;
    const size_t lds = (size_t)4 * bucket_num * sizeof(EvalSlot);
    double* partials = static_cast<double*>(workspace);
    if (up)
        hipLaunchKernelGGL(depth_eval_kernel<true>, dim3(grid), dim3(DIR_TPB), lds, dir_s(stream), pred, depth, mask, (int)n, off, h, w, H, W,
                           sy, sx, mult, bucket_num, pred_vec, mask_vec, partials);
    else
        hipLaunchKernelGGL(depth_eval_kernel<false>, dim3(grid), dim3(DIR_TPB), lds, dir_s(stream), pred, depth, mask, (int)n, off, h, w, H, W,
                           sy, sx, mult, bucket_num, pred_vec, mask_vec, partials);
    DIR_LAUNCH_CHECK();
    return dir_table_fold(partials, grid, bucket_num * 8, table, stream);
}
