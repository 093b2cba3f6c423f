// NYUD2-DIR balanced depth evaluation (nyud2-dir/util.py:35-133 `Evaluator`, nyud2-dir/test.py:39-59) as ONE streaming pass:
// per kept pixel the eight terms of RMSE / MAE / ABS_REL / LG10 / delta1-3 / NUM, summed per 0.1 m depth bucket into a
// [bucket_num][8] float64 table.  The reference upsamples the prediction (F.interpolate bilinear, align_corners=True), boolean-
// indexes, copies everything to the host and maps a Python function over every pixel; here the upsampled value is formed in
// registers and nothing per pixel is ever written.
//
// Reduction, bit-reproducible (no float atomics anywhere):
//   thread   one aligned 16-byte quad of `depth` per step (edge quads element-wise), terms in float32 as the reference forms them
//   wave     per distinct bucket among the lanes (depth is spatially smooth: usually 1-3), a 64-lane butterfly sum in float64;
//            lane 0 adds it to the wave's PRIVATE LDS table (program order, no atomics)
//   block    the four wave tables added in wave order -> one [bucket_num][8] float64 partial in the workspace
//   fold     a second launch adds the partials in block order onto the caller's table
// The three delta columns and NUM are counts: packed 4 x 16 bit through the butterfly, uint32 in LDS, exact in float64.
#include "dir_common.h"

#define EVAL_MAX_BUCKETS 256                  // LDS: 4 waves x bucket_num x 48 B <= 48 KB
#define EVAL_MAX_BLOCKS 1024
#define EVAL_LN10 2.30258509299404568402f     // (float)math.log(10)

struct EvalSlot {                             // one bucket row of a wave's LDS table
    double s[4];                              // d*d, d, d/depth, |lg10 pred - lg10 depth|
    uint32_t c[4];                            // delta1, delta2, delta3, NUM
};

struct EvalTerms {
    double s[4];
    unsigned long long c;                     // 4 x 16-bit counts: delta1 | delta2 << 16 | delta3 << 32 | NUM << 48
    int b;                                    // bucket, -1 = nothing to add
};

static int eval_grid(long long n) {
    const long long quads = (n + 3 + 3) / 4;  // the quad grid is anchored at the 16-byte boundary below `depth`: up to 3 slots of lead-in
    long long g = (quads + DIR_TPB - 1) / DIR_TPB;
    if (g > EVAL_MAX_BLOCKS) g = EVAL_MAX_BLOCKS;
    return g < 1 ? 1 : (int)g;
}

// Evaluator.get_bin_idx: min(int(depth * mult), bucket_num - 1), the float32 product truncated (as dir_fds_bin_scaled, bucket_start 0)
__device__ __forceinline__ int eval_bucket(float depth, float mult, int bucket_num) {
    const float v = depth * mult;
    int k = (v >= 2147483520.0f) ? 2147483647 : ((v <= 0.0f) ? 0 : (int)v);
    return k > bucket_num - 1 ? bucket_num - 1 : k;
}

__device__ __forceinline__ void eval_pixel(float p, float z, float mult, int bucket_num, float t[4], unsigned long long& c, int& b) {
    b = eval_bucket(z, mult, bucket_num);
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

__device__ __forceinline__ unsigned long long eval_wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, DIR_WAVE);
    return v;
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
        const unsigned long long cs = eval_wave_sum_u64(m ? t.c : 0ull);       // <= 64 lanes x 4 pixels per field
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
    for (int i = threadIdx.x; i < 4 * bucket_num * (int)(sizeof(EvalSlot) / 4); i += DIR_TPB) reinterpret_cast<uint32_t*>(eval_smem)[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & (DIR_WAVE - 1);
    EvalSlot* tab = tabs + (threadIdx.x / DIR_WAVE) * bucket_num;

    const int quads = (n + off + 3) / 4;
    const int rounds = (quads + (int)gridDim.x * DIR_TPB - 1) / ((int)gridDim.x * DIR_TPB);       // whole waves stay in the loop (shuffles)
    for (int it = 0; it < rounds; ++it) {
        const int q = (it * (int)gridDim.x + (int)blockIdx.x) * DIR_TPB + (int)threadIdx.x;
        const int i0 = 4 * q - off;                                               // may be < 0 (lead-in) or reach past n (tail)
        float z[4], p[4];
        bool keep[4];
        const bool inside = q < quads;
        const bool full = inside && i0 >= 0 && i0 + 3 < n;
        if (full) {
            const float4 zv = *reinterpret_cast<const float4*>(depth + i0);       // 16-byte aligned by construction of the quad grid
            z[0] = zv.x; z[1] = zv.y; z[2] = zv.z; z[3] = zv.w;
            if (mask) {
                if (mask_vec) {
                    const uint32_t mv = *reinterpret_cast<const uint32_t*>(mask + i0);
#pragma unroll
                    for (int j = 0; j < 4; ++j) keep[j] = ((mv >> (8 * j)) & 0xffu) != 0;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) keep[j] = mask[i0 + j] != 0;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) keep[j] = true;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + j;
                const bool in = inside && i >= 0 && i < n;
                z[j] = in ? depth[i] : 0.0f;
                keep[j] = in && (!mask || mask[i] != 0);
            }
        }
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
        } else if (full && pred_vec) {
            const float4 pv = *reinterpret_cast<const float4*>(pred + i0);
            p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = keep[j] ? pred[i0 + j] : 1.0f;
        }

        float t[4][4];
        unsigned long long c[4];
        int b[4];
        int b_first = -1;
        bool one_bucket = true;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            eval_pixel(p[j], z[j], mult, bucket_num, t[j], c[j], b[j]);
            if (!keep[j]) b[j] = -1;
            else if (b_first < 0) b_first = b[j];
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
    double* out = partials + (size_t)blockIdx.x * bucket_num * 8;
    for (int i = threadIdx.x; i < bucket_num * 8; i += DIR_TPB) {
        const int bkt = i >> 3, col = i & 7;
        double v = 0.0;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) {                                          // wave order
            const EvalSlot& s = tabs[wv * bucket_num + bkt];
            v += col < 4 ? s.s[col] : (double)s.c[col - 4];
        }
        out[i] = v;
    }
}

__global__ void __launch_bounds__(DIR_TPB)
depth_eval_fold_kernel(const double* __restrict__ partials, int blocks, int entries, double* __restrict__ table) {
    const int i = blockIdx.x * DIR_TPB + threadIdx.x;
    if (i >= entries) return;
    double v = 0.0;
#pragma unroll 8
    for (int g = 0; g < blocks; ++g) v += partials[(size_t)g * entries + i];       // block order
    table[i] += v;
}

extern "C" size_t dir_depth_eval_workspace(long long n, int bucket_num) {
    if (n <= 0 || bucket_num <= 0 || bucket_num > EVAL_MAX_BUCKETS) return 0;
    return (size_t)eval_grid(n) * bucket_num * 8 * sizeof(double);
}

extern "C" int dir_depth_eval_accumulate(const float* pred, const float* depth, const uint8_t* mask, int N, int h, int w, int H, int W,
                                         float mult, int bucket_num, double* table, void* workspace, size_t workspace_bytes,
                                         dir_stream_t stream) {
    DIR_RETURN_IF(N < 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || bucket_num <= 0 || !(mult > 0.0f), DIR_EINVAL);
    DIR_RETURN_IF(bucket_num > EVAL_MAX_BUCKETS, DIR_EUNSUPPORTED);
    if (N == 0) return DIR_OK;
    DIR_RETURN_IF(!pred || !depth || !table || !workspace, DIR_EINVAL);
    DIR_RETURN_IF((reinterpret_cast<uintptr_t>(pred) & 3u) || (reinterpret_cast<uintptr_t>(depth) & 3u) ||
                  (reinterpret_cast<uintptr_t>(table) & 7u) || (reinterpret_cast<uintptr_t>(workspace) & 7u), DIR_EINVAL);
    const long long n = (long long)N * H * W, np = (long long)N * h * w;
    DIR_RETURN_IF(n > 2100000000LL || np > 2100000000LL, DIR_EUNSUPPORTED);       // 32-bit pixel indices (4 * quad of the last round included): split the batch
    DIR_RETURN_IF(workspace_bytes < dir_depth_eval_workspace(n, bucket_num), DIR_EWORKSPACE);
    const int grid = eval_grid(n);
    const int off = (int)((reinterpret_cast<uintptr_t>(depth) >> 2) & 3u);        // elements between the 16-byte boundary below and depth[0]
    const bool up = h != H || w != W;
    const bool pred_vec = !up && ((reinterpret_cast<uintptr_t>(pred) >> 2) & 3u) == (unsigned)off;
    const bool mask_vec = mask && ((reinterpret_cast<uintptr_t>(mask) - (uintptr_t)off) & 3u) == 0;
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
    const int entries = bucket_num * 8;
    hipLaunchKernelGGL(depth_eval_fold_kernel, dim3(dir_cdiv(entries, DIR_TPB)), dim3(DIR_TPB), 0, dir_s(stream), partials, grid, entries, table);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}
