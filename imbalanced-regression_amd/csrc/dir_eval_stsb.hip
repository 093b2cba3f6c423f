// Balanced STS-B evaluation (sts-b-dir/util.py:101-172 `STSShotAverage.get_metric`) over the WHOLE evaluation set: per shot group
// (many / medium / few / overall) the sums behind MSE, L1, G-Mean, Pearson and Spearman.  The reference keeps python lists on the
// host, bins every label with a numpy call of its own and hands four slices to scipy; here the host reads 60 numbers.
//
//   launch 1  moments   one sample per thread: bin by a search over the edge table in LDS, group id to the workspace, the terms in
//                       float64 as the reference forms them (p = 5.0 * (double)pred, l = (double)label, d = |p - l|), per group a
//                       wavefront butterfly, the four wave sums in wave order -> one [3][10] float64 partial per workgroup
//   launch 2  ranks     the hot path, O(n^2) compares and no sort: thread i counts, over every j, pred_j < pred_i, pred_j == pred_i,
//                       label_j < label_i, label_j == label_i, once over all samples and once over its own group.  The doubled
//                       average rank with ties is the integer 2 * less + equal + 1; Spearman's rho follows on the host from five
//                       integer sums per group (sum a, sum b, sum a^2, sum b^2, sum ab), so it is exact and independent of sample order
//   launch 3  fold      one workgroup adds the partials in workgroup order, forms the overall moment row as many + medium + few and
//                       writes the two tables
// No float atomics anywhere: the moment table is bit-reproducible.  The rank sums are integers (LDS integer adds, then a fold in
// workgroup order): integer addition is associative, no order can change a bit.
//
// LDS layout of the rank kernel: the j tile of one workgroup as three arrays (pred[256], label[256] float32, group[256] bytes).  Every
// lane of a wavefront reads the SAME j, so each read is one broadcast address (no bank conflict whatever the layout); the arrays are
// read 16 bytes (4 samples) at a time to keep the LDS instruction count at 3 per 4 samples next to ~14 VALU operations per sample.
// The tail of the last tile is padded with NaN, which is neither less than nor equal to anything: padding counts nowhere.
#include "dir_common.h"
#include <math.h>

#define STSB_MAX_N 65536
#define STSB_MAX_BINS 256
#define STSB_GROUPS 3
#define STSB_MCOLS 10                          // NUM, ZERO, sum d^2, sum d, sum ln d, sum p', sum l', sum p'^2, sum l'^2, sum p'l'
#define STSB_MSUMS 8                           // the float64 columns (2..9)
#define STSB_MSTRIDE 32                        // doubles per workgroup partial: [3][10] + the invalid-sample count at 30
#define STSB_RCOLS 5                           // sum a, sum b, sum a^2, sum b^2, sum ab
#define STSB_RSTRIDE ((STSB_GROUPS + 1) * STSB_RCOLS)
#define STSB_INVALID 3                         // group id of a sample that is in no sum
#define STSB_SHIFT 2.5                         // the middle of [0, 5]: raw moments of p - 2.5, l - 2.5 lose no digits to the mean

static int stsb_grid(long long n) { return (int)((n + DIR_TPB - 1) / DIR_TPB); }
static size_t stsb_gid_bytes(long long n) { return dir_align_up((size_t)n, 256); }

__global__ void __launch_bounds__(DIR_TPB)
stsb_moments_kernel(const float* __restrict__ pred, const float* __restrict__ label, int n, const float* __restrict__ edges,
                    int num_bins, const uint8_t* __restrict__ group_of_bin, uint8_t* __restrict__ gid, double* __restrict__ partials) {
    __shared__ float s_edges[STSB_MAX_BINS + 1];
    __shared__ uint8_t s_group[STSB_MAX_BINS];
    __shared__ double s_red[DIR_TPB / DIR_WAVE][STSB_MSTRIDE];
    for (int k = threadIdx.x; k <= num_bins; k += DIR_TPB) s_edges[k] = edges[k];
    for (int k = threadIdx.x; k < num_bins; k += DIR_TPB) s_group[k] = group_of_bin[k];
    __syncthreads();

    const int i = blockIdx.x * DIR_TPB + threadIdx.x;
    int g = -1;                                                                    // -1: no sample (past n), STSB_INVALID: counted as invalid
    double t[STSB_MSUMS];
#pragma unroll
    for (int c = 0; c < STSB_MSUMS; ++c) t[c] = 0.0;
    bool zero = false;
    if (i < n) {
        const float lf = label[i], pf = pred[i];
        g = STSB_INVALID;
        if (lf >= s_edges[0] && lf <= s_edges[num_bins] && pf == pf) {            // a NaN label fails both comparisons
            int lo = 0, hi = num_bins + 1;                                         // number of edges <= label: first edge > label
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_edges[mid] <= lf) lo = mid + 1; else hi = mid;
            }
            int bin = lo - 1;
            if (bin > num_bins - 1) bin = num_bins - 1;                            // label == edges[num_bins] (util.py:117-118)
            const int gb = s_group[bin];
            if (gb < STSB_GROUPS) g = gb;
        }
        gid[i] = (uint8_t)g;
        if (g != STSB_INVALID) {
            const double p = 5.0 * (double)pf, l = (double)lf;                     // util.py:143-144
            const double d = fabs(p - l);
            const double ps = p - STSB_SHIFT, ls = l - STSB_SHIFT;
            zero = d == 0.0;
            t[0] = d * d; t[1] = d; t[2] = d > 0.0 ? log(d) : 0.0;
            t[3] = ps; t[4] = ls; t[5] = ps * ps; t[6] = ls * ls; t[7] = ps * ls;
        }
    }
    const int lane = threadIdx.x & (DIR_WAVE - 1), wave = threadIdx.x / DIR_WAVE;
#pragma unroll
    for (int gg = 0; gg < STSB_GROUPS; ++gg) {
        const bool mine = g == gg;
        const uint32_t num = dir_wave_sum_u32(mine ? 1u : 0u);
        const uint32_t zer = dir_wave_sum_u32(mine && zero ? 1u : 0u);
        if (lane == 0) { s_red[wave][gg * STSB_MCOLS] = (double)num; s_red[wave][gg * STSB_MCOLS + 1] = (double)zer; }
#pragma unroll
        for (int c = 0; c < STSB_MSUMS; ++c) {
            const double v = dir_wave_sum(mine ? t[c] : 0.0);                      // adding 0.0 changes no sum
            if (lane == 0) s_red[wave][gg * STSB_MCOLS + 2 + c] = v;
        }
    }
    const uint32_t bad = dir_wave_sum_u32(g == STSB_INVALID ? 1u : 0u);
    if (lane == 0) { s_red[wave][30] = (double)bad; s_red[wave][31] = 0.0; }
    __syncthreads();
    if (threadIdx.x < STSB_MSTRIDE) {
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < DIR_TPB / DIR_WAVE; ++w) v += s_red[w][threadIdx.x];   // wave order
        partials[(size_t)blockIdx.x * STSB_MSTRIDE + threadIdx.x] = v;
    }
}

// one j: the eight counters of thread i (less / equal, pred / label, all samples / own group)
#define STSB_COUNT(PJ, LJ, GJ) do {                                                                                       \
        const uint32_t same_ = (GJ) == gi ? 1u : 0u;                                                                     \
        const uint32_t pl_ = (PJ) < pi ? 1u : 0u, pe_ = (PJ) == pi ? 1u : 0u;                                            \
        const uint32_t ll_ = (LJ) < li ? 1u : 0u, le_ = (LJ) == li ? 1u : 0u;                                            \
        p_less += pl_; p_eq += pe_; l_less += ll_; l_eq += le_;                                                          \
        pg_less += pl_ & same_; pg_eq += pe_ & same_; lg_less += ll_ & same_; lg_eq += le_ & same_;                      \
    } while (0)

__global__ void __launch_bounds__(DIR_TPB)
stsb_rank_kernel(const float* __restrict__ pred, const float* __restrict__ label, const uint8_t* __restrict__ gid, int n,
                 unsigned long long* __restrict__ partials) {
    __shared__ __align__(16) float s_pred[DIR_TPB];
    __shared__ __align__(16) float s_label[DIR_TPB];
    __shared__ __align__(16) uint8_t s_gid[DIR_TPB];
    __shared__ unsigned long long s_acc[STSB_RSTRIDE];
    if (threadIdx.x < STSB_RSTRIDE) s_acc[threadIdx.x] = 0ull;
    const float qnan = __int_as_float(0x7fc00000);
    const int i = blockIdx.x * DIR_TPB + threadIdx.x;
    const bool in = i < n;
    const float pi = in ? pred[i] : qnan, li = in ? label[i] : qnan;
    const uint32_t gi = in ? gid[i] : 0xfeu;
    uint32_t p_less = 0, p_eq = 0, l_less = 0, l_eq = 0, pg_less = 0, pg_eq = 0, lg_less = 0, lg_eq = 0;

    const int tiles = (n + DIR_TPB - 1) / DIR_TPB;
    int j = threadIdx.x;
    float pn = j < n ? pred[j] : qnan, ln = j < n ? label[j] : qnan;                 // the next tile, loaded while the current one is compared
    uint8_t gn = j < n ? gid[j] : (uint8_t)0xff;
    for (int t = 0; t < tiles; ++t) {
        __syncthreads();                                                           // every lane is done with the previous tile
        s_pred[threadIdx.x] = pn; s_label[threadIdx.x] = ln; s_gid[threadIdx.x] = gn;
        __syncthreads();
        j = (t + 1) * DIR_TPB + threadIdx.x;
        if (t + 1 < tiles) {
            pn = j < n ? pred[j] : qnan; ln = j < n ? label[j] : qnan; gn = j < n ? gid[j] : (uint8_t)0xff;
        }
#pragma unroll 4
        for (int k = 0; k < DIR_TPB / 4; ++k) {
            const float4 p4 = reinterpret_cast<const float4*>(s_pred)[k];          // one address for the whole wavefront: a broadcast
            const float4 l4 = reinterpret_cast<const float4*>(s_label)[k];
            const uint32_t g4 = reinterpret_cast<const uint32_t*>(s_gid)[k];
            STSB_COUNT(p4.x, l4.x, g4 & 0xffu);
            STSB_COUNT(p4.y, l4.y, (g4 >> 8) & 0xffu);
            STSB_COUNT(p4.z, l4.z, (g4 >> 16) & 0xffu);
            STSB_COUNT(p4.w, l4.w, g4 >> 24);
        }
    }
    if (in && gi < STSB_GROUPS) {
        const unsigned long long a = 2ull * p_less + p_eq + 1ull, b = 2ull * l_less + l_eq + 1ull;          // doubled ranks, whole set
        const unsigned long long ag = 2ull * pg_less + pg_eq + 1ull, bg = 2ull * lg_less + lg_eq + 1ull;    // within the own group
        unsigned long long* own = s_acc + gi * STSB_RCOLS;
        unsigned long long* all = s_acc + STSB_GROUPS * STSB_RCOLS;
        atomicAdd(own + 0, ag); atomicAdd(own + 1, bg); atomicAdd(own + 2, ag * ag); atomicAdd(own + 3, bg * bg); atomicAdd(own + 4, ag * bg);
        atomicAdd(all + 0, a); atomicAdd(all + 1, b); atomicAdd(all + 2, a * a); atomicAdd(all + 3, b * b); atomicAdd(all + 4, a * b);
    }
    __syncthreads();
    if (threadIdx.x < STSB_RSTRIDE) partials[(size_t)blockIdx.x * STSB_RSTRIDE + threadIdx.x] = s_acc[threadIdx.x];
}

__global__ void __launch_bounds__(DIR_TPB)
stsb_fold_kernel(const double* __restrict__ mpart, const unsigned long long* __restrict__ rpart, int blocks,
                 double* __restrict__ moments, long long* __restrict__ ranks) {
    __shared__ double s_m[STSB_MSTRIDE];
    __shared__ unsigned long long s_r[STSB_RSTRIDE];
    const int t = threadIdx.x;
    if (t < STSB_MSTRIDE) {
        double v = 0.0;
        for (int b = 0; b < blocks; ++b) v += mpart[(size_t)b * STSB_MSTRIDE + t];                 // workgroup order
        s_m[t] = v;
    } else if (t >= DIR_WAVE && t < DIR_WAVE + STSB_RSTRIDE) {
        unsigned long long v = 0ull;
        for (int b = 0; b < blocks; ++b) v += rpart[(size_t)b * STSB_RSTRIDE + (t - DIR_WAVE)];
        s_r[t - DIR_WAVE] = v;
    }
    __syncthreads();
    if (t < STSB_GROUPS * STSB_MCOLS) moments[t] = s_m[t];
    if (t < STSB_MCOLS) moments[STSB_GROUPS * STSB_MCOLS + t] = (s_m[t] + s_m[STSB_MCOLS + t]) + s_m[2 * STSB_MCOLS + t];
    if (t < STSB_RSTRIDE) {
        long long v = (long long)s_r[t];
        if (t == STSB_GROUPS * STSB_RCOLS && s_m[30] > 0.0) v = -(long long)s_m[30];              // the documented error slot
        ranks[t] = v;
    }
}

extern "C" size_t dir_stsb_eval_workspace(long long n, int num_bins) {
    if (n <= 0 || n > STSB_MAX_N || num_bins <= 0 || num_bins > STSB_MAX_BINS) return 0;
    return stsb_gid_bytes(n) + (size_t)stsb_grid(n) * (STSB_MSTRIDE * sizeof(double) + STSB_RSTRIDE * sizeof(unsigned long long));
}

extern "C" int dir_stsb_eval(const float* pred, const float* label, long long n, const float* edges, int num_bins,
                             const uint8_t* group_of_bin, double* moments, long long* ranks, void* workspace, size_t workspace_bytes,
                             dir_stream_t stream) {
    DIR_RETURN_IF(n <= 0 || num_bins <= 0, DIR_EINVAL);
    DIR_RETURN_IF(n > STSB_MAX_N || num_bins > STSB_MAX_BINS, DIR_EUNSUPPORTED);
    DIR_RETURN_IF(!pred || !label || !edges || !group_of_bin || !moments || !ranks || !workspace, DIR_EINVAL);
    DIR_RETURN_IF(dir_misaligned(pred, 4) || dir_misaligned(label, 4) || dir_misaligned(edges, 4) || dir_misaligned(moments, 8) ||
                  dir_misaligned(ranks, 8) || dir_misaligned(workspace, 8), DIR_EINVAL);
    DIR_RETURN_IF(workspace_bytes < dir_stsb_eval_workspace(n, num_bins), DIR_EWORKSPACE);
    const int grid = stsb_grid(n);
    uint8_t* gid = static_cast<uint8_t*>(workspace);
    double* mpart = reinterpret_cast<double*>(gid + stsb_gid_bytes(n));
    unsigned long long* rpart = reinterpret_cast<unsigned long long*>(mpart + (size_t)grid * STSB_MSTRIDE);
    hipLaunchKernelGGL(stsb_moments_kernel, dim3(grid), dim3(DIR_TPB), 0, dir_s(stream), pred, label, (int)n, edges, num_bins,
                       group_of_bin, gid, mpart);
    DIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(stsb_rank_kernel, dim3(grid), dim3(DIR_TPB), 0, dir_s(stream), pred, label, gid, (int)n, rpart);
    DIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(stsb_fold_kernel, dim3(1), dim3(DIR_TPB), 0, dir_s(stream), mpart, rpart, grid, moments, ranks);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}
