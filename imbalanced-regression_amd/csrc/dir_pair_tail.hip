// Fused STS-B-DIR pair head: what HeadlessPairEncoder.forward does after the LSTM and MultiTaskModel.forward up to the loss
// (sts-b-dir/models.py:155-166 and :84-92): dropout on the two sentence encodings, padding to -inf, max over time,
// cat[u, v, |u - v|, u * v], FDS.smooth in place (sts-b-dir/fds.py:127-141), Linear(4D, 1) — and its backward. The STS-B counterpart of
// dir_tail.hip; float32 only.
//
//   forward  : TWO launches.  Grid (column tile, sample): a workgroup owns 256 columns of one sample, 64 lanes x 4 columns, and its four
//              waves split the sample's rows (four runs of consecutive t per sentence, merged in t order through LDS).  16-byte loads,
//              the rows loaded whether masked or not, up to eight in flight per thread; the mask decides what enters the maximum.  The
//              Philox keep mask of dir_rng.h is regenerated on the fly, max / argmax stay in registers.  Wave 0 forms the four
//              segments, calibrates them in registers, stores emb [B, 4D] once (calibrated: the reference calibrates in place, so
//              its out['embs'] is this tensor), u / v [B, 2D] and the two argmax maps for the backward, and reduces sum emb * W over
//              the tile (wavefront shuffles) into partial[tile][b].  A fold adds the tiles in order and the bias.
//   backward : THREE launches.  Grid (column tile, sample, sentence): g = dlogits * W (+ demb), times the calibration scale, du / dv in
//              registers (the [B, 4D] gradient is never materialised), one Philox call per column for the keep factor of the argmax
//              element, then ONE streaming pass writes every element of ds: the gradient at t == arg, zero elsewhere (no memset +
//              scatter).  dweight / dbias by the fixed-order two-stage reduction over the batch of dir_tail_bwd.
// No atomics, no cooperative launch, every sum in a fixed order: bit-reproducible.  The arithmetic is one float32 rounding per
// operation (-ffp-contract=off) in the order include/dir_hip.h states, so emb, arg and ds are bit-identical to the unfused chain.
// D % 4 != 0 or a pointer off a 16-byte boundary: the same kernels with element-wise accesses (template parameter VEC).
#include <initializer_list>
#include "dir_common.h"
#include "dir_rng.h"

namespace {

constexpr int PT_COLS = 4;                                    // columns per thread: one 16-byte access
constexpr int PT_FWD_TILE = DIR_WAVE * PT_COLS;               // forward: columns per workgroup (D = 3000: 12 tiles, the last one partial)
constexpr int PT_TILE = DIR_TPB * PT_COLS;                    // backward: columns per workgroup (D = 3000: 3 tiles, the last one partial)
constexpr int PT_ROWS = 8;                                    // rows in flight per thread

__device__ __forceinline__ float pt_calib1(float x, float m1, float s, float m2) {
    return (s < 0.0f) ? x : (x - m1) * s + m2;               // = dir_fds_calibrate_fwd; s < 0 = "leave untouched"
}

__device__ __forceinline__ uint32_t pt_pick(const DirU32x4& r, uint32_t k) {      // r.v[k] without a dynamically indexed array
    return k == 0 ? r.v[0] : k == 1 ? r.v[1] : k == 2 ? r.v[2] : r.v[3];
}

// v[j] = p[i + j] for the columns c0 + j < D.  VEC: c0 < D means all four exist (D % 4 == 0) and p + i is 16-byte aligned.
template <bool VEC, typename T>
__device__ __forceinline__ void pt_load4(const T* __restrict__ p, size_t i, int c0, int D, T (&v)[4], T fill) {
    if constexpr (VEC) {
        typedef __attribute__((ext_vector_type(4))) T T4;
        const T4 t = *reinterpret_cast<const T4*>(p + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (c0 + j < D) ? p[i + j] : fill;
    }
}

template <bool VEC, typename T>
__device__ __forceinline__ void pt_store4(T* __restrict__ p, size_t i, int c0, int D, const T (&v)[4]) {
    if constexpr (VEC) {
        typedef __attribute__((ext_vector_type(4))) T T4;
        T4 t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *reinterpret_cast<T4*>(p + i) = t;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (c0 + j < D) p[i + j] = v[j];
    }
}

// drop() of the elements e0 .. e0 + 3.  VEC: e0 % 4 == 0, one Philox call; otherwise the four may straddle two groups.
template <bool VEC>
__device__ __forceinline__ void pt_drop4(const DirDropout& d, uint64_t e0, float (&v)[4]) {
    const DirU32x4 r0 = dir_dropout_bits(d, e0 >> 2);
    if constexpr (VEC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = dir_dropout_apply(d, r0.v[j], v[j]);
    } else {
        const DirU32x4 r1 = dir_dropout_bits(d, (e0 >> 2) + 1);
        const uint32_t k0 = (uint32_t)e0 & 3u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k = k0 + j;
            v[j] = dir_dropout_apply(d, k < 4 ? pt_pick(r0, k) : pt_pick(r1, k - 4), v[j]);
        }
    }
}

// Running maximum of torch.max(dim=1): the lowest t that attains it, a NaN wins over every number and the lowest NaN stays.
__device__ __forceinline__ void pt_max_step(float x, int t, float& m, int& arg) {
    if (arg < 0 || x > m || (x != x && m == m)) { m = x; arg = t; }
}

// m[j] / arg[j] of the columns c0 + j of sample b over the unmasked rows t in [tb, te) of s [B, T, D] (models.py:155-164)
template <bool VEC, bool DROP>
__device__ __forceinline__ void pt_max_over_time(const float* __restrict__ s, const uint8_t* __restrict__ mask, int b, int T, int tb,
                                                 int te, int D, int c0, const DirDropout& dr, float (&m)[4], int (&arg)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { m[j] = -INFINITY; arg[j] = -1; }
    const size_t row0 = (size_t)b * T;
    for (int t0 = tb; t0 < te; t0 += PT_ROWS) {
        float x[PT_ROWS][4];
#pragma unroll
        for (int r = 0; r < PT_ROWS; ++r)
            if (t0 + r < te) pt_load4<VEC>(s, (row0 + t0 + r) * D + c0, c0, D, x[r], 0.0f);
#pragma unroll
        for (int r = 0; r < PT_ROWS; ++r) {
            if (t0 + r < te && mask[row0 + t0 + r] != 0) {
                if constexpr (DROP) pt_drop4<VEC>(dr, (uint64_t)(row0 + t0 + r) * (uint64_t)D + (uint64_t)c0, x[r]);
#pragma unroll
                for (int j = 0; j < 4; ++j) pt_max_step(x[r][j], t0 + r, m[j], arg[j]);
            }
        }
    }
}

// One workgroup = one sample x PT_FWD_TILE columns.  Its four waves split the rows of each sentence into four runs of consecutive t
// (more waves per CU to hide the HBM latency than one thread per column quad over all rows would give); the runs are merged in t
// order with the same step rule, so the result is that of one pass over t.  Wave 0 then forms, calibrates and stores the embedding.
template <bool VEC, bool DROP>
__global__ void __launch_bounds__(DIR_TPB)
pair_fwd_kernel(const float* __restrict__ s1, const float* __restrict__ s2, const uint8_t* __restrict__ mask1,
                const uint8_t* __restrict__ mask2, int B, int T1, int T2, int D, const int32_t* __restrict__ bins, int nb,
                const float* __restrict__ m1, const float* __restrict__ scale, const float* __restrict__ m2,
                const float* __restrict__ weight, const DirDropout d1, const DirDropout d2, float* __restrict__ emb,
                float* __restrict__ uv, int32_t* __restrict__ arg1, int32_t* __restrict__ arg2, float* __restrict__ partial) {
    constexpr int WAVES = DIR_TPB / DIR_WAVE;
    __shared__ float run_m[2][WAVES][4][DIR_WAVE];            // [sentence][wave][column of the quad][lane]
    __shared__ int run_a[2][WAVES][4][DIR_WAVE];
    const int b = blockIdx.y, lane = threadIdx.x & (DIR_WAVE - 1), wave = threadIdx.x / DIR_WAVE;
    const int c0 = blockIdx.x * PT_FWD_TILE + lane * PT_COLS;
    if (c0 < D) {
        float m[4];
        int a[4];
        const int r1 = (T1 + WAVES - 1) / WAVES, r2 = (T2 + WAVES - 1) / WAVES;      // rows per run
        const int e1 = (wave + 1) * r1 < T1 ? (wave + 1) * r1 : T1, e2 = (wave + 1) * r2 < T2 ? (wave + 1) * r2 : T2;
        pt_max_over_time<VEC, DROP>(s1, mask1, b, T1, wave * r1, e1, D, c0, d1, m, a);
#pragma unroll
        for (int j = 0; j < 4; ++j) { run_m[0][wave][j][lane] = m[j]; run_a[0][wave][j][lane] = a[j]; }
        pt_max_over_time<VEC, DROP>(s2, mask2, b, T2, wave * r2, e2, D, c0, d2, m, a);
#pragma unroll
        for (int j = 0; j < 4; ++j) { run_m[1][wave][j][lane] = m[j]; run_a[1][wave][j][lane] = a[j]; }
    }
    __syncthreads();
    if (wave != 0) return;
    float dot = 0.0f;
    if (c0 < D) {
        float u[4], v[4];
        int a1[4], a2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u[j] = run_m[0][0][j][lane]; a1[j] = run_a[0][0][j][lane];
            v[j] = run_m[1][0][j][lane]; a2[j] = run_a[1][0][j][lane];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) {                                   // later runs hold later t: ties stay with the lowest
                if (run_a[0][w][j][lane] >= 0) pt_max_step(run_m[0][w][j][lane], run_a[0][w][j][lane], u[j], a1[j]);
                if (run_a[1][w][j][lane] >= 0) pt_max_step(run_m[1][w][j][lane], run_a[1][w][j][lane], v[j], a2[j]);
            }
        }
        pt_store4<VEC>(arg1, (size_t)b * D + c0, c0, D, a1);
        pt_store4<VEC>(arg2, (size_t)b * D + c0, c0, D, a2);
        pt_store4<VEC>(uv, (size_t)b * 2 * D + c0, c0, D, u);
        pt_store4<VEC>(uv, (size_t)b * 2 * D + D + c0, c0, D, v);
        float f[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { f[0][j] = u[j]; f[1][j] = v[j]; f[2][j] = fabsf(u[j] - v[j]); f[3][j] = u[j] * v[j]; }   // models.py:166
        int bin = bins ? bins[b] : -1;
        if (bin >= nb) bin = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const size_t col = (size_t)k * D + c0;
            if (bin >= 0) {
                const size_t to = (size_t)bin * 4 * D + col;
                float a[4], sc[4], c[4];
                pt_load4<VEC>(m1, to, c0, D, a, 0.0f);
                pt_load4<VEC>(scale, to, c0, D, sc, -1.0f);
                pt_load4<VEC>(m2, to, c0, D, c, 0.0f);
#pragma unroll
                for (int j = 0; j < 4; ++j) f[k][j] = pt_calib1(f[k][j], a[j], sc[j], c[j]);
            }
            pt_store4<VEC>(emb, (size_t)b * 4 * D + col, c0, D, f[k]);
            float w[4];
            pt_load4<VEC>(weight, col, c0, D, w, 0.0f);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (VEC || c0 + j < D) dot += f[k][j] * w[j];
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, DIR_WAVE);
    if (lane == 0) partial[(size_t)blockIdx.x * B + b] = dot;
}

// logits[b] = (partial[0][b] + partial[1][b] + ...) + bias, tiles in order
__global__ void __launch_bounds__(DIR_TPB)
pair_fwd_fold_kernel(const float* __restrict__ partial, int tiles, int B, const float* __restrict__ bias, float* __restrict__ logits) {
    const int b = blockIdx.x * DIR_TPB + threadIdx.x;
    if (b >= B) return;
    float s = partial[b];
    for (int z = 1; z < tiles; ++z) s += partial[(size_t)z * B + b];
    logits[b] = s + bias[0];
}

// blockIdx.z = sentence.  Writes every element of ds [B, T, D] of its (sample, column tile).
template <bool VEC, bool DROP>
__global__ void __launch_bounds__(DIR_TPB)
pair_bwd_ds_kernel(const float* __restrict__ dlogits, const float* __restrict__ demb, const int32_t* __restrict__ bins, int nb,
                   const float* __restrict__ scale, const float* __restrict__ weight, const float* __restrict__ uv,
                   const int32_t* __restrict__ arg1, const int32_t* __restrict__ arg2, int T1, int T2, int D,
                   const DirDropout d1, const DirDropout d2, float* __restrict__ ds1, float* __restrict__ ds2) {
    const bool second = blockIdx.z != 0;
    float* __restrict__ ds = second ? ds2 : ds1;
    if (!ds) return;
    const int b = blockIdx.y;
    const int c0 = blockIdx.x * PT_TILE + threadIdx.x * PT_COLS;
    if (c0 >= D) return;
    const int T = second ? T2 : T1;
    const float dl = dlogits[b];
    int bin = bins ? bins[b] : -1;
    if (bin >= nb) bin = -1;
    float g[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t col = (size_t)k * D + c0;
        float w[4];
        pt_load4<VEC>(weight, col, c0, D, w, 0.0f);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[k][j] = dl * w[j];                        // Linear backward
        if (demb) {                                                             // + a gradient that reached the returned embedding
            float e[4];
            pt_load4<VEC>(demb, (size_t)b * 4 * D + col, c0, D, e, 0.0f);
#pragma unroll
            for (int j = 0; j < 4; ++j) g[k][j] += e[j];
        }
        if (bin >= 0) {                                                         // calibrate backward
            float sc[4];
            pt_load4<VEC>(scale, (size_t)bin * 4 * D + col, c0, D, sc, -1.0f);
#pragma unroll
            for (int j = 0; j < 4; ++j) g[k][j] = sc[j] < 0.0f ? g[k][j] : g[k][j] * sc[j];
        }
    }
    float u[4], v[4], gd[4];
    int arg[4];
    pt_load4<VEC>(uv, (size_t)b * 2 * D + c0, c0, D, u, 0.0f);
    pt_load4<VEC>(uv, (size_t)b * 2 * D + D + c0, c0, D, v, 0.0f);
    pt_load4<VEC>(second ? arg2 : arg1, (size_t)b * D + c0, c0, D, arg, -1);
    const DirDropout& dr = second ? d2 : d1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float sg = (float)((u[j] > v[j]) - (u[j] < v[j]));               // sign(u - v), sign(0) = 0
        gd[j] = second ? (g[1][j] - sg * g[2][j]) + g[3][j] * u[j]              // dv
                       : (g[0][j] + sg * g[2][j]) + g[3][j] * v[j];             // du
        if constexpr (DROP) {
            if (arg[j] >= 0) {                                                  // the keep factor of the one element that was the maximum
                const uint64_t e = ((uint64_t)b * (uint64_t)T + (uint64_t)arg[j]) * (uint64_t)D + (uint64_t)(c0 + j);
                gd[j] = dir_dropout_apply(dr, pt_pick(dir_dropout_bits(dr, e >> 2), (uint32_t)e & 3u), gd[j]);
            }
        }
    }
    const size_t row0 = (size_t)b * T;
    for (int t = 0; t < T; ++t) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (t == arg[j]) ? gd[j] : 0.0f;
        pt_store4<VEC>(ds, (row0 + t) * D + c0, c0, D, o);
    }
}

// partial[slice][k] = sum over the rows of the slice (in order) of dlogits[b] * emb[b, k]
__global__ void __launch_bounds__(DIR_TPB)
pair_bwd_dw_partial_kernel(const float* __restrict__ dlogits, const float* __restrict__ emb, int B, int K, int rows_per_slice,
                           float* __restrict__ partial) {
    const int k = blockIdx.x * DIR_TPB + threadIdx.x;
    if (k >= K) return;
    const int b0 = blockIdx.y * rows_per_slice;
    const int b1 = (b0 + rows_per_slice < B) ? b0 + rows_per_slice : B;
    float s = 0.0f;
    for (int b = b0; b < b1; ++b) s += dlogits[b] * emb[(size_t)b * K + k];
    partial[(size_t)blockIdx.y * K + k] = s;
}

__global__ void __launch_bounds__(DIR_TPB)
pair_bwd_dw_final_kernel(const float* __restrict__ partial, int slices, const float* __restrict__ dlogits, int B, int K,
                         float* __restrict__ dweight, float* __restrict__ dbias) {
    __shared__ float red[DIR_TPB];
    const int t = threadIdx.x;
    const int k = blockIdx.x * DIR_TPB + t;
    if (k < K) {
        float s = partial[k];
        for (int z = 1; z < slices; ++z) s += partial[(size_t)z * K + k];       // fixed order: bit-reproducible
        dweight[k] = s;
    }
    if (blockIdx.x == 0 && dbias) {
        float s = 0.0f;
        for (int b = t; b < B; b += DIR_TPB) s += dlogits[b];
        red[t] = s;
        __syncthreads();
        for (int o = DIR_TPB / 2; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
        if (t == 0) dbias[0] = red[0];
    }
}

int pair_slices(int B, int* rows_per_slice) {                 // the batch slices of the dweight reduction (as dir_tail_bwd)
    int rps = (B + 31) / 32; if (rps < 8) rps = 8;
    *rows_per_slice = rps;
    return (B + rps - 1) / rps;
}

bool pair_p_ok(double p) { return p >= 0.0 && p <= 1.0; }                      // (false for NaN)

// element counts stay below 2^31 (the Python side sizes int32 argmax maps and the grids with them)
bool pair_too_large(int B, int T1, int T2, int D) {
    const long long lim = 1ll << 31;
    const long long t = T1 > T2 ? T1 : T2;
    return (long long)B * t * D >= lim || (long long)B * 4 * D >= lim;
}

bool pair_all_aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps) if (!dir_aligned16(p)) return false;             // (NULL passes)
    return true;
}

}  // namespace

extern "C" size_t dir_pair_tail_workspace(int B, int D) {
    if (B <= 0 || D <= 0 || (long long)B * 4 * D >= (1ll << 31)) return 0;
    int rps;
    const size_t fwd = (size_t)dir_cdiv(D, PT_FWD_TILE) * B, bwd = (size_t)pair_slices(B, &rps) * 4 * D;
    return dir_align_up((fwd > bwd ? fwd : bwd) * sizeof(float), 256);
}

extern "C" int dir_pair_tail_fwd(const float* s1, const float* s2, const uint8_t* mask1, const uint8_t* mask2, int B, int T1, int T2,
                                 int D, const int32_t* bins, int nb, const float* m1, const float* scale, const float* m2,
                                 const float* weight, const float* bias, uint64_t seed, uint64_t offset1, uint64_t offset2, double p,
                                 float* emb, float* uv, int32_t* arg1, int32_t* arg2, float* logits, void* workspace,
                                 size_t workspace_bytes, dir_stream_t stream) {
    DIR_RETURN_IF(B <= 0 || T1 <= 0 || T2 <= 0 || D <= 0 || !pair_p_ok(p), DIR_EINVAL);
    DIR_RETURN_IF(!s1 || !s2 || !mask1 || !mask2 || !weight || !bias || !emb || !uv || !arg1 || !arg2 || !logits, DIR_EINVAL);
    const bool calibrate = bins || m1 || scale || m2;
    DIR_RETURN_IF(calibrate && (!bins || !m1 || !scale || !m2 || nb <= 0), DIR_EINVAL);
    DIR_RETURN_IF(dir_misaligned(s1, 4) || dir_misaligned(s2, 4) || dir_misaligned(emb, 4) || dir_misaligned(uv, 4), DIR_EINVAL);
    DIR_RETURN_IF(pair_too_large(B, T1, T2, D) || B > 65535, DIR_EUNSUPPORTED);
    DIR_RETURN_IF(!workspace || workspace_bytes < dir_pair_tail_workspace(B, D), DIR_EWORKSPACE);
    const int tiles = dir_cdiv(D, PT_FWD_TILE);
    const bool vec = D % 4 == 0 && pair_all_aligned16({s1, s2, m1, scale, m2, weight, emb, uv, arg1, arg2});
    const bool drop = p != 0.0;                                                // p == 0: the kernels without dropout, bit for bit
    const DirDropout d1 = dir_dropout_params(seed, offset1, p), d2 = dir_dropout_params(seed, offset2, p);
    float* partial = static_cast<float*>(workspace);
    const dim3 grid(tiles, B), block(DIR_TPB);
#define PAIR_FWD(V, P) hipLaunchKernelGGL((pair_fwd_kernel<V, P>), grid, block, 0, dir_s(stream), s1, s2, mask1, mask2, B, T1, T2, D, \
                                          bins, nb, m1, scale, m2, weight, d1, d2, emb, uv, arg1, arg2, partial)
    if (vec) { if (drop) PAIR_FWD(true, true); else PAIR_FWD(true, false); }
    else     { if (drop) PAIR_FWD(false, true); else PAIR_FWD(false, false); }
#undef PAIR_FWD
    DIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(pair_fwd_fold_kernel, dim3(dir_cdiv(B, DIR_TPB)), block, 0, dir_s(stream), partial, tiles, B, bias, logits);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}

extern "C" int dir_pair_tail_bwd(const float* dlogits, const float* demb, const int32_t* bins, int nb, const float* scale,
                                 const float* weight, const float* emb, const float* uv, const int32_t* arg1, const int32_t* arg2,
                                 int B, int T1, int T2, int D, uint64_t seed, uint64_t offset1, uint64_t offset2, double p,
                                 float* ds1, float* ds2, float* dweight, float* dbias, void* workspace, size_t workspace_bytes,
                                 dir_stream_t stream) {
    DIR_RETURN_IF(B <= 0 || T1 <= 0 || T2 <= 0 || D <= 0 || !pair_p_ok(p), DIR_EINVAL);
    DIR_RETURN_IF(!dlogits || !weight, DIR_EINVAL);
    DIR_RETURN_IF((bins != nullptr) != (scale != nullptr) || (bins && nb <= 0), DIR_EINVAL);
    DIR_RETURN_IF((ds1 || ds2) && (!uv || !arg1 || !arg2), DIR_EINVAL);
    DIR_RETURN_IF(dweight && !emb, DIR_EINVAL);
    DIR_RETURN_IF(dir_misaligned(ds1, 4) || dir_misaligned(ds2, 4) || dir_misaligned(demb, 4) || dir_misaligned(uv, 4), DIR_EINVAL);
    DIR_RETURN_IF(pair_too_large(B, T1, T2, D) || B > 65535, DIR_EUNSUPPORTED);
    DIR_RETURN_IF(dweight && (!workspace || workspace_bytes < dir_pair_tail_workspace(B, D)), DIR_EWORKSPACE);
    if (ds1 || ds2) {
        const bool vec = D % 4 == 0 && pair_all_aligned16({demb, scale, weight, uv, arg1, arg2, ds1, ds2});
        const bool drop = p != 0.0;
        const DirDropout d1 = dir_dropout_params(seed, offset1, p), d2 = dir_dropout_params(seed, offset2, p);
        const dim3 grid(dir_cdiv(D, PT_TILE), B, 2), block(DIR_TPB);
#define PAIR_BWD(V, P) hipLaunchKernelGGL((pair_bwd_ds_kernel<V, P>), grid, block, 0, dir_s(stream), dlogits, demb, bins, nb, scale, \
                                          weight, uv, arg1, arg2, T1, T2, D, d1, d2, ds1, ds2)
        if (vec) { if (drop) PAIR_BWD(true, true); else PAIR_BWD(true, false); }
        else     { if (drop) PAIR_BWD(false, true); else PAIR_BWD(false, false); }
#undef PAIR_BWD
        DIR_LAUNCH_CHECK();
    }
    if (dweight) {
        int rps;
        const int slices = pair_slices(B, &rps), K = 4 * D;
        float* partial = static_cast<float*>(workspace);
        hipLaunchKernelGGL(pair_bwd_dw_partial_kernel, dim3(dir_cdiv(K, DIR_TPB), slices), dim3(DIR_TPB), 0, dir_s(stream), dlogits, emb,
                           B, K, rps, partial);
        DIR_LAUNCH_CHECK();
        hipLaunchKernelGGL(pair_bwd_dw_final_kernel, dim3(dir_cdiv(K, DIR_TPB)), dim3(DIR_TPB), 0, dir_s(stream), partial, slices,
                           dlogits, B, K, dweight, dbias);
        DIR_LAUNCH_CHECK();
    }
    return DIR_OK;
}
