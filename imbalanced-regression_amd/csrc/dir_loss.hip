// Weighted regression losses, forward value + gradient in one launch (gfx950).
// Replaces imbdb-wiki-dir/loss.py:5-48 and the autograd graph torch builds for them
// (3-6 tiny kernels forward, as many backward, for n = batch size elements).
#include "dir_common.h"

#define LOSS_SINGLE_MAX (DIR_TPB * 64)      // <= 16384 elements: one workgroup, one launch

struct LossArgs { int kind; float beta, gamma; int activate; };

// per-element value (float32, op order of loss.py) and d value / d x (float32)
__device__ __forceinline__ void loss_elem(const LossArgs a, float x, float y, float w, bool has_w,
                                          float& val, float& grad) {
    const float d = x - y;
    const float ad = fabsf(d);
    const float sgn = (d > 0.0f) ? 1.0f : ((d < 0.0f) ? -1.0f : 0.0f);   // torch sign(0) = 0
    float v, g;
    switch (a.kind) {
    case DIR_LOSS_MSE:                                   // loss.py:5-10
        v = d * d; g = 2.0f * d; break;
    case DIR_LOSS_L1:                                    // loss.py:13-18
        v = ad; g = sgn; break;
    case DIR_LOSS_FOCAL_MSE:
    case DIR_LOSS_FOCAL_L1: {                            // loss.py:21-38
        const float z = a.beta * ad;
        float act, dact;                                 // activation and d act / d |d|
        if (a.activate == 1) { act = tanhf(z); dact = (1.0f - act * act) * a.beta; }
        else { const float s = 1.0f / (1.0f + expf(-z)); act = 2.0f * s - 1.0f; dact = 2.0f * s * (1.0f - s) * a.beta; }
        const float base = (a.kind == DIR_LOSS_FOCAL_MSE) ? d * d : ad;
        const float dbase = (a.kind == DIR_LOSS_FOCAL_MSE) ? 2.0f * d : sgn;
        float pw, dpw;                                   // act^gamma and gamma*act^(gamma-1)
        if (a.gamma == 1.0f) { pw = act; dpw = 1.0f; }
        else { pw = powf(act, a.gamma); dpw = a.gamma * powf(act, a.gamma - 1.0f); }
        v = base * pw;
        g = dbase * pw + base * dpw * dact * sgn;
        break; }
    default: {                                           // DIR_LOSS_HUBER, loss.py:41-48
        const bool quad = ad < a.beta;
        v = quad ? (0.5f * (ad * ad)) / a.beta : ad - 0.5f * a.beta;
        g = quad ? d / a.beta : sgn;
        break; }
    }
    if (has_w) { v = v * w; g = g * w; }
    val = v; grad = g;
}

// One workgroup: whole loss in one launch (the training-batch case, n = B).
__global__ void __launch_bounds__(DIR_TPB)
loss_single_kernel(LossArgs a, const float* __restrict__ x, const float* __restrict__ y,
                   const float* __restrict__ w, int n, float* __restrict__ loss, float* __restrict__ dx) {
    __shared__ double sh[DIR_TPB / DIR_WAVE];
    const float inv_n = 1.0f / (float)n;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += DIR_TPB) {
        float v, g;
        loss_elem(a, x[i], y[i], w ? w[i] : 1.0f, w != nullptr, v, g);
        acc += (double)v;
        if (dx) dx[i] = g * inv_n;
    }
    const double tot = dir_block_sum(acc, sh);
    if (threadIdx.x == 0) loss[0] = (float)(tot / (double)n);
}

// Large n (dense per-pixel targets): partial sums per workgroup, then a fixed-order final sum.
__global__ void __launch_bounds__(DIR_TPB)
loss_partial_kernel(LossArgs a, const float* __restrict__ x, const float* __restrict__ y,
                    const float* __restrict__ w, int n, double* __restrict__ partial, float* __restrict__ dx) {
    __shared__ double sh[DIR_TPB / DIR_WAVE];
    const float inv_n = 1.0f / (float)n;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * DIR_TPB + threadIdx.x; i < n; i += (long long)gridDim.x * DIR_TPB) {
        float v, g;
        loss_elem(a, x[i], y[i], w ? w[i] : 1.0f, w != nullptr, v, g);
        acc += (double)v;
        if (dx) dx[i] = g * inv_n;
    }
    const double tot = dir_block_sum(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(DIR_TPB)
loss_final_kernel(const double* __restrict__ partial, int nparts, int n, float* __restrict__ loss) {
    __shared__ double sh[DIR_TPB / DIR_WAVE];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += DIR_TPB) acc += partial[i];
    const double tot = dir_block_sum(acc, sh);
    if (threadIdx.x == 0) loss[0] = (float)(tot / (double)n);
}

static int loss_parts(int n) {
    int g = dir_cdiv(n, DIR_TPB * 8);
    return g > 2048 ? 2048 : g;
}

extern "C" size_t dir_weighted_loss_workspace(int n) {
    if (n <= LOSS_SINGLE_MAX) return 0;
    return dir_align_up(sizeof(double) * (size_t)loss_parts(n), 256);
}

extern "C" int dir_weighted_loss(int kind, const float* x, const float* y, const float* w, int n,
                                 float beta, float gamma, int activate,
                                 float* loss, float* dx_unit, void* workspace, size_t workspace_bytes,
                                 dir_stream_t stream) {
    DIR_RETURN_IF(kind < DIR_LOSS_MSE || kind > DIR_LOSS_HUBER, DIR_EINVAL);
    DIR_RETURN_IF(!x || !y || !loss || n <= 0, DIR_EINVAL);
    DIR_RETURN_IF(activate != 0 && activate != 1, DIR_EINVAL);
    LossArgs a{kind, beta, gamma, activate};
    if (n <= LOSS_SINGLE_MAX) {
        hipLaunchKernelGGL(loss_single_kernel, dim3(1), dim3(DIR_TPB), 0, dir_s(stream), a, x, y, w, n, loss, dx_unit);
        DIR_LAUNCH_CHECK();
        return DIR_OK;
    }
    const int parts = loss_parts(n);
    DIR_RETURN_IF(!workspace || workspace_bytes < sizeof(double) * (size_t)parts, DIR_EWORKSPACE);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(loss_partial_kernel, dim3(parts), dim3(DIR_TPB), 0, dir_s(stream), a, x, y, w, n, partial, dx_unit);
    DIR_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(DIR_TPB), 0, dir_s(stream), partial, parts, n, loss);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}

__global__ void __launch_bounds__(DIR_TPB)
scale_by_scalar_kernel(const float* __restrict__ in, const float* __restrict__ scalar, float* __restrict__ out, int n) {
    const float s = *scalar;
    for (long long i = (long long)blockIdx.x * DIR_TPB + threadIdx.x; i < n; i += (long long)gridDim.x * DIR_TPB)
        out[i] = in[i] * s;
}

extern "C" int dir_scale_by_device_scalar(const float* in, const float* scalar, float* out, int n, dir_stream_t stream) {
    DIR_RETURN_IF(!in || !scalar || !out || n < 0, DIR_EINVAL);
    if (n == 0) return DIR_OK;
    int grid = dir_cdiv(n, DIR_TPB); if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(scale_by_scalar_kernel, dim3(grid), dim3(DIR_TPB), 0, dir_s(stream), in, scalar, out, n);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}
