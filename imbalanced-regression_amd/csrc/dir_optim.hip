// Optimizer steps and weight preparation of the convolution layers for MI355X / gfx950 (CDNA4).
//
// dir_adam_step / dir_sgd_step: torch.optim.Adam / SGD for EVERY parameter tensor of the network in one launch each, fused with the
// weight preparation below for the rows that are convolution weights. dir_conv_prep_weights*: the float32 master weight
// [Cout][R][S][Cin] -> the bf16 operands the MFMA convolution kernels (dir_conv.hip, dir_conv_wgrad*.hip) consume.
#include <cmath>
#include "dir_common.h"
#include "dir_conv_shared.h"

// ---------------------------------------------------------------------------------------------------------------
// Weight preparation: one launch per conv layer and optimizer step turns the float32 master weight
// [Cout][R][S][Cin] into the two bf16 operands the MFMA kernels consume — w16 (same layout, forward / wgrad shape)
// and, optionally, w16_rot [Cin][R][S][Cout] with the taps rotated by 180 degrees (the data-gradient convolution's
// weight) — instead of a cast + flip + permute + copy chain of library kernels.
namespace {
// One layer: w [Cout][RS][Cin] f32 -> w16 (same layout, bf16) and optionally w16_rot [Cin][RS][Cout] with the taps
// reversed. Cin, Cout % 64 == 0: the (co, ci) transpose of each tap goes through a 64x64 LDS tile, so both the float
// reads (256 B rows) and the two bf16 writes (128 B rows) are coalesced. Tiles are strided over gridDim.x.
// rot_mode 0: w16_rot = [Cin][R][S][Cout] with the taps rotated by 180 degrees (stride-1 data gradient).
// rot_mode 1 (3x3 only): w16_rot = the four parity-class weights of the STRIDE-2 data gradient, packed back to back:
//   class (a, b) = (r != 1, s != 1) holds the (1 + a) x (1 + b) taps that reach output pixels (2 i + a, 2 j + b), as
//   [Cin][(1 + a)(1 + b)][Cout] with tap (dr, ds) = (r == 0, s == 0) (dY row i + dr, column j + ds); class bases at
//   0, 1, 3, 5 taps.
__device__ __forceinline__ size_t conv_prep_rot_index(int rot_mode, int ci, int tap, int co, int RS, int Cin, int Cout) {
    if (rot_mode == 0) return ((size_t)ci * RS + (RS - 1 - tap)) * Cout + co;
    const int r = tap / 3, s = tap - 3 * r;
    const int a = r != 1, b = s != 1, dr = r == 0, ds = s == 0;
    const int taps = (1 + a) * (1 + b), t = dr * (1 + b) + ds;
    const int base = a ? (b ? 5 : 3) : (b ? 1 : 0);
    return (size_t)base * Cin * Cout + ((size_t)ci * taps + t) * Cout + co;
}

// Adam (torch.optim.Adam's single-tensor arithmetic, no amsgrad): one element; returns the new parameter value
struct AdamH { float step_size, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay, bias_correction2_sqrt; };   // (host: float64, then rounded, like torch's Python scalars)
__device__ __forceinline__ float adam_update(float p, float g, float* __restrict__ m, float* __restrict__ v, size_t i, const AdamH& h) {
    if (h.weight_decay != 0.0f) g = g + h.weight_decay * p;                      // grad.add(param, alpha=weight_decay)
    const float m0 = m[i], v0 = v[i];
    const float m1 = m0 + h.one_minus_beta1 * (g - m0);                           // exp_avg.lerp_(grad, 1 - beta1)
    const float v1 = v0 * h.beta2 + h.one_minus_beta2 * (g * g);                  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    m[i] = m1; v[i] = v1;
    const float denom = sqrtf(v1) / h.bias_correction2_sqrt + h.eps;              // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
    return p - h.step_size * (m1 / denom);                                        // param.addcdiv_(exp_avg, denom, value=-step_size), step_size = lr / bias_correction1
}

// torch.optim.SGD's single-tensor arithmetic (sgd.py: _single_tensor_sgd), one element; returns the new parameter value. The `add(x, alpha=a)`
// steps are written as fmaf, which is how torch's element-wise kernels evaluate `a + alpha * b`.
struct SgdH { float lr, momentum, one_minus_dampening, weight_decay; int nesterov, first; };
__device__ __forceinline__ float sgd_update(float p, float g, float* __restrict__ buf, size_t i, const SgdH& h) {
    if (h.weight_decay != 0.0f) g = __fmaf_rn(h.weight_decay, p, g);                 // grad = grad.add(param, alpha=weight_decay)
    if (h.momentum != 0.0f) {
        const float b = h.first ? g : __fmaf_rn(h.one_minus_dampening, g, buf[i] * h.momentum);   // buf = clone(grad) | buf.mul_(momentum).add_(grad, alpha=1 - dampening)
        buf[i] = b;
        g = h.nesterov ? __fmaf_rn(h.momentum, b, g) : b;                             // grad = grad.add(buf, alpha=momentum) | buf
    }
    return __fmaf_rn(-h.lr, g, p);                                                    // param.add_(grad, alpha=-lr)
}
// what the weight preparation pass does to the master weight first: nothing, an Adam step, an SGD step
struct OptNone { __device__ __forceinline__ float operator()(float w, size_t) const { return w; } static constexpr bool UPDATES = false; };
struct OptAdam { const float* g; float* m; float* v; AdamH h; static constexpr bool UPDATES = true;
                 __device__ __forceinline__ float operator()(float w, size_t i) const { return adam_update(w, g[i], m, v, i, h); } };
struct OptSgd { const float* g; float* buf; SgdH h; static constexpr bool UPDATES = true;
                __device__ __forceinline__ float operator()(float w, size_t i) const { return sgd_update(w, g[i], buf, i, h); } };

// OPT::UPDATES: w is first UPDATED in place from (g, m, v) — the optimizer step — and the bf16 operands are made from the new value in the
// same pass (dir_adam_step): one read of the master weight for the optimizer and the two layout conversions together.
template <typename OPT = OptNone>
__device__ __forceinline__ void conv_prep_body(float* __restrict__ w, int Cout, int RS, int Cin,
                                               uint16_t* __restrict__ w16, uint16_t* __restrict__ w16_rot, int rot_mode,
                                               const OPT opt = OPT{}) {
    __shared__ uint16_t tile[64][66];
    const int t = threadIdx.x, tx = t & 63, ty = t >> 6;           // 4 rows of 64 per pass
    if ((Cout & 63) || (Cin & 63)) {                               // generic fallback (not used by ResNet-50's layers)
        const size_t n = (size_t)Cout * RS * Cin;
        for (size_t i = (size_t)blockIdx.x * DIR_TPB + t; i < n; i += (size_t)gridDim.x * DIR_TPB) {
            float wv = w[i];
            if (OPT::UPDATES) { wv = opt(wv, i); w[i] = wv; }
            const uint16_t h = (uint16_t)cv_f2bf(wv);
            w16[i] = h;
            if (w16_rot) {
                const int ci = (int)(i % Cin); const size_t t1 = i / Cin; const int tap = (int)(t1 % RS); const int co = (int)(t1 / RS);
                w16_rot[conv_prep_rot_index(rot_mode, ci, tap, co, RS, Cin, Cout)] = h;
            }
        }
        return;
    }
    const int tci = Cin >> 6, tco = Cout >> 6, ntiles = tci * tco * RS;
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int ci0 = (tl % tci) << 6; const int t1 = tl / tci; const int tap = t1 % RS; const int co0 = (t1 / RS) << 6;
#pragma unroll 4
        for (int r = ty; r < 64; r += 4) {                         // row = output channel, 64 consecutive input channels
            const size_t i = ((size_t)(co0 + r) * RS + tap) * Cin + ci0 + tx;
            float wv = w[i];
            if (OPT::UPDATES) { wv = opt(wv, i); w[i] = wv; }
            const uint16_t hb = (uint16_t)cv_f2bf(wv);
            w16[i] = hb;
            tile[r][tx] = hb;
        }
        if (w16_rot) {
            __syncthreads();
#pragma unroll 4
            for (int r = ty; r < 64; r += 4)                       // row = input channel, 64 consecutive output channels
                w16_rot[conv_prep_rot_index(rot_mode, ci0 + r, tap, co0 + tx, RS, Cin, Cout)] = tile[tx][r];
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(DIR_TPB)
conv_prep_weights_kernel(const float* __restrict__ w, int Cout, int RS, int Cin, uint16_t* __restrict__ w16,
                         uint16_t* __restrict__ w16_rot, int rot_mode) {
    conv_prep_body(const_cast<float*>(w), Cout, RS, Cin, w16, w16_rot, rot_mode);
}

// blockIdx.y = layer; the layer's row of the table holds its pointers and extents
__global__ void __launch_bounds__(DIR_TPB)
conv_prep_weights_batched_kernel(const long long* __restrict__ table) {
    const long long* e = table + (size_t)blockIdx.y * 7;
    conv_prep_body(reinterpret_cast<float*>(e[0]), (int)e[3], (int)e[4], (int)e[5],
                   reinterpret_cast<uint16_t*>(e[1]), reinterpret_cast<uint16_t*>(e[2]), (int)e[6]);
}

// One Adam step for EVERY parameter tensor of the network in one launch (blockIdx.y = tensor; row of the table = 12 int64:
// param, grad, exp_avg, exp_avg_sq, numel, w16, w16_rot, Cout, RS, Cin, rot_mode, 0). Rows with w16 != 0 are convolution weights:
// their bf16 operands for the next forward / data gradient are rewritten from the updated value in the same pass.
__global__ void __launch_bounds__(DIR_TPB)
adam_step_kernel(const long long* __restrict__ table, AdamH h) {
    const long long* e = table + (size_t)blockIdx.y * 12;
    float* w = reinterpret_cast<float*>(e[0]);
    const float* g = reinterpret_cast<const float*>(e[1]);
    float* m = reinterpret_cast<float*>(e[2]);
    float* v = reinterpret_cast<float*>(e[3]);
    if (e[5]) {
        conv_prep_body<OptAdam>(w, (int)e[7], (int)e[8], (int)e[9], reinterpret_cast<uint16_t*>(e[5]), reinterpret_cast<uint16_t*>(e[6]), (int)e[10], OptAdam{g, m, v, h});
        return;
    }
    const size_t n = (size_t)e[4];
    for (size_t i = (size_t)blockIdx.x * DIR_TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * DIR_TPB)
        w[i] = adam_update(w[i], g[i], m, v, i, h);
}

// The same launch shape for torch.optim.SGD (rows: param, grad, momentum_buffer (0 = no momentum), 0, numel, w16, w16_rot, Cout, RS, Cin, rot_mode, 0)
__global__ void __launch_bounds__(DIR_TPB)
sgd_step_kernel(const long long* __restrict__ table, SgdH h) {
    const long long* e = table + (size_t)blockIdx.y * 12;
    float* w = reinterpret_cast<float*>(e[0]);
    const float* g = reinterpret_cast<const float*>(e[1]);
    float* buf = reinterpret_cast<float*>(e[2]);
    if (e[5]) {
        conv_prep_body<OptSgd>(w, (int)e[7], (int)e[8], (int)e[9], reinterpret_cast<uint16_t*>(e[5]), reinterpret_cast<uint16_t*>(e[6]), (int)e[10], OptSgd{g, buf, h});
        return;
    }
    const size_t n = (size_t)e[4];
    for (size_t i = (size_t)blockIdx.x * DIR_TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * DIR_TPB)
        w[i] = sgd_update(w[i], g[i], buf, i, h);
}
}  // namespace

// torch.optim.SGD.step() (train.py:163-164 builds it for --optimizer sgd) for all parameters in ONE launch, fused with the bf16 weight
// preparation like dir_adam_step. table: device [ntensors][12] int64 (see sgd_step_kernel). first != 0: the momentum buffers do not
// hold a value yet (torch creates them as clone(grad) at the first step); momentum == 0: no buffer is touched (entries may be 0).
extern "C" int dir_sgd_step(const void* table, int ntensors, double lr, double momentum, double dampening, double weight_decay, int nesterov,
                            int first, dir_stream_t stream) {
    DIR_RETURN_IF(!table || ntensors <= 0 || ntensors > 65535, DIR_EINVAL);
    DIR_RETURN_IF(nesterov && (momentum <= 0.0 || dampening != 0.0), DIR_EINVAL);       // torch: "Nesterov momentum requires a momentum and zero dampening"
    SgdH h;
    h.lr = (float)lr; h.momentum = (float)momentum; h.one_minus_dampening = (float)(1.0 - dampening); h.weight_decay = (float)weight_decay;
    h.nesterov = nesterov ? 1 : 0; h.first = first ? 1 : 0;
    hipLaunchKernelGGL(sgd_step_kernel, dim3(128, ntensors), dim3(DIR_TPB), 0, dir_s(stream), static_cast<const long long*>(table), h);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}

// torch.optim.Adam.step() (train.py:161-162 builds the optimizer, :259-260 steps it) for all parameters in ONE launch, fused with
// the bf16 weight preparation of the convolution layers (dir_conv_prep_weights_batched). table: device [ntensors][12] int64 (see
// adam_step_kernel); step >= 1 is the step count AFTER the increment (bias corrections 1 - beta^step, computed on the host in
// float64 like torch's non-capturable path). float32 parameters, gradients and state, all dense.
extern "C" int dir_adam_step(const void* table, int ntensors, double lr, double beta1, double beta2, double eps, double weight_decay,
                             long long step, dir_stream_t stream) {
    DIR_RETURN_IF(!table || ntensors <= 0 || ntensors > 65535 || step < 1, DIR_EINVAL);
    AdamH h;
    h.beta2 = (float)beta2; h.one_minus_beta1 = (float)(1.0 - beta1); h.one_minus_beta2 = (float)(1.0 - beta2);
    h.eps = (float)eps; h.weight_decay = (float)weight_decay;
    h.step_size = (float)(lr / (1.0 - pow(beta1, (double)step)));
    h.bias_correction2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step));
    hipLaunchKernelGGL(adam_step_kernel, dim3(128, ntensors), dim3(DIR_TPB), 0, dir_s(stream), static_cast<const long long*>(table), h);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}

extern "C" int dir_conv_prep_weights_batched(const void* table, int nlayers, dir_stream_t stream) {
    DIR_RETURN_IF(!table || nlayers <= 0 || nlayers > 65535, DIR_EINVAL);
    hipLaunchKernelGGL(conv_prep_weights_batched_kernel, dim3(128, nlayers), dim3(DIR_TPB), 0, dir_s(stream),
                       static_cast<const long long*>(table));
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}

extern "C" int dir_conv_prep_weights_ex(const float* w, int Cout, int R, int S, int Cin, void* w16, void* w16_rot,
                                        int rot_mode, dir_stream_t stream);
extern "C" int dir_conv_prep_weights(const float* w, int Cout, int R, int S, int Cin, void* w16, void* w16_rot,
                                     dir_stream_t stream) {
    return dir_conv_prep_weights_ex(w, Cout, R, S, Cin, w16, w16_rot, 0, stream);
}

extern "C" int dir_conv_prep_weights_ex(const float* w, int Cout, int R, int S, int Cin, void* w16, void* w16_rot,
                                        int rot_mode, dir_stream_t stream) {
    DIR_RETURN_IF(!w || !w16 || Cout <= 0 || R <= 0 || S <= 0 || Cin <= 0, DIR_EINVAL);
    DIR_RETURN_IF(rot_mode < 0 || rot_mode > 1 || (rot_mode == 1 && (R != 3 || S != 3)), DIR_EINVAL);
    const size_t n = (size_t)Cout * R * S * Cin;
    int grid = dir_cdiv((long long)n, DIR_TPB); if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(conv_prep_weights_kernel, dim3(grid), dim3(DIR_TPB), 0, dir_s(stream), w, Cout, R * S, Cin,
                       static_cast<uint16_t*>(w16), static_cast<uint16_t*>(w16_rot), rot_mode);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}
