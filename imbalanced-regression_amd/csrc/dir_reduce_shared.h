// Shared pieces of the streaming reductions (dir_eval.hip, dir_eval_age.hip, dir_loss_nyud2.hip): the 16-byte quad grid and the
// wave-private LDS tables with their fold. What each kernel does per sample, and in which order it adds, stays in its own file.
#pragma once
#include "dir_common.h"

// ---- the quad grid ------------------------------------------------------------------------------------------------------------------
// Quad q covers elements 4q - off .. 4q - off + 3 of every operand, off = the anchor operand's distance (in elements) from the
// 16-byte boundary below it: up to 3 slots of lead-in before element 0, a partial quad at the tail. Full quads of the anchor are
// 16-byte aligned by construction; another float operand is when it sits at the same offset, a byte mask when mask - off is
// 4-byte aligned. Edge quads, and full quads of an operand at another offset, go element by element.
static inline int dir_quad_grid(long long n, int max_blocks) {
    const long long quads = (n + 3 + 3) / 4;
    long long g = (quads + DIR_TPB - 1) / DIR_TPB;
    if (g > max_blocks) g = max_blocks;
    return g < 1 ? 1 : (int)g;
}
static inline int dir_quad_offset(const float* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3u); }
static inline bool dir_quad_same_offset(const float* p, int off) { return dir_quad_offset(p) == off; }
static inline bool dir_quad_mask_aligned(const uint8_t* mask, int off) {
    return mask && ((reinterpret_cast<uintptr_t>(mask) - (uintptr_t)off) & 3u) == 0;
}

// I = index type: int where the entry point bounds n (2.1e9, so that 4 * quad of the last round fits), long long otherwise
template <typename I>
struct DirQuad {
    I i0;                                     // first element: may be < 0 (lead-in) or reach past n (tail)
    bool inside;                              // q < quads (whole waves stay in their loop for the shuffles)
    bool full;                                // all four elements exist
};

template <typename I>
__device__ __forceinline__ DirQuad<I> dir_quad(I q, I quads, int off, I n) {
    DirQuad<I> d;
    d.i0 = 4 * q - off;
    d.inside = q < quads;
    d.full = d.inside && d.i0 >= 0 && d.i0 + 3 < n;
    return d;
}

// in[j]: element i0 + j exists
template <typename I>
__device__ __forceinline__ void dir_quad_in(const DirQuad<I>& d, I n, bool in[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) in[j] = d.full || (d.inside && d.i0 + j >= 0 && d.i0 + j < n);
}

// four floats: one float4 when the quad is full and the operand is at the anchor's offset (vec), else v[j] = pr[j] ? p[i0 + j] : fill
template <typename I>
__device__ __forceinline__ void dir_quad_load(const float* __restrict__ p, const DirQuad<I>& d, bool vec, const bool pr[4], float fill,
                                              float v[4]) {
    if (d.full && vec) {
        const float4 t = *reinterpret_cast<const float4*>(p + d.i0);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = pr[j] ? p[d.i0 + j] : fill;
    }
}

// four keep flags: in[j] and, with a mask, a non-zero mask byte (one uint32_t load when the quad is full and the mask aligned)
template <typename I>
__device__ __forceinline__ void dir_quad_keep(const uint8_t* __restrict__ mask, const DirQuad<I>& d, bool vec, const bool in[4],
                                              bool keep[4]) {
    if (mask && d.full && vec) {
        const uint32_t mv = *reinterpret_cast<const uint32_t*>(mask + d.i0);
#pragma unroll
        for (int j = 0; j < 4; ++j) keep[j] = ((mv >> (8 * j)) & 0xffu) != 0;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) keep[j] = in[j] && (!mask || mask[d.i0 + j] != 0);
    }
}

// ---- wave-private LDS tables ----------------------------------------------------------------------------------------------------------
// [DIR_TPB / DIR_WAVE waves][rows] slots in dynamic LDS, each wave adding to its own in program order (no atomics). Counts are
// uint32_t in LDS and exact in float64. The workgroup's partial is [rows][NS + NC] float64, sums before counts.
template <int NS, int NC>
struct DirSlot {
    double s[NS];
    uint32_t c[NC];
};

// the caller puts a barrier after this
template <int NS, int NC>
__device__ __forceinline__ void dir_slots_zero(DirSlot<NS, NC>* tabs, int rows) {
    uint32_t* w = reinterpret_cast<uint32_t*>(tabs);
    for (int i = threadIdx.x; i < (DIR_TPB / DIR_WAVE) * rows * (int)(sizeof(DirSlot<NS, NC>) / 4); i += DIR_TPB) w[i] = 0u;
}

// after a barrier: the wave tables added in wave order -> out [rows][NS + NC]
template <int NS, int NC>
__device__ __forceinline__ void dir_slots_write(const DirSlot<NS, NC>* tabs, int rows, double* __restrict__ out) {
    constexpr int COLS = NS + NC;
    for (int i = threadIdx.x; i < rows * COLS; i += DIR_TPB) {
        const int r = i / COLS, col = i - r * COLS;
        double v = 0.0;
#pragma unroll
        for (int wv = 0; wv < DIR_TPB / DIR_WAVE; ++wv) {
            const DirSlot<NS, NC>& s = tabs[wv * rows + r];
            v += col < NS ? s.s[col] : (double)s.c[col - NS];
        }
        out[i] = v;
    }
}

// partials [blocks][entries] added in block order onto the caller's table (a template so that a file that includes this header and
// never folds gets no copy of the kernel)
template <typename T>
static __global__ void __launch_bounds__(DIR_TPB)
dir_table_fold_kernel(const T* __restrict__ partials, int blocks, int entries, T* __restrict__ table) {
    const int i = blockIdx.x * DIR_TPB + threadIdx.x;
    if (i >= entries) return;
    T v = 0;
#pragma unroll 8
    for (int g = 0; g < blocks; ++g) v += partials[(size_t)g * entries + i];
    table[i] += v;
}

template <typename T>
static inline int dir_table_fold(const T* partials, int blocks, int entries, T* table, dir_stream_t stream) {
    hipLaunchKernelGGL(dir_table_fold_kernel<T>, dim3(dir_cdiv(entries, DIR_TPB)), dim3(DIR_TPB), 0, dir_s(stream), partials, blocks, entries, table);
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}
