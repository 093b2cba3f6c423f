// JPEG decode, device stage: everything behind the entropy decoder (dir_jpeg_host.cpp), for a batch of B images described by a device
// table, written straight into the ragged `flat` uint8 buffer dir_resize_u8 consumes. Bit for bit libjpeg(-turbo) as Pillow drives it:
//   launch 1  dequantise + 8x8 inverse DCT (jidctint.c "islow": CONST_BITS 13, PASS1_BITS 2, column pass, row pass, its DESCALE
//             roundings) + range limit -> one byte plane per component in the workspace (plane stride = blocks per row * 8);
//   launch 2  chroma upsampling (jdsample.c "fancy": triangle filters whose edges are the component's TRUE down-sampled size, plain
//             replication when the chroma row has two samples or fewer) + YCbCr -> RGB (jdcolor.c's 16-bit fixed-point tables) -> flat.
// Byte / int32 work, HBM-trivial (about 3 B per pixel in, 3 B out): coalesced access and nothing more.
//   table [B][DIR_JPEG_ROW] int64 = (coef offset, flat byte offset, W, H, components, luma hsamp, luma vsamp, quant slot)
// The planes of an image sit at its coefficient offset in the workspace: one plane byte per coefficient.
#include "dir_common.h"

namespace {
constexpr int JP_BLOCKS = DIR_TPB / 8;                       // 8 lanes per 8x8 block: 32 blocks per workgroup, 8 per wavefront
constexpr int JP_PITCH = 9;                                  // LDS words per block row: with 72 words per block the column-pass stores
constexpr int JP_BLOCK_WORDS = 8 * JP_PITCH;                 // and the row-pass loads of a 32-lane half hit 32 different banks
constexpr int JP_PX = 4;                                     // pixels per thread in launch 2

struct JpImage {
    long long coef_off, flat_off;
    int W, H, ncomp, hs, vs, slot;
    int bw0, bh0, bw1, bh1;                                  // block grids: luma, chroma
    long long nblk0, nblk1, nblocks;
    bool ok;
};

// One table row, checked against everything the launch was sized for: a row that does not fit is skipped by both kernels, never read
// or written through (the table is device memory, the host entry point cannot look at it without a sync).
__device__ __forceinline__ JpImage jp_row(const long long* __restrict__ table, int b, long long ncoef, int nslots, long long max_blocks,
                                          long long max_pixels, long long flat_bytes) {
    const long long* r = table + (size_t)b * DIR_JPEG_ROW;
    JpImage im;
    im.coef_off = r[0]; im.flat_off = r[1];
    const long long W = r[2], H = r[3], nc = r[4], hs = r[5], vs = r[6], slot = r[7];
    im.ok = W > 0 && H > 0 && W <= DIR_JPEG_MAX_DIM && H <= DIR_JPEG_MAX_DIM && (nc == 1 || nc == 3) && slot >= 0 && slot < nslots &&
            ((hs == 1 && vs == 1) || (nc == 3 && hs == 2 && (vs == 1 || vs == 2)));
    im.W = (int)W; im.H = (int)H; im.ncomp = (int)nc; im.hs = (int)hs; im.vs = (int)vs; im.slot = (int)slot;
    if (!im.ok) return im;
    im.bw1 = (im.W + 8 * im.hs - 1) / (8 * im.hs); im.bh1 = (im.H + 8 * im.vs - 1) / (8 * im.vs);     // MCUs per row / column
    im.bw0 = im.bw1 * im.hs; im.bh0 = im.bh1 * im.vs;
    im.nblk0 = (long long)im.bw0 * im.bh0;
    im.nblk1 = im.ncomp == 3 ? (long long)im.bw1 * im.bh1 : 0;
    im.nblocks = im.nblk0 + 2 * im.nblk1;
    im.ok = im.nblocks <= max_blocks && W * H <= max_pixels && im.coef_off >= 0 && (im.coef_off & 7) == 0 && im.coef_off + im.nblocks * 64 <= ncoef &&
            im.flat_off >= 0 && im.flat_off + W * H * 3 <= flat_bytes;
    return im;
}

// jidctint.c's one-dimensional pass on eight values, before the final descale. uint32 arithmetic: wrap-around is defined, and add,
// subtract, multiply and left shift give the low 32 bits of the library's (long) results — equal to them on every stream whose true
// intermediates fit 32 bits, which covers every valid one; only DESCALE's right shift is signed.
__device__ __forceinline__ void jp_idct8(const uint32_t in[8], uint32_t out[8]) {
    constexpr uint32_t F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
                       F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
                       F_2_562915447 = 20995, F_3_072711026 = 25172;
    uint32_t z1, z2, z3, z4, z5, tmp0, tmp1, tmp2, tmp3;
    // even part
    z2 = in[2]; z3 = in[6];
    z1 = (z2 + z3) * F_0_541196100;
    tmp2 = z1 + z3 * (0u - F_1_847759065);
    tmp3 = z1 + z2 * F_0_765366865;
    z2 = in[0]; z3 = in[4];
    tmp0 = (z2 + z3) << 13;
    tmp1 = (z2 - z3) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    // odd part
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2; z4 = tmp1 + tmp3;
    z5 = (z3 + z4) * F_1_175875602;
    tmp0 *= F_0_298631336; tmp1 *= F_2_053119869; tmp2 *= F_3_072711026; tmp3 *= F_1_501321110;
    z1 *= 0u - F_0_899976223; z2 *= 0u - F_2_562915447; z3 *= 0u - F_1_961570560; z4 *= 0u - F_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
    out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
    out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}
__device__ __forceinline__ int jp_descale(uint32_t x, int n) { return (int)(x + (1u << (n - 1))) >> n; }
// the library's range-limit table: the low 10 bits as a signed number, + 128, clamped to a byte
__device__ __forceinline__ uint32_t jp_limit(int v) {
    v = ((v & 1023) ^ 512) - 512 + 128;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// grid (ceil(max_blocks / 32), B). Lane j of a block's 8 lanes: column j in pass 1, row j in pass 2; the 8x8 int32 intermediate is
// transposed through LDS. The library's zero-AC shortcuts give the same bits as the full computation: no branch on them.
__global__ void __launch_bounds__(DIR_TPB)
jpeg_idct_kernel(const int16_t* __restrict__ coef, long long ncoef, const uint16_t* __restrict__ quant, int nslots, const long long* __restrict__ table,
                 long long max_blocks, long long max_pixels, long long flat_bytes, uint8_t* __restrict__ planes) {
    __shared__ uint32_t ws[JP_BLOCKS * JP_BLOCK_WORDS];
    const JpImage im = jp_row(table, blockIdx.y, ncoef, nslots, max_blocks, max_pixels, flat_bytes);
    const int j = threadIdx.x & 7, lb = threadIdx.x >> 3;
    const long long g = (long long)blockIdx.x * JP_BLOCKS + lb;                      // block of the image, components back to back
    const bool live = im.ok && g < im.nblocks;                                         // (no early return: the barrier below is for everybody)
    int comp = 0, bw = 1;
    long long gl = 0, plane = 0;
    if (live) {
        comp = g < im.nblk0 ? 0 : (g < im.nblk0 + im.nblk1 ? 1 : 2);
        gl = g - (comp == 0 ? 0 : (comp == 1 ? im.nblk0 : im.nblk0 + im.nblk1));
        plane = im.coef_off + 64 * (g - gl);
        bw = comp == 0 ? im.bw0 : im.bw1;
    }
    uint32_t v[8], o[8];
    uint32_t* w = ws + lb * JP_BLOCK_WORDS;
    if (live) {
        const int16_t* c = coef + im.coef_off + g * 64 + j;
        const uint16_t* q = quant + ((size_t)im.slot * 3 + comp) * 64 + j;
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = (uint32_t)((int)c[8 * r] * (int)q[8 * r]);        // |product| < 2^31: int16 times uint16
        jp_idct8(v, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r * JP_PITCH + j] = (uint32_t)jp_descale(o[r], 13 - 2);
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = w[j * JP_PITCH + k];
        jp_idct8(v, o);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= jp_limit(jp_descale(o[k], 13 + 2 + 3)) << (8 * k);
            hi |= jp_limit(jp_descale(o[k + 4], 13 + 2 + 3)) << (8 * k);
        }
        const int by = (int)(gl / bw), bx = (int)(gl - (long long)by * bw);
        // 8-byte aligned: the plane offset is a multiple of 64 (coef_off % 8 == 0 is checked, blocks are 64), the stride and bx * 8 of 8
        *reinterpret_cast<uint2*>(planes + plane + ((long long)by * 8 + j) * ((long long)bw * 8) + (long long)bx * 8) = make_uint2(lo, hi);
    }
}

// one chroma sample at full resolution for pixel (x, y): jdsample.c's fullsize / h2v1 / h2v2 upsamplers. p: the component's plane, stride
// its padded width; cw, ch: its TRUE size, ceil(W / hs) x ceil(H / vs) — the filters' edges, beyond which the neighbour is the sample itself.
__device__ __forceinline__ int jp_chroma(const uint8_t* __restrict__ p, int stride, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * stride + x];
    const int cx = x >> 1, cy = vs == 2 ? y >> 1 : y;
    const uint8_t* row = p + (size_t)cy * stride;
    if (cw <= 2) return row[cx];                                                     // too narrow for the triangle filter: replication
    const int nx = (x & 1) ? (cx + 1 < cw ? cx + 1 : cx) : (cx > 0 ? cx - 1 : cx);
    if (vs == 1) return (3 * row[cx] + row[nx] + ((x & 1) ? 2 : 1)) >> 2;
    const int ny = (y & 1) ? (cy + 1 < ch ? cy + 1 : cy) : (cy > 0 ? cy - 1 : cy);
    const uint8_t* far = p + (size_t)ny * stride;
    const int here = 3 * row[cx] + far[cx], there = 3 * row[nx] + far[nx];            // vertical stage: 3 * near + far
    return (3 * here + there + ((x & 1) ? 7 : 8)) >> 4;
}

// grid (ceil(max_pixels / 256), B), of which an image uses H * ceil(W / 4) threads: a thread writes up to 4 adjacent pixels of one row.
__global__ void __launch_bounds__(DIR_TPB)
jpeg_colour_kernel(const uint8_t* __restrict__ planes, long long ncoef, int nslots, const long long* __restrict__ table, long long max_blocks,
                   long long max_pixels, long long flat_bytes, uint8_t* __restrict__ flat) {
    const JpImage im = jp_row(table, blockIdx.y, ncoef, nslots, max_blocks, max_pixels, flat_bytes);
    if (!im.ok) return;
    const int per_row = (im.W + JP_PX - 1) / JP_PX;
    const long long i = (long long)blockIdx.x * DIR_TPB + threadIdx.x;
    if (i >= (long long)im.H * per_row) return;
    const int y = (int)(i / per_row), x0 = (int)(i - (long long)y * per_row) * JP_PX;
    const int n = im.W - x0 < JP_PX ? im.W - x0 : JP_PX;
    const uint8_t* py = planes + im.coef_off;
    const uint8_t* pcb = py + im.nblk0 * 64;
    const uint8_t* pcr = pcb + im.nblk1 * 64;
    const int s0 = im.bw0 * 8, s1 = im.bw1 * 8;
    const int cw = (im.W + im.hs - 1) / im.hs, ch = (im.H + im.vs - 1) / im.vs;
    uint8_t px[3 * JP_PX];
#pragma unroll
    for (int k = 0; k < JP_PX; ++k) {
        const int x = x0 + (k < n ? k : 0);
        const int Y = py[(size_t)y * s0 + x];
        int R = Y, G = Y, B = Y;
        if (im.ncomp == 3) {
            // jdcolor.c: FIX(v) = (int)(v * 65536 + .5); R = Y + ((FIX(1.40200) * Cr + ONE_HALF) >> 16), B likewise with FIX(1.77200) * Cb,
            // G = Y + ((-FIX(0.34414) * Cb + ONE_HALF - FIX(0.71414) * Cr) >> 16); arithmetic shifts, then the clamp
            const int cb = jp_chroma(pcb, s1, cw, ch, im.hs, im.vs, x, y) - 128, cr = jp_chroma(pcr, s1, cw, ch, im.hs, im.vs, x, y) - 128;
            R = Y + ((91881 * cr + 32768) >> 16);
            G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
            B = Y + ((116130 * cb + 32768) >> 16);
            R = R < 0 ? 0 : (R > 255 ? 255 : R); G = G < 0 ? 0 : (G > 255 ? 255 : G); B = B < 0 ? 0 : (B > 255 ? 255 : B);
        }
        px[3 * k] = (uint8_t)R; px[3 * k + 1] = (uint8_t)G; px[3 * k + 2] = (uint8_t)B;
    }
    uint8_t* o = flat + im.flat_off + ((size_t)y * im.W + x0) * 3;
    if (n == JP_PX && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {                    // 12 bytes as three words
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k) o4[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 3 * JP_PX; ++k)
            if (k < 3 * n) o[k] = px[k];
    }
}
}  // namespace

extern "C" size_t dir_jpeg_reconstruct_workspace(long long ncoef) {
    return ncoef > 0 ? dir_align_up((size_t)ncoef, 256) : 0;
}

extern "C" int dir_jpeg_reconstruct(const int16_t* coef, long long ncoef, const uint16_t* quant, int nslots, const long long* table, int B,
                                    long long max_blocks, long long max_pixels, void* flat, long long flat_bytes, void* workspace,
                                    size_t workspace_bytes, dir_stream_t stream) {
    DIR_RETURN_IF(!coef || !quant || !table || !flat || !workspace || B <= 0 || ncoef <= 0 || nslots <= 0 || max_blocks <= 0 || max_pixels <= 0 ||
                  flat_bytes <= 0, DIR_EINVAL);
    DIR_RETURN_IF((reinterpret_cast<uintptr_t>(coef) & 1u) || (reinterpret_cast<uintptr_t>(quant) & 1u) || (reinterpret_cast<uintptr_t>(table) & 7u) ||
                  (reinterpret_cast<uintptr_t>(workspace) & 7u), DIR_EINVAL);
    DIR_RETURN_IF(B > 65535 || max_pixels > (long long)DIR_JPEG_MAX_DIM * DIR_JPEG_MAX_DIM, DIR_EUNSUPPORTED);
    DIR_RETURN_IF(max_blocks * 64 > ncoef, DIR_EINVAL);
    DIR_RETURN_IF(workspace_bytes < (size_t)ncoef, DIR_EWORKSPACE);
    hipStream_t s = dir_s(stream);
    uint8_t* planes = static_cast<uint8_t*>(workspace);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3(dir_cdiv(max_blocks, JP_BLOCKS), B), dim3(DIR_TPB), 0, s, coef, ncoef, quant, nslots, table, max_blocks,
                       max_pixels, flat_bytes, planes);
    DIR_LAUNCH_CHECK();
    // threads of an image: H * ceil(W / 4) <= H * W <= max_pixels, with equality for W = 1: sized for the worst aspect ratio
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3(dir_cdiv(max_pixels, DIR_TPB), B), dim3(DIR_TPB), 0, s, planes, ncoef, nslots, table, max_blocks,
                       max_pixels, flat_bytes, static_cast<uint8_t*>(flat));
    DIR_LAUNCH_CHECK();
    return DIR_OK;
}
