// Index arithmetic shared by every convolution kernel family (dir_conv.hip, dir_conv_wgrad.hip, dir_conv_f32.hip): the workgroup -> tile
// remap and the GEMM-row -> pixel decode. Plain integer / float code with no HIP dependency, so that a host program can include this
// header and check the functions the kernels run (tests/csrc/check_pixel_decode.cpp).
#pragma once

#if defined(__HIPCC__)
#define CV_INDEX_FN __host__ __device__ __forceinline__
#else
#define CV_INDEX_FN inline
#endif

// Workgroup id -> linear tile index, XCD-aware and bijective on [0, nblocks): the hardware deals workgroup b to XCD b % 8, so the linear
// tile space is cut into 8 contiguous chunks (the first nblocks % 8 of them one tile longer) and neighbouring tiles run on the same XCD:
// the operand re-reads of tiles that share rows hit that XCD's L2.
CV_INDEX_FN int cv_xcd_tile(int block, int nblocks) {
    const int q = nblocks / 8, r = nblocks % 8, xcd = block % 8, i = block / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + i;
}

// GEMM row m = (n * Ho + ho) * Wo + wo -> (n, ho, wo) with inv_wo = 1.0f / Wo, inv_ho = 1.0f / Ho: a float reciprocal and one correction
// step per level instead of two integer divisions. PRECONDITION: 0 <= m < 2^24 (then (float)m is exact and the truncated product is off
// by at most one, which the correction repairs); the host launchers refuse larger problems.
CV_INDEX_FN void cv_pixel_decode(int m, int Wo, int Ho, float inv_wo, float inv_ho, int& n, int& ho, int& wo) {
    int q1 = (int)((float)m * inv_wo);
    wo = m - q1 * Wo;
    if (wo < 0) { --q1; wo += Wo; } else if (wo >= Wo) { ++q1; wo -= Wo; }
    n = (int)((float)q1 * inv_ho);
    ho = q1 - n * Ho;
    if (ho < 0) { --n; ho += Ho; } else if (ho >= Ho) { ++n; ho -= Ho; }
}
