// Host check of cv_pixel_decode (csrc/dir_conv_index.h, the very function the convolution kernels compile): for every GEMM row m in
// [0, 2^24) — the range the launchers admit — the float-reciprocal decode must equal integer division, for ResNet-50's maps and for
// degenerate / lopsided ones. Exit status 0 = no mismatch. Built by tests/test_pixel_decode_host.py with the host compiler and
// -fsanitize=address,undefined; no HIP involved.
#include <cstdio>
#include "dir_conv_index.h"

int main() {
    static const int maps[][2] = {{56, 56}, {28, 28}, {14, 14}, {7, 7}, {112, 112}, {1, 1}, {3, 200}, {200, 3}, {13, 9}, {223, 1}, {1, 223}, {2, 2}, {5, 3}};   // (Wo, Ho)
    long long bad = 0;
    for (const auto& wh : maps) {
        const int Wo = wh[0], Ho = wh[1];
        const float inv_wo = 1.0f / (float)Wo, inv_ho = 1.0f / (float)Ho;          // as the host launchers compute them
        long long bad_here = 0;
        for (int m = 0; m < (1 << 24); ++m) {
            int n, ho, wo;
            cv_pixel_decode(m, Wo, Ho, inv_wo, inv_ho, n, ho, wo);
            const int q = m / Wo;
            if (wo != m % Wo || ho != q % Ho || n != q / Ho) {
                if (bad_here++ < 5) std::printf("Wo=%d Ho=%d m=%d: decode (%d, %d, %d), exact (%d, %d, %d)\n", Wo, Ho, m, n, ho, wo, q / Ho, q % Ho, m % Wo);
            }
        }
        std::printf("Wo=%d Ho=%d: %lld mismatches\n", Wo, Ho, bad_here);
        bad += bad_here;
    }
    // the tile remap is a bijection on [0, nblocks) (checked for every grid up to 2048 workgroups)
    static bool seen[2048];
    for (int nb = 1; nb <= 2048; ++nb) {
        for (int i = 0; i < nb; ++i) seen[i] = false;
        for (int b = 0; b < nb; ++b) {
            const int lin = cv_xcd_tile(b, nb);
            if (lin < 0 || lin >= nb || seen[lin]) { if (bad++ < 5) std::printf("cv_xcd_tile(%d, %d) = %d: out of range or repeated\n", b, nb, lin); }
            else seen[lin] = true;
        }
    }
    return bad ? 1 : 0;
}
