// resample_mfma_host.hpp -- host-side (plain C++, no HIP) geometry of resample_mfma_kernel
// (kernels_resample.hip): per 16-row output tile its top input offset, the K-steps in sixteens, the tile
// groups one workgroup stages together, and the tap image in A-operand order of v_mfma_f32_16x16x4_f32.
// Header-only so that tests/cpp/resample_mfma_host_test.cpp can dump it with g++ on a box without a GPU
// (tests/test_mfma_model_host.py compares it with the numpy model of the kernel).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace fmrx {

constexpr int kRsTiles = 4;                    // output tiles per workgroup: one per wave
constexpr int kRsPieces = 160;                 // 16-byte pieces per staged row at most (16 rows x 161 x 16 B = 41 KB)

struct RsMfmaGeometry {
    int ks4 = 0;                               // K-steps / 4: an even count from 8 to 16 (kernel instances)
    int k = 0;                                 // inputs the widest tile's 16 rows touch
    int max_pieces = 0;                        // largest staged row, in 16-byte pieces
    std::vector<int> top;                      // [tile]: input offset (in the period) of K index 0; top % 4 == 3
    std::vector<int> groups;                   // [group][4]: m0, m1, lo (oldest staged input), pieces
    std::vector<float> img;                    // [tile][lane][4 ks4]
};

// Output r = q U + 16 m + i of period q: tile m, row i.  Tile m: K index w <-> input offset top[m] - w inside the period.
// Returns false where the kernel does not apply (D % 4 != 0, U < 16, a window wider than 16 K-step groups of 16 or a
// staged row longer than kRsPieces).
inline bool resample_mfma_geometry(const float *h, int taps, int U, int D, RsMfmaGeometry &g)
{
    const int J = (taps + U - 1) / U;
    if (D % 4 != 0 || U < 16) return false;
    const int ntiles = (U + 15) / 16;
    std::vector<int> top(ntiles), b0(ntiles);
    int K = 0;
    for (int m = 0; m < ntiles; m++) {
        const int r_last = std::min(16 * m + 15, U - 1);
        const int bmax = static_cast<int>(static_cast<long>(r_last) * D / U);
        b0[m] = static_cast<int>(static_cast<long>(16 * m) * D / U);
        top[m] = (bmax + 1 + 3) / 4 * 4 - 1;
        K = std::max(K, top[m] - b0[m] + J);
    }
    const int KS4 = std::max(8, (K + 31) / 32 * 2);             // K-steps in sixteens: an even count from 8 to 16 (kernel instances)
    if (KS4 > 16) return false;
    // tile groups of kRsTiles consecutive tiles (one per wave): a period's staged window = what the group's tiles read
    std::vector<int> grp;
    int max_pieces = 0;
    for (int m = 0; m < ntiles; m += kRsTiles) {
        const int m1 = std::min(m + kRsTiles, ntiles);
        const int lo = top[m] - 16 * KS4 + 1;                      // oldest input tile m reads; top % 4 == 3 -> a multiple of 4
        const int pieces = (top[m1 - 1] - lo + 1) / 4;
        if (pieces > kRsPieces) return false;
        max_pieces = std::max(max_pieces, pieces);
        grp.insert(grp.end(), {m, m1, lo, pieces});
    }
    // tap image [tile][lane][K-step]: lane (row i = lane & 15, kq = lane >> 4), K-step ks <-> K index w = 16 (ks/4) + 4 kq + ks%4
    std::vector<float> img(static_cast<size_t>(ntiles) * 64 * 4 * KS4, 0.0f);
    for (int m = 0; m < ntiles; m++)
        for (int lane = 0; lane < 64; lane++) {
            const int i = lane & 15, kq = lane >> 4, r = 16 * m + i;
            if (r >= U) continue;
            const long rd = static_cast<long>(r) * D;
            const int ph = static_cast<int>(rd % U), bi = static_cast<int>(rd / U);
            for (int ks = 0; ks < 4 * KS4; ks++) {
                const int w = 16 * (ks / 4) + 4 * kq + ks % 4;
                const int j = bi - (top[m] - w);
                if (j >= 0 && j < J && ph + static_cast<long>(j) * U < taps)
                    img[(static_cast<size_t>(m) * 64 + lane) * 4 * KS4 + ks] = h[ph + j * U];
            }
        }
    g.ks4 = KS4;
    g.k = K;
    g.max_pieces = max_pieces;
    g.top = std::move(top);
    g.groups = std::move(grp);
    g.img = std::move(img);
    return true;
}

// staging loads per thread: the 16-byte-piece instance, and the element instance (even counts only)
inline int resample_mfma_nl(int max_pieces) { return std::max(4, (max_pieces + 15) / 16); }
inline int resample_mfma_nl_elem(int max_pieces) { return (resample_mfma_nl(max_pieces) + 1) / 2 * 2; }

// piece staging reads from the first period's lowest window start to the last period's highest one + 16 NL pieces: true
// when that stays within `front` samples in front of the block and `back` behind it
inline bool resample_mfma_reach_ok(const RsMfmaGeometry &g, int D, int front, int back)
{
    const int nl = resample_mfma_nl(g.max_pieces);
    int lo_min = 0, lo_max = 0;
    for (size_t k = 0; k < g.groups.size(); k += 4) {
        lo_min = std::min(lo_min, g.groups[k + 2]);
        lo_max = std::max(lo_max, g.groups[k + 2]);
    }
    return -lo_min <= front && lo_max + 64 * nl - D <= back;
}

}  // namespace fmrx
