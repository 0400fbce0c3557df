// kernels_audio_meters.hip -- the kernel of the audio meters (include/fmrx.h: fmrx_audio_meters_*; DESIGN.md section 4.14;
// defined by tests/_audio_meters_model.py).
//
// The walk of one channel is audio_meters_core.hpp's, the body the host reference compiles too.  Its recurrence cannot be
// started in the middle of a row (the high-pass has its poles at 0.995), so the parallelism is over channels: one lane walks one
// channel, a wave (= a workgroup) 64 of them; the two rows of a stereo channel are two independent chains in the lane, which
// hides half the latency of the dependent float64 operations.
//
// Where the samples come from.  One lane per row reading global memory would touch 64 different lines with every load.  Instead
// the wave fetches a tile of [64 * ac rows][32 samples], each row's 128 bytes contiguous (a whole line where rows are 16-byte
// aligned): with 16-byte loads 8 lanes cover a row's piece and one load instruction 8 rows.  The tile of chunk j + 1 is in
// flight in registers while the lanes walk chunk j out of LDS, so the tile is double-buffered between registers and LDS, and
// the wave waits for memory only where a chunk's loads take longer than walking the chunk before it.  In LDS the tile is
// [ac][64][33]: lane l reads its row at dword (r * 64 + l) * 33 + k, and the odd pitch puts the 32 lanes of each half of a
// ds_read_b32 on 32 different banks.  (The fill's ds_write_b32 are 2-way conflicted, which that instruction's rate hides.)
// Rows that are not 16-byte aligned (the base is not, or the pitch is no multiple of 4) are fetched 4 bytes per lane, 32 lanes
// per row's piece; the arithmetic is the same.  No load reaches past sample n of a row or past the last row: the pieces of a
// 16-byte fetch that would are fetched singly.
//
// State and results are field-major ([field][n_channels]): the lanes' loads and stores are consecutive.  Bins go out as they
// close, [n_channels][2][max_bins]; the rest of a channel's bins is zeroed at the end.  Everything is written with plain
// vector stores.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 4.14; no variant uses scratch.
#include "audio_meters_core.hpp"
#include "fmrx_internal.hpp"

namespace fmrx {
namespace {

constexpr int kLanes = 64;         // channels per wave and workgroup
constexpr int kChunk = 32;         // samples per row in a tile
constexpr int kPitch = kChunk + 1;   // dwords per tile row in LDS
constexpr int kUnroll = 8;         // samples the walk's loop is unrolled by: enough LDS reads in flight, registers to spare

struct KernelArgs {
    const float *x;
    size_t pitch, n, max_bins;
    long n_channels;
    unsigned bin_len;
    audio_meters::Coefs c;
    double *state;
    unsigned *fill;
    double *sums;
    unsigned *counts;
    double *bins;
};

// VEC floats per lane and load: a row's piece takes kChunk / VEC lanes, one load instruction 64 / (kChunk / VEC) rows
template <int AC, int VEC>
struct Tile {
    static constexpr int kRows = kLanes * AC;
    static constexpr int kLanesPerRow = kChunk / VEC;
    static constexpr int kRowsPerLoad = kLanes / kLanesPerRow;
    static constexpr int kLoads = kRows / kRowsPerLoad;
};

// the wave's rows [row0, row0 + kRows) of chunk k0 -> stage; what lies past n or past the last row reads 0 and is never walked
template <int AC, int VEC>
__device__ __forceinline__ void fetch(const KernelArgs &a, size_t row0, size_t rows, size_t k0, int lane, float (&stage)[Tile<AC, VEC>::kLoads][VEC])
{
    using T = Tile<AC, VEC>;
    const int frow = lane / T::kLanesPerRow;
    const size_t col = k0 + static_cast<size_t>(lane % T::kLanesPerRow) * VEC;
#pragma unroll
    for (int i = 0; i < T::kLoads; i++) {
        const size_t row = row0 + static_cast<size_t>(i * T::kRowsPerLoad + frow);
        const float *p = a.x + row * a.pitch + col;
        const bool in = row < rows;
        if (VEC == 4 && in && col + 4 <= a.n) {
            const float4 v = *reinterpret_cast<const float4 *>(p);
            const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < VEC; e++) stage[i][e] = e4[e];
        } else {
#pragma unroll
            for (int e = 0; e < VEC; e++) stage[i][e] = in && col + e < a.n ? p[e] : 0.0f;
        }
    }
}

// stage -> the LDS tile [AC][64][kPitch]: global row R of the wave (channel R / AC, audio channel R % AC) is tile row (R % AC) * 64 + R / AC
template <int AC, int VEC>
__device__ __forceinline__ void stash(float *tile, int lane, const float (&stage)[Tile<AC, VEC>::kLoads][VEC])
{
    using T = Tile<AC, VEC>;
    const int frow = lane / T::kLanesPerRow, fcol = (lane % T::kLanesPerRow) * VEC;
#pragma unroll
    for (int i = 0; i < T::kLoads; i++) {
        const int R = i * T::kRowsPerLoad + frow;
        float *q = tile + ((R % AC) * kLanes + R / AC) * kPitch + fcol;
#pragma unroll
        for (int e = 0; e < VEC; e++) q[e] = stage[i][e];
    }
}

template <int AC, int VEC>
__global__ __launch_bounds__(kLanes) void audio_meters_kernel(KernelArgs a)
{
    using T = Tile<AC, VEC>;
    __shared__ float tile[T::kRows * kPitch];
    const int lane = threadIdx.x;
    const size_t N = static_cast<size_t>(a.n_channels);
    const size_t ch0 = static_cast<size_t>(blockIdx.x) * kLanes, ch = ch0 + lane;
    const bool live = ch < N;
    const size_t row0 = ch0 * AC, rows = N * AC;

    audio_meters::Walk<AC> w;
    w.begin();
#pragma unroll
    for (int r = 0; r < AC; r++) {
#pragma unroll
        for (int i = 0; i < 4; i++) w.z[r][i] = live ? a.state[(r * 4 + i) * N + ch] : 0.0;
        w.bin_acc[r] = live ? a.state[(8 + r) * N + ch] : 0.0;
    }
    w.bin_fill = live ? a.fill[ch] : 0u;
    double *bins = a.bins + (live ? ch : 0) * 2 * a.max_bins;

    float stage[T::kLoads][VEC];
    fetch<AC, VEC>(a, row0, rows, 0, lane, stage);
    const float *mine = tile + lane * kPitch;
    for (size_t k0 = 0; k0 < a.n; k0 += kChunk) {
        __syncthreads();   // the walk of the chunk before has read the tile
        stash<AC, VEC>(tile, lane, stage);
        __syncthreads();
        if (k0 + kChunk < a.n) fetch<AC, VEC>(a, row0, rows, k0 + kChunk, lane, stage);
        const size_t left = a.n - k0;
        if (live) {
            if (left >= kChunk) {
#pragma unroll 1
                for (int g = 0; g < kChunk; g += kUnroll) {
                    if (w.bin_fill + kUnroll < a.bin_len) {   // no bin closes in this group: one straight-line block to schedule
#pragma unroll
                        for (int k = 0; k < kUnroll; k++) {
                            const float x[2] = {mine[g + k], mine[(AC - 1) * kLanes * kPitch + g + k]};
                            w.accumulate(a.c, x);
                        }
                        w.bin_fill += kUnroll;
                    } else {
#pragma unroll 1
                        for (int k = 0; k < kUnroll; k++) {
                            const float x[2] = {mine[g + k], mine[(AC - 1) * kLanes * kPitch + g + k]};
                            w.sample(a.c, x, a.bin_len, bins, a.max_bins);
                        }
                    }
                }
            } else {
                for (int k = 0; k < static_cast<int>(left); k++) {
                    const float x[2] = {mine[k], mine[(AC - 1) * kLanes * kPitch + k]};
                    w.sample(a.c, x, a.bin_len, bins, a.max_bins);
                }
            }
        }
    }
    if (!live) return;
    w.finish(bins, a.max_bins);
#pragma unroll
    for (int r = 0; r < AC; r++) {
#pragma unroll
        for (int i = 0; i < 4; i++) a.state[(r * 4 + i) * N + ch] = w.z[r][i];
        a.state[(8 + r) * N + ch] = w.bin_acc[r];
    }
    a.fill[ch] = w.bin_fill;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const bool has = r < AC;
        a.sums[(0 + r) * N + ch] = has ? static_cast<double>(w.peak[r % AC]) : 0.0;
        a.sums[(2 + r) * N + ch] = has ? w.sum_x[r % AC] : 0.0;
        a.sums[(4 + r) * N + ch] = has ? w.sum_x2[r % AC] : 0.0;
        a.sums[(6 + r) * N + ch] = has ? w.sum_k2[r % AC] : 0.0;
        a.counts[r * N + ch] = has ? w.over[r % AC] : 0u;
    }
    a.sums[8 * N + ch] = w.sum_lr;
    a.counts[2 * N + ch] = w.bins_done;
}

}  // namespace

int audio_meters_launch(const AudioMetersArgs &g, hipStream_t s)
{
    if (!g.x || !g.state || !g.fill || !g.sums || !g.counts || !g.bins) return fail(FMRX_EINVAL, "audio_meters: null buffer");
    if (g.n_channels < 1 || (g.ac != 1 && g.ac != 2)) return fail(FMRX_EINVAL, "audio_meters: n_channels >= 1, audio_channels 1 or 2");
    if (g.n < 1 || g.n > (size_t{1} << 26) || g.pitch < g.n) return fail(FMRX_EINVAL, "audio_meters: 1 .. 2^26 samples per row, in a pitch that holds them");
    if (g.bin_len < 1 || g.max_bins < g.n / g.bin_len + 1) return fail(FMRX_EINVAL, "audio_meters: %zu bins do not hold a call of %zu samples", g.max_bins, g.n);
    if (reinterpret_cast<uintptr_t>(g.x) % sizeof(float)) return fail(FMRX_EINVAL, "audio_meters: the rows must be 4-byte aligned");
    KernelArgs a{};
    a.x = g.x;
    a.pitch = g.pitch;
    a.n = g.n;
    a.max_bins = g.max_bins;
    a.n_channels = g.n_channels;
    a.bin_len = g.bin_len;
    std::memcpy(a.c.q, g.coef, sizeof a.c.q);
    a.state = g.state;
    a.fill = g.fill;
    a.sums = g.sums;
    a.counts = g.counts;
    a.bins = g.bins;
    const bool wide = reinterpret_cast<uintptr_t>(g.x) % 16 == 0 && g.pitch % 4 == 0;
    const unsigned blocks = static_cast<unsigned>((static_cast<size_t>(g.n_channels) + kLanes - 1) / kLanes);
    if (g.ac == 2 && wide) {
        audio_meters_kernel<2, 4><<<blocks, kLanes, 0, s>>>(a);
    } else if (g.ac == 2) {
        audio_meters_kernel<2, 1><<<blocks, kLanes, 0, s>>>(a);
    } else if (wide) {
        audio_meters_kernel<1, 4><<<blocks, kLanes, 0, s>>>(a);
    } else {
        audio_meters_kernel<1, 1><<<blocks, kLanes, 0, s>>>(a);
    }
    FMRX_LAUNCH_CHECK("audio_meters_kernel<%d,%d>", g.ac, wide ? 4 : 1);
    return FMRX_OK;
}

}  // namespace fmrx
