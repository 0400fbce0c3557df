// kernels_audio_spectrum.hip -- the kernels of the audio spectrum meter (include/fmrx.h: fmrx_audio_spectrum_*; DESIGN.md section
// 4.17; defined by tests/_audio_spectrum_model.py).
//
// A frame's 2 x 128 chains are one matrix product: the M rows are the outputs (re_k and im_k of 128 bins), K the 256 window
// positions, the N columns 16 frames.  v_mfma_f32_16x16x4_f32 adds its 4 products to an accumulator as a chain of exactly rounded
// fmaf in K order, so 64 dependent instructions whose K index is j = 4 s + kq (s the instruction, kq the K index inside it) are
// the model's chain over j ascending.  Operands (lane = 16 kq + i):
//   A  lane (i, kq) of instruction s holds the cosine of output row i at window position j = 4 s + kq: C[(k j) mod 256] for re_k,
//      C[(k j - 64) mod 256] for im_k, read as one pair from the 2 KiB table in LDS; the index advances by 4 k per instruction
//   B  lane (i, kq) holds xw[j = 4 s + kq] of frame (column) i; the windowed frames stand in LDS as [column][kq][s], so that four
//      instructions' operands are one 16-byte read
//   D  lane (i, kq) holds rows 4 kq .. 4 kq + 3 of column i
// A wave owns the re tile and the im tile of 2 x 16 bins: four independent accumulators, 128 cycles of issue between the
// dependent ones, and re_k and im_k of a frame in one lane, so that p_k needs no exchange.  The four waves of a workgroup cover
// the 128 bins of 16 frames.
//
// Which frames share an instruction is free (the columns are independent).  A row of at most 2 048 samples completes at most 8
// frames whatever its fill, so two rows share a workgroup, 8 columns each: the L and R rows of a stereo channel, two
// neighbouring channels of a mono bank.  Their tile sum is the call's sum and is stored plainly.  A longer row has workgroups of
// its own, tile t of 16 frames in the grid's y; each writes its tile's float64 sums to a scratch array, and a second small
// launch adds them ascending: the order is part of the definition, so no floating atomics.  The rows ride in the grid's x.
//
// A workgroup stages x w once per frame into LDS (stream position p of a row is its carried samples, then the call's; the loads
// are 4 bytes per lane, consecutive lanes consecutive samples, at any alignment: the pass is bound by the matrix cores, not by
// its fetches), multiplies, writes the p_k to LDS, sums the bands over ascending bins from LDS, one lane per (column, band), and
// then the frames of a row in float64, one lane per (row, band).  No load reaches past sample n of a row or past the last row:
// columns beyond a row's completed frames load from the carried state instead and multiply zeros.
//
// The carried state (fill per channel, the open frame's samples per row) is read from one pair of buffers and written to
// another, which the host swaps per call: no workgroup reads what another writes.  Every store is a plain vector store.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 4.17; no kernel uses scratch.
#include "fmrx_internal.hpp"
#include "audio_spectrum_core.hpp"

namespace fmrx {
namespace {

using f4 = float __attribute__((ext_vector_type(4)));
using f2 = float __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kFrame = audio_spectrum::kFrame, kBins = audio_spectrum::kBins, kTile = audio_spectrum::kTile, kMaxBands = audio_spectrum::kMaxBands;
constexpr int kSteps = kFrame / 4;            // matrix instructions of a chain
constexpr int kXwPitch = kSteps + 4;          // floats per (column, kq) in LDS: 16-byte pieces stay aligned, the lanes' reads spread over the banks
constexpr int kPowPitch = kBins + 4;          // floats per column of bin powers
// The cosine table in LDS: entry m holds the pair (C[m], C[(m - 64) mod 256]), the A operands of re_k and im_k at one angle, one
// 8-byte read.  Entry m stands in slot m + m / 32: the lanes of kq = 0 ask for multiples of 4 k, which without the skew fall
// on 8 of the 32 slots a cycle serves (up to 8 lanes each); with it 16 consecutive bins at any stride meet 16 different ones.
constexpr int kCosSlots = kFrame + kFrame / 32;
__device__ __forceinline__ int cos_slot(int m) { return m + (m >> 5); }
constexpr size_t kPairMax = kAudioSpectrumPairMax;
static_assert(kThreads == kFrame, "one lane per window position in the staging");
static_assert(kWaves * 32 == kBins, "a wave owns 32 bins");
static_assert((255 + kPairMax) / kFrame <= kTile / 2, "two rows share a tile");

__device__ const audio_spectrum::Tables d_tables = audio_spectrum::make_tables();

// PAIR: the workgroup holds rows 2 x and 2 x + 1 (of n_rows = n_channels AC), up to 8 frames each; else row x, tile y
template <int AC, bool PAIR>
__global__ __launch_bounds__(kThreads) void audio_spectrum_kernel(const float *__restrict__ x, size_t pitch, unsigned n_audio, unsigned n_channels,
                                                                  const int *__restrict__ edges, int n_bands, const unsigned *__restrict__ fill_in,
                                                                  const float *__restrict__ carry_in, unsigned *__restrict__ fill_out,
                                                                  float *__restrict__ carry_out, unsigned *__restrict__ frames_out,
                                                                  double *__restrict__ res, double *__restrict__ tiles)
{
    __shared__ __attribute__((aligned(16))) float xw[kTile * 4 * kXwPitch];
    __shared__ __attribute__((aligned(16))) float pw[kTile * kPowPitch];
    __shared__ __attribute__((aligned(8))) f2 ct[kCosSlots];
    __shared__ float bandp[kTile][kMaxBands];
    __shared__ int se[kMaxBands + 1];

    constexpr int S = PAIR ? 2 : 1;             // rows of the workgroup
    constexpr int PER = kTile / S;              // columns of a row
    const int tid = static_cast<int>(threadIdx.x);
    const size_t N = n_channels, n_rows = N * AC;
    const int n = static_cast<int>(n_audio);

    // the workgroup's rows: flat row R = channel AC + r; its fill, the frames F the call completes, the first frame q0 and the
    // count of frames of this tile (the same in every lane)
    size_t R[S];
    bool has[S];
    int fill[S], F[S], q0[S], cnt[S];
    int live = 0;
#pragma unroll
    for (int s = 0; s < S; s++) {
        R[s] = static_cast<size_t>(blockIdx.x) * S + s;
        has[s] = R[s] < n_rows;
        fill[s] = has[s] ? static_cast<int>(fill_in[R[s] / AC] & (kFrame - 1)) : 0;
        F[s] = has[s] ? (fill[s] + n) / kFrame : 0;
        q0[s] = PAIR ? 0 : static_cast<int>(blockIdx.y) * kTile;
        cnt[s] = F[s] - q0[s] < 0 ? 0 : (F[s] - q0[s] < PER ? F[s] - q0[s] : PER);
        live += cnt[s];
    }
    // stream position p < fill + n of row s: the carried samples, then the call's
    const auto stream = [&](int s, int p) -> float {
        return p < fill[s] ? carry_in[R[s] * kFrame + p] : x[R[s] * pitch + static_cast<size_t>(p - fill[s])];
    };

    if (live > 0) {
        ct[cos_slot(tid)] = (f2){d_tables.c[tid], d_tables.c[(tid + 3 * kFrame / 4) & (kFrame - 1)]};   // (m - 64) mod 256
        if (tid <= n_bands) se[tid] = edges[tid];
        // x w of window position j = tid of every column, to [column][kq = j mod 4][s = j div 4]
        const float w = d_tables.w[tid];
        float *dst = xw + (tid & 3) * kXwPitch + (tid >> 2);
        // all 16 loads are issued before the first is waited for: no branch around a load.  A column beyond the row's frames
        // loads the carried state's first KiB instead (it exists for every handle) and stages a zero
        float v[kTile];
#pragma unroll
        for (int c = 0; c < kTile; c++) {
            const int s = c / PER, q = c % PER;
            const int p = (q0[s] + q) * kFrame + tid;
            const float *at = carry_in + tid;
            if (q < cnt[s]) at = p < fill[s] ? carry_in + R[s] * kFrame + p : x + R[s] * pitch + static_cast<size_t>(p - fill[s]);
            v[c] = *at;
        }
#pragma unroll
        for (int c = 0; c < kTile; c++) dst[c * 4 * kXwPitch] = (c % PER < cnt[c / PER] ? v[c] : 0.0f) * w;
    }
    __syncthreads();

    // the next call's state, by the workgroup of the row's first tile: the samples behind the last completed frame
    if (PAIR || blockIdx.y == 0) {
#pragma unroll
        for (int s = 0; s < S; s++) {
            if (!has[s]) continue;
            const int left = (fill[s] + n) & (kFrame - 1);
            if (tid < left) carry_out[R[s] * kFrame + tid] = stream(s, F[s] * kFrame + tid);
            if (tid == 0 && R[s] % AC == 0) {
                fill_out[R[s] / AC] = static_cast<unsigned>(left);
                frames_out[R[s] / AC] = static_cast<unsigned>(F[s]);
            }
        }
    }

    if (live > 0) {
        const int lane = tid & 63, wv = tid >> 6;
        const int i = lane & 15, kq = lane >> 4;
        f4 re[2], im[2];
        int idx[2], step[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int k = 32 * wv + 16 * t + i;      // the bin of this lane's row of A
            re[t] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
            im[t] = re[t];
            idx[t] = (k * kq) & (kFrame - 1);
            step[t] = (4 * k) & (kFrame - 1);
        }
        const float *bcol = xw + (i * 4 + kq) * kXwPitch;
        for (int s4 = 0; s4 < kSteps / 4; s4++) {
            const f4 b = *reinterpret_cast<const f4 *>(bcol + 4 * s4);
#pragma unroll
            for (int e = 0; e < 4; e++) {
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    const f2 a = ct[cos_slot(idx[t])];
                    re[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[e], re[t], 0, 0, 0);
                    im[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[e], im[t], 0, 0, 0);
                    idx[t] = (idx[t] + step[t]) & (kFrame - 1);
                }
            }
        }
        // this lane: column i, bins 32 wv + 16 t + 4 kq + v
#pragma unroll
        for (int t = 0; t < 2; t++) {
            f4 p;
#pragma unroll
            for (int v = 0; v < 4; v++) p[v] = audio_spectrum::bin_power(re[t][v], im[t][v]);
            *reinterpret_cast<f4 *>(pw + i * kPowPitch + 32 * wv + 16 * t + 4 * kq) = p;
        }
    }
    __syncthreads();

    if (live > 0) {
        for (int task = tid; task < kTile * kMaxBands; task += kThreads) {
            const int c = task / kMaxBands, b = task % kMaxBands;
            if (b < n_bands) bandp[c][b] = audio_spectrum::band_sum(pw + c * kPowPitch, se[b], se[b + 1]);
        }
    }
    __syncthreads();

    // the tile's sum over its frames, ascending from +0.0, in float64
    if (tid < S * kMaxBands) {
        const int s = tid / kMaxBands, b = tid % kMaxBands;
        const bool second = S == 2 && s == 1;   // (no indexing of the per-row registers by a lane's own s)
        const bool mine = second ? has[S - 1] : has[0];
        const int frames = second ? cnt[S - 1] : cnt[0];
        const size_t row = second ? R[S - 1] : R[0];
        if (mine && b < n_bands) {
            double acc = 0.0;
            for (int q = 0; q < frames; q++) acc = acc + static_cast<double>(bandp[s * PER + q][b]);
            if (PAIR) res[((row % AC) * n_bands + b) * N + row / AC] = acc;
            else tiles[(static_cast<size_t>(blockIdx.y) * n_rows + row) * n_bands + b] = acc;
        }
    }
}

// the call's sum over a long row's tiles, ascending from +0.0: one lane per (row, band)
template <int AC>
__global__ __launch_bounds__(kThreads) void audio_spectrum_sum_kernel(const double *__restrict__ tiles, unsigned n_tiles, unsigned n_channels, int n_bands,
                                                                      double *__restrict__ res)
{
    const size_t N = n_channels, n_rows = N * AC;
    const size_t id = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
    if (id >= n_rows * n_bands) return;
    const size_t R = id / n_bands, b = id % n_bands;
    double acc = 0.0;
    for (unsigned t = 0; t < n_tiles; t++) acc = acc + tiles[(static_cast<size_t>(t) * n_rows + R) * n_bands + b];
    res[((R % AC) * n_bands + b) * N + R / AC] = acc;
}

}  // namespace

size_t audio_spectrum_tiles(size_t n) { return ((kFrame - 1 + n) / kFrame + kTile - 1) / kTile; }

int audio_spectrum_launch(const AudioSpectrumArgs &a, hipStream_t s)
{
    if (!a.x || !a.edges || !a.fill_in || !a.carry_in || !a.fill_out || !a.carry_out || !a.frames || !a.res) return fail(FMRX_EINVAL, "audio_spectrum: null buffer");
    if (a.n_channels < 1 || (a.ac != 1 && a.ac != 2)) return fail(FMRX_EINVAL, "audio_spectrum: n_channels >= 1, audio_channels 1 or 2");
    if (a.n_bands < 1 || a.n_bands > kMaxBands) return fail(FMRX_EINVAL, "audio_spectrum: 1 .. 32 bands");
    if (a.n < 1 || a.n > (size_t{1} << 26) || a.pitch < a.n) return fail(FMRX_EINVAL, "audio_spectrum: 1 .. 2^26 samples per row, in a pitch that holds them");
    if (reinterpret_cast<uintptr_t>(a.x) % sizeof(float)) return fail(FMRX_EINVAL, "audio_spectrum: the rows must be 4-byte aligned");
    if (a.fill_in == a.fill_out || a.carry_in == a.carry_out) return fail(FMRX_EINVAL, "audio_spectrum: one state buffer is read, another written");
    const bool pair = a.n <= kPairMax;
    if (!pair && !a.tiles) return fail(FMRX_EINVAL, "audio_spectrum: a row of more than 2048 samples needs the tile sums' buffer");
    const size_t n_rows = static_cast<size_t>(a.n_channels) * a.ac;
    const unsigned n = static_cast<unsigned>(a.n), N = static_cast<unsigned>(a.n_channels);
    const unsigned n_tiles = static_cast<unsigned>(audio_spectrum_tiles(a.n));   // at most 2^14
    const dim3 grid(static_cast<unsigned>(pair ? (n_rows + 1) / 2 : n_rows), pair ? 1u : n_tiles);
#define FMRX_AS_LAUNCH(AC, PAIR)                                                                                                              \
    audio_spectrum_kernel<AC, PAIR><<<grid, kThreads, 0, s>>>(a.x, a.pitch, n, N, a.edges, a.n_bands, a.fill_in, a.carry_in, a.fill_out, a.carry_out, \
                                                              a.frames, a.res, a.tiles)
    if (a.ac == 2 && pair) FMRX_AS_LAUNCH(2, true);
    else if (a.ac == 2) FMRX_AS_LAUNCH(2, false);
    else if (pair) FMRX_AS_LAUNCH(1, true);
    else FMRX_AS_LAUNCH(1, false);
#undef FMRX_AS_LAUNCH
    FMRX_LAUNCH_CHECK("audio_spectrum_kernel<%d,%d>", a.ac, pair ? 1 : 0);
    if (!pair) {
        const unsigned blocks = static_cast<unsigned>((n_rows * a.n_bands + kThreads - 1) / kThreads);
        if (a.ac == 2) audio_spectrum_sum_kernel<2><<<blocks, kThreads, 0, s>>>(a.tiles, n_tiles, N, a.n_bands, a.res);
        else audio_spectrum_sum_kernel<1><<<blocks, kThreads, 0, s>>>(a.tiles, n_tiles, N, a.n_bands, a.res);
        FMRX_LAUNCH_CHECK("audio_spectrum_sum_kernel<%d>", a.ac);
    }
    return FMRX_OK;
}

}  // namespace fmrx
