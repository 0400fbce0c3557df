// kernels_audio_features.hip -- the kernel of the audio feature frames (include/fmrx.h: fmrx_audio_features_*; DESIGN.md section
// 4.18; defined by tests/_audio_features_model.py).
//
// A frame's 2 x n_bins chains are one matrix product: the M rows are the outputs (re_k and im_k), K the win window positions,
// the N columns 16 frames.  v_mfma_f32_16x16x4_f32 adds its 4 products to an accumulator as a chain of exactly rounded fmaf in K
// order, so win / 4 dependent instructions whose K index is j = 4 s + kq (s the instruction, kq the K index inside it) are the
// model's chain over j ascending.  Operands (lane = 16 kq + i):
//   A  lane (i, kq) of instruction s holds the cosine of output row i at window position j = 4 s + kq: C[(k j) mod win] for re_k,
//      C[(k j - win/4) mod win] for im_k, read as one pair from the table in LDS; the index advances by 4 k mod win per
//      instruction: an add and a conditional subtract, win being no power of two
//   B  lane (i, kq) holds xw[j = 4 s + kq] of frame (column) i; the windowed frames stand in LDS as [column][kq][s], so that four
//      instructions' operands are one 16-byte read
//   D  lane (i, kq) holds rows 4 kq .. 4 kq + 3 of column i
// A wave owns the re tile and the im tile of 2 x 16 bins: four independent accumulators, 128 cycles of issue between the
// dependent ones, and re_k and im_k of a frame in one lane, so that p_k needs no exchange.  A workgroup has as many waves as
// the geometry has pairs of bin tiles (7 for 201 bins, at most 8), each over all win positions of the same 16 columns.
//
// The columns of a workgroup are 16 consecutive entries of the flattened list (channel, frame q < F_max): a tile spans several
// channels of a bank, and one long row spreads over many tiles with no second launch, every frame's output being independent.
// A column whose channel completed no frame q (or that lies behind the last channel) stages zeros and stores +0.
//
// K comes in slices of 320 window positions (the chain's order does not care when a slice arrives): m w of the 16 columns' slice
// stands in one of two LDS buffers (stream position p of a channel is its carried samples, then the mono mix of the call's;
// overlapping frames window the same samples again; the loads are 4 bytes per lane, consecutive lanes consecutive samples, at
// any alignment).  The next slice is staged in front of the matrix work on the current one, in batches of 6 elements per lane
// whose loads -- both rows, no branch around a load -- are issued together; the workgroup's matrix cores idle for that long, and
// the CU's other workgroup has them: the kernel is held to 128 registers and 80 KiB of LDS so that two are resident.  The
// p_k go to LDS and the mel chains run from there, one lane per (column, mel).  No load reaches past sample n of a row, past
// the last row or past fill of the carried state: an element that is not wanted loads the window table's first entry instead.
//
// The carried state (fill and the mono mix behind the last completed frame's hop, per channel) is read from one pair of buffers
// and written to another, which the host swaps per call, by the workgroup that holds the channel's column q = 0: no workgroup
// reads what another writes.  Every store is a plain vector store.
//
// LDS: two slices of 16 columns x 4 x 84 floats of m w (42 KiB), the cosine pairs (10.3 KiB), the window (5 KiB) and the bin
// powers (16.3 KiB): two workgroups per CU, one staging while the other multiplies.  Resources
// (-Rpass-analysis=kernel-resource-usage, gfx950): profiles/audio_features/; the kernel uses no scratch.
#include "fmrx_internal.hpp"
#include "audio_features_core.hpp"

namespace fmrx {
namespace {

using f4 = float __attribute__((ext_vector_type(4)));
using f2 = float __attribute__((ext_vector_type(2)));

constexpr int kMaxWin = audio_features::kMaxWin, kMaxBins = audio_features::kMaxBins, kTile = audio_features::kTile;
constexpr int kMaxWaves = kMaxBins / 32, kMaxThreads = 64 * kMaxWaves;
constexpr int kSlice = 320;                   // window positions staged at a time
constexpr int kSliceSteps = kSlice / 4;       // matrix instructions of a slice's piece of a chain
constexpr int kSliceElems = kTile * kSlice;   // (column, position) elements of a slice
constexpr int kAhead = 6;                     // elements a lane fetches at a time: a slice is two such batches for 7 waves
constexpr int kXwPitch = kSliceSteps + 4;     // floats per (column, kq) in LDS: 16-byte pieces stay aligned, the lanes' reads spread over the banks
constexpr int kXwBuf = kTile * 4 * kXwPitch;  // floats of one slice buffer
constexpr int kPowPitch = kMaxBins + 4;       // floats per column of bin powers
// The cosine table in LDS: entry m holds the pair (C[m], C[(m - win/4) mod win]), the A operands of re_k and im_k at one angle, one
// 8-byte read.  Entry m stands in slot m + m / 32, the spectrum meter's skew: 16 consecutive bins at a stride of 4 k entries
// meet different slots where the stride alone would fold them onto a few.
constexpr int kCosSlots = kMaxWin + kMaxWin / 32;
__device__ __forceinline__ int cos_slot(int m) { return m + (m >> 5); }
constexpr unsigned kNoChannel = 0xffffffffu;
static_assert(kMaxWin % 4 == 0 && kSlice % 16 == 0 && kAhead <= 32, "slices of whole 16-byte pieces; one mask bit per fetched element");

struct Params {
    const float *x;
    size_t pitch, f_max;
    unsigned n, n_channels;
    int win, hop, n_bins, n_mels;
    const float *w, *c, *mel_w;
    const int *mel_lo, *mel_hi;
    const unsigned *fill_in;
    const float *carry_in;
    unsigned *fill_out;
    float *carry_out;
    unsigned *frames;
    float *feat;
};

template <int AC>
__global__ __launch_bounds__(kMaxThreads) __attribute__((amdgpu_waves_per_eu(4))) void audio_features_kernel(const Params P)
{
    __shared__ __attribute__((aligned(16))) float xw[2 * kXwBuf];
    __shared__ __attribute__((aligned(16))) float pw[kTile * kPowPitch];
    __shared__ __attribute__((aligned(8))) f2 ct[kCosSlots];
    __shared__ float sw[kMaxWin];
    // the columns: channel (kNoChannel behind the last), frame q of the call, the channel's fill and completed frames F
    __shared__ unsigned col_ch[kTile];
    __shared__ int col_q[kTile], col_fill[kTile], col_F[kTile];

    const int tid = static_cast<int>(threadIdx.x), nthr = static_cast<int>(blockDim.x);
    const int win = P.win, hop = P.hop, n = static_cast<int>(P.n);
    const size_t N = P.n_channels, total = N * P.f_max;
    const size_t g0 = static_cast<size_t>(blockIdx.x) * kTile;

    // the cosine pairs and the window
    for (int m = tid; m < win; m += nthr) {
        const int mi = m - win / 4;
        ct[cos_slot(m)] = (f2){P.c[m], P.c[mi < 0 ? mi + win : mi]};
        sw[m] = P.w[m];
    }
    if (tid < kTile) {
        const size_t g = g0 + tid;
        const bool has = g < total;
        const size_t ch = has ? g / P.f_max : 0;
        int fill = 0, F = 0;
        if (has) {
            const unsigned f = P.fill_in[ch];
            fill = static_cast<int>(f < static_cast<unsigned>(win) ? f : static_cast<unsigned>(win - 1));
            F = static_cast<int>(audio_features::frames_of(static_cast<unsigned>(fill + n), static_cast<unsigned>(win), static_cast<unsigned>(hop)));
        }
        col_ch[tid] = has ? static_cast<unsigned>(ch) : kNoChannel;
        col_q[tid] = has ? static_cast<int>(g % P.f_max) : 0;
        col_fill[tid] = fill;
        col_F[tid] = F;
    }
    __syncthreads();

    // where stream position p < fill + n of channel ch stands: among the carried samples, or in the call's rows (the first of them)
    const auto carried = [&](unsigned ch, int p) { return P.carry_in + static_cast<size_t>(ch) * win + p; };
    const auto fresh = [&](unsigned ch, int fill, int p) { return P.x + static_cast<size_t>(ch) * AC * P.pitch + static_cast<size_t>(p - fill); };
    const auto mix = [&](const float *at) { return AC == 2 ? audio_features::mono_mix(at[0], at[P.pitch]) : at[0]; };

    // the next call's state, by the workgroup of the channel's first column: the samples behind the last completed hop
    int live = 0;
    for (int c = 0; c < kTile; c++) {
        const unsigned ch = col_ch[c];
        if (ch == kNoChannel) break;
        const int q = col_q[c], fill = col_fill[c], F = col_F[c];
        live += q < F ? 1 : 0;
        if (q != 0) continue;
        const int start = F * hop, left = fill + n - start;
        float *out = P.carry_out + static_cast<size_t>(ch) * win;
        for (int e = tid; e < left; e += nthr) {
            const int p = start + e;
            out[e] = p < fill ? *carried(ch, p) : mix(fresh(ch, fill, p));
        }
        if (tid == 0) {
            P.fill_out[ch] = static_cast<unsigned>(left);
            P.frames[ch] = static_cast<unsigned>(F);
        }
    }

    if (live > 0) {
        // element e of a slice: column e div 320, position j0 + e mod 320; m w goes to [column][kq = j mod 4][s = (j - j0) div 4]
        // wanted: the position lies inside the window and the column is live
        const auto place = [&](int e, int j0, int &c, int &j, bool &wanted) {
            c = e / kSlice;
            const int jj = e - c * kSlice;
            j = j0 + jj;
            wanted = j < win && col_ch[c] != kNoChannel && col_q[c] < col_F[c];
            return c * 4 * kXwPitch + (jj & 3) * kXwPitch + (jj >> 2);
        };
        float ra[kAhead], rb[kAhead];
        unsigned want_mask = 0, carry_mask = 0;
        // the loads of a batch of kAhead elements per lane, all issued before any is waited for
        const auto fetch = [&](int j0, int base) {
            want_mask = carry_mask = 0;
#pragma unroll
            for (int u = 0; u < kAhead; u++) {
                const int e = base + tid + u * nthr;
                int c = 0, j = 0;
                bool wanted = false;
                if (e < kSliceElems) place(e, j0, c, j, wanted);
                const float *at = P.w, *bt = P.w;
                if (wanted) {
                    const unsigned ch = col_ch[c];
                    const int fill = col_fill[c], p = col_q[c] * hop + j;
                    if (p < fill) {
                        at = bt = carried(ch, p);
                        carry_mask |= 1u << u;
                    } else {
                        at = fresh(ch, fill, p);
                        bt = at + P.pitch;
                    }
                    want_mask |= 1u << u;
                }
                ra[u] = *at;
                rb[u] = AC == 2 ? *bt : 0.0f;
            }
        };
        // ... and stored
        const auto stage = [&](int j0, int base, float *buf) {
#pragma unroll
            for (int u = 0; u < kAhead; u++) {
                const int e = base + tid + u * nthr;
                if (e >= kSliceElems) continue;
                int c, j;
                bool wanted;
                const int at = place(e, j0, c, j, wanted);
                float m = ra[u];
                if (AC == 2 && !((carry_mask >> u) & 1u)) m = audio_features::mono_mix(ra[u], rb[u]);
                if (j < win) buf[at] = (want_mask >> u) & 1u ? m * sw[j] : 0.0f;
            }
        };
        // a slice: in batches of kAhead elements per lane
        const auto slice = [&](int j0, float *buf) {
            for (int base = 0; base < kSliceElems; base += kAhead * nthr) {
                fetch(j0, base);
                stage(j0, base, buf);
            }
        };

        const int lane = tid & 63, wv = tid >> 6;
        const int i = lane & 15, kq = lane >> 4;
        f4 re[2], im[2];
        int idx[2], step[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int k = 32 * wv + 16 * t + i;      // the bin of this lane's row of A (rows from n_bins on are computed and not read)
            re[t] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
            im[t] = re[t];
            idx[t] = (k * kq) % win;
            step[t] = (4 * k) % win;
        }
        const auto one = [&](float b) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const f2 a = ct[cos_slot(idx[t])];
                re[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b, re[t], 0, 0, 0);
                im[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b, im[t], 0, 0, 0);
                idx[t] += step[t];
                if (idx[t] >= win) idx[t] -= win;
            }
        };

        const int steps = win >> 2, n_slices = (win + kSlice - 1) / kSlice;
        slice(0, xw);
        __syncthreads();
        for (int s = 0; s < n_slices; s++) {
            const bool more = s + 1 < n_slices;
            if (more) slice((s + 1) * kSlice, xw + ((s + 1) & 1) * kXwBuf);
            const float *bcol = xw + (s & 1) * kXwBuf + (i * 4 + kq) * kXwPitch;
            const int here = steps - s * kSliceSteps < kSliceSteps ? steps - s * kSliceSteps : kSliceSteps;
            const int groups = here >> 2, tail = here & 3;
            for (int s4 = 0; s4 < groups; s4++) {
                const f4 b = *reinterpret_cast<const f4 *>(bcol + 4 * s4);
#pragma unroll
                for (int e = 0; e < 4; e++) one(b[e]);
            }
            if (tail > 0) {      // the piece's entries from `tail` on lie inside the pitch and are not used
                const f4 b = *reinterpret_cast<const f4 *>(bcol + 4 * groups);
#pragma unroll
                for (int e = 0; e < 3; e++)
                    if (e < tail) one(b[e]);
            }
            __syncthreads();
        }
        // this lane: column i, bins 32 wv + 16 t + 4 kq + v
#pragma unroll
        for (int t = 0; t < 2; t++) {
            f4 p;
#pragma unroll
            for (int v = 0; v < 4; v++) p[v] = audio_features::bin_power(re[t][v], im[t][v]);
            *reinterpret_cast<f4 *>(pw + i * kPowPitch + 32 * wv + 16 * t + 4 * kq) = p;
        }
    }
    __syncthreads();

    // the mel chains, one lane per (mel, column): 16 neighbouring lanes share a filter; a dead column stores +0
    for (int task = tid; task < P.n_mels * kTile; task += nthr) {
        const int b = task >> 4, c = task & (kTile - 1);
        if (col_ch[c] == kNoChannel) continue;
        float v = 0.0f;
        if (col_q[c] < col_F[c]) v = audio_features::mel_chain(P.mel_w + static_cast<size_t>(b) * P.n_bins, pw + c * kPowPitch, P.mel_lo[b], P.mel_hi[b]);
        P.feat[(g0 + c) * P.n_mels + b] = v;
    }
}

}  // namespace

size_t audio_features_tiles(size_t n_channels, size_t f_max) { return (n_channels * f_max + kTile - 1) / kTile; }

int audio_features_launch(const AudioFeaturesArgs &a, hipStream_t s)
{
    if (!a.x || !a.w || !a.c || !a.mel_w || !a.mel_lo || !a.mel_hi || !a.fill_in || !a.carry_in || !a.fill_out || !a.carry_out || !a.frames || !a.feat)
        return fail(FMRX_EINVAL, "audio_features: null buffer");
    if (a.n_channels < 1 || (a.ac != 1 && a.ac != 2)) return fail(FMRX_EINVAL, "audio_features: n_channels >= 1, audio_channels 1 or 2");
    if (a.win < 16 || a.win > kMaxWin || a.win % 4 || a.hop < 1 || a.hop > a.win || a.n_bins < 1 || a.n_bins > kMaxBins || a.n_bins > a.win / 2 ||
        a.n_mels < 1 || a.n_mels > audio_features::kMaxMels)
        return fail(FMRX_EINVAL, "audio_features: geometry win %d hop %d n_bins %d n_mels %d", a.win, a.hop, a.n_bins, a.n_mels);
    if (a.n < 1 || a.n > (size_t{1} << 26) || a.pitch < a.n) return fail(FMRX_EINVAL, "audio_features: 1 .. 2^26 samples per row, in a pitch that holds them");
    if (a.f_max < audio_features::max_frames(a.n, static_cast<unsigned>(a.hop))) return fail(FMRX_EINVAL, "audio_features: %zu frames per channel do not hold a call of %zu samples", a.f_max, a.n);
    if (reinterpret_cast<uintptr_t>(a.x) % sizeof(float)) return fail(FMRX_EINVAL, "audio_features: the rows must be 4-byte aligned");
    if (a.fill_in == a.fill_out || a.carry_in == a.carry_out) return fail(FMRX_EINVAL, "audio_features: one state buffer is read, another written");
    const size_t tiles = audio_features_tiles(a.n_channels, a.f_max);
    if (tiles > 0x7fffffffu) return fail(FMRX_EINVAL, "audio_features: %zu tiles of 16 frames exceed a grid", tiles);
    Params p;
    p.x = a.x;
    p.pitch = a.pitch;
    p.f_max = a.f_max;
    p.n = static_cast<unsigned>(a.n);
    p.n_channels = static_cast<unsigned>(a.n_channels);
    p.win = a.win;
    p.hop = a.hop;
    p.n_bins = a.n_bins;
    p.n_mels = a.n_mels;
    p.w = a.w;
    p.c = a.c;
    p.mel_w = a.mel_w;
    p.mel_lo = a.mel_lo;
    p.mel_hi = a.mel_hi;
    p.fill_in = a.fill_in;
    p.carry_in = a.carry_in;
    p.fill_out = a.fill_out;
    p.carry_out = a.carry_out;
    p.frames = a.frames;
    p.feat = a.feat;
    const unsigned threads = 64u * static_cast<unsigned>(((a.n_bins + 15) / 16 + 1) / 2);   // a wave per pair of bin tiles
    const unsigned grid = static_cast<unsigned>(tiles);
    if (a.ac == 2) audio_features_kernel<2><<<grid, threads, 0, s>>>(p);
    else audio_features_kernel<1><<<grid, threads, 0, s>>>(p);
    FMRX_LAUNCH_CHECK("audio_features_kernel<%d>", a.ac);
    return FMRX_OK;
}

}  // namespace fmrx
