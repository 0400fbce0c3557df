// kernels_audio_resample.hip -- the kernel of the audio rate converter (include/fmrx.h: fmrx_audio_resample_*; DESIGN.md section
// 4.19; defined by tests/_audio_resample_model.py).
//
// A polyphase FIR at a rational rate: parallel in time, so the outputs of a row are tiled.  The channel rides in the grid's x
// (banks have more than 65 535 receivers), a tile of tile_out outputs of its rows in y: 1 024 where the window they read fits
// kWinMax floats per row, fewer at steep decimations.  The tiles cover all m_max outputs of the handle: a tile beyond the call's
// count M only stores zeros, so the results need no clear in front of the launch.
//
// A workgroup stages the tap table ([up][taps] floats, at most 64 KiB) and, per converted row, the tile's input window in LDS: the
// samples from the newest input of its first output less T - 1 to the newest input of its last, sample wbase + m at dword m with
// wbase a multiple of 4, so that the 16-byte pieces of an aligned row stay aligned.  In front of the call's first sample stands the
// channel's carried state.  With a mix the two rows are added and halved on the way into LDS (the carried samples are mixed ones
// already).  Rows that are 16-byte aligned (the base is, and the pitch is a multiple of 4) are fetched in 16-byte pieces, all
// others 4 bytes per lane, the same arithmetic; no load reaches past sample n of a row or past the last row: the pieces of a
// 16-byte fetch that would are fetched singly.
//
// A lane runs two outputs per step, q and q + 256, in the halves of packed fmas (audio_resample_core.hpp's step4): consecutive
// lanes hold consecutive outputs, so their sample reads step by down / up dwords through the LDS banks and their stores are
// contiguous.  An output's position is t = pos + q down, 64-bit for the tile's first output and 32-bit relative to it inside the
// tile.  For up = 1 both halves read the same taps.  The chains run over exactly T taps, T a multiple of 4: nothing is padded.
//
// The state is read from one pair of buffers and written to another (the host swaps them per call) by the workgroup of a
// channel's first tile, which fetches the row's last T - 1 samples (or, in a short call, the carried ones in front of them)
// itself: the last tile's window need not hold them all.  No workgroup reads what another writes.  Every store is a plain vector
// store.
//
// LDS and occupancy: 4 (up taps + R cap) bytes, cap the window's dwords.  48 -> 16 kHz mono mix: 0.3 + 12.3 KiB, so the 7 waves per
// SIMD that 72 VGPRs allow (7 workgroups per CU) are what bounds it; 48 -> 44.1 kHz per row: 16.1 + 2 x 4.5 KiB, 6 workgroups;
// 44.1 -> 16 kHz: 42.5 + 11.3 KiB, 2 workgroups; a 64 KiB table with two full windows (112 KiB) 1.  Resources
// (-Rpass-analysis=kernel-resource-usage, gfx950): profiles/audio_resample/kernel_resource_usage.txt; no variant uses scratch.
#include "fmrx_internal.hpp"
#include "audio_resample_core.hpp"
#include "device_math.hpp"

namespace fmrx {
namespace {

using audio_resample::f2;
using audio_resample::f4;

constexpr int kThreads = 256;
constexpr unsigned kTileOutMax = 1024;   // outputs of a tile: two steps of 2 x 256
constexpr unsigned kWinMax = 6144;       // floats of a row's window in LDS, at most

// the dwords of a tile's window: the span of the newest inputs of tile_out outputs, T - 1 in front, 3 for wbase's rounding down,
// rounded up to whole 16-byte pieces
unsigned window_cap(unsigned up, unsigned down, unsigned taps, unsigned tile_out)
{
    const unsigned span = static_cast<unsigned>((static_cast<uint64_t>(tile_out - 1) * down + (up - 1)) / up) + 1;   // i of the last less i of the first, + 1, at most
    return (span + (taps - 1) + 3 + 3) / 4 * 4;
}

template <int AC, int R, int VEC>
__global__ __launch_bounds__(kThreads) void audio_resample_kernel(const float *__restrict__ x, size_t pitch, unsigned n_audio, unsigned n_channels,
                                                                  unsigned U, unsigned D, unsigned T, const float *__restrict__ taps,
                                                                  const unsigned *__restrict__ pos_in, const float *__restrict__ carry_in,
                                                                  unsigned *__restrict__ pos_out, float *__restrict__ carry_out, size_t m_max,
                                                                  unsigned tile_out, unsigned cap, float *__restrict__ out_f32,
                                                                  int16_t *__restrict__ out_pcm, int wrap, unsigned *__restrict__ counts)
{
    static_assert(R == 1 || R == AC, "the mono mix or every row");
    constexpr bool kMix = AC == 2 && R == 1;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *const sh = lds;                                  // [U][T]
    float *const sw = lds + static_cast<size_t>(U) * T;     // [R][cap]
    const size_t ch = blockIdx.x;
    const int tid = static_cast<int>(threadIdx.x);
    const long n = static_cast<long>(n_audio);
    const int C = static_cast<int>(T) - 1;                  // carried samples per row
    const unsigned pos = pos_in[ch];
    const uint64_t M = audio_resample::outputs_of(n_audio, U, D, pos);
    const uint64_t q0 = static_cast<uint64_t>(blockIdx.y) * tile_out;                       // the tile's first output
    const uint64_t q_end = q0 + tile_out < m_max ? q0 + tile_out : m_max;                   // behind its last entry of the results
    const unsigned live = q0 >= M ? 0u : static_cast<unsigned>((M < q_end ? M : q_end) - q0);   // its outputs that the call completes

    const float *const row0 = x + ch * AC * pitch;
    const float *const st0 = carry_in + ch * R * C;
    // sample p of converted row r's stream: the row (mixed), the carried state in front of it, nothing behind it
    const auto one = [&](int r, long p) -> float {
        if (p >= n) return 0.0f;
        if (p >= 0) return kMix ? audio_resample::mono_mix(row0[p], row0[pitch + p]) : row0[r * pitch + p];
        return p >= -C ? st0[r * C + (p + C)] : 0.0f;
    };

    // the next call's state, by the channel's first tile: the streams' last T - 1 samples, the position, and the count
    if (blockIdx.y == 0) {
        for (int k = tid; k < R * C; k += kThreads) {
            const int r = k / C, j = k % C;
            carry_out[ch * R * C + k] = one(r, n - C + j);
        }
        if (tid == 0) {
            pos_out[ch] = static_cast<unsigned>(pos + M * D - static_cast<uint64_t>(n_audio) * U);
            counts[ch] = static_cast<unsigned>(M);
        }
    }

    if (live > 0) {   // uniform over the workgroup
        // the tile's first output: t = pos + q0 D; its newest input i_first and phase; outputs inside the tile count from there
        const uint64_t t_first = pos + q0 * D;
        const long i_first = static_cast<long>(t_first / U);
        const unsigned p_first = static_cast<unsigned>(t_first % U);
        const long w0 = i_first - C;
        const long wbase = w0 - (((w0 % 4) + 4) % 4);       // a multiple of 4, at most 3 below
        const unsigned i_span = static_cast<unsigned>((p_first + static_cast<uint64_t>(live - 1) * D) / U);   // newest input of the last output, less i_first
        const int used = static_cast<int>(i_first - wbase) + static_cast<int>(i_span) + 1;                   // dwords of the window, <= cap

        for (int m = tid * 4; m < static_cast<int>(U * T); m += kThreads * 4) *reinterpret_cast<f4 *>(&sh[m]) = *reinterpret_cast<const f4 *>(&taps[m]);
        if (VEC == 4) {
            for (int q = tid; q < (used + 3) / 4; q += kThreads) {
                const long p0 = wbase + 4 * q;
                if (p0 >= 0 && p0 + 4 <= n) {
                    if (kMix) {
                        const f4 a = *reinterpret_cast<const f4 *>(row0 + p0), b = *reinterpret_cast<const f4 *>(row0 + pitch + p0);
                        f4 v;
#pragma unroll
                        for (int i = 0; i < 4; i++) v[i] = audio_resample::mono_mix(a[i], b[i]);
                        *reinterpret_cast<f4 *>(&sw[4 * q]) = v;
                    } else {
#pragma unroll
                        for (int r = 0; r < R; r++) *reinterpret_cast<f4 *>(&sw[r * cap + 4 * q]) = *reinterpret_cast<const f4 *>(row0 + r * pitch + p0);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < R; r++) {
                        f4 v;
#pragma unroll
                        for (int i = 0; i < 4; i++) v[i] = one(r, p0 + i);
                        *reinterpret_cast<f4 *>(&sw[r * cap + 4 * q]) = v;
                    }
                }
            }
        } else {
            for (int m = tid; m < used; m += kThreads) {
#pragma unroll
                for (int r = 0; r < R; r++) sw[r * cap + m] = one(r, wbase + m);
            }
        }
        __syncthreads();

        const int lbase = static_cast<int>(i_first - wbase);    // the dword of x[i_first]
        const bool one_phase = U == 1;
        for (unsigned k0 = 0; k0 < live; k0 += 2 * kThreads) {
            const unsigned ka = k0 + tid, kb = ka + kThreads;   // the tile's outputs of this lane
            const bool has_a = ka < live, has_b = kb < live;
            if (!has_a) break;                                  // (then not has_b either)
            const unsigned ta = p_first + ka * D, tb = p_first + (has_b ? kb : ka) * D;   // < 2^10 tile_out + up: 32-bit
            const unsigned ia = ta / U, pa = ta - ia * U, ib = tb / U, pb = tb - ib * U;
            const float *const ha = sh + pa * T, *const hb = sh + pb * T;
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float *const xa = sw + r * cap + lbase + ia, *const xb = sw + r * cap + lbase + ib;   // the newest inputs
                f2 acc = {0.0f, 0.0f};
                for (int j = 0; j < static_cast<int>(T); j += 4) {
                    const f4 va = *reinterpret_cast<const f4 *>(ha + j);
                    const f4 vb = one_phase ? va : *reinterpret_cast<const f4 *>(hb + j);
                    const float sa[4] = {xa[-j], xa[-j - 1], xa[-j - 2], xa[-j - 3]}, sb[4] = {xb[-j], xb[-j - 1], xb[-j - 2], xb[-j - 3]};
                    acc = audio_resample::step4(acc, va, vb, sa, sb);
                }
                const size_t o = (ch * R + r) * m_max + q0;
                if (out_f32) {
                    out_f32[o + ka] = acc[0];
                    if (has_b) out_f32[o + kb] = acc[1];
                }
                if (out_pcm) {
                    out_pcm[o + ka] = pcm_pack(acc[0], wrap);
                    if (has_b) out_pcm[o + kb] = pcm_pack(acc[1], wrap);
                }
            }
        }
    }

    // entries of the results at and beyond the call's count: +0 / 0
    const unsigned entries = static_cast<unsigned>(q_end - q0);
    for (unsigned k = live + tid; k < entries; k += kThreads) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const size_t o = (ch * R + r) * m_max + q0 + k;
            if (out_f32) out_f32[o] = 0.0f;
            if (out_pcm) out_pcm[o] = 0;
        }
    }
}

template <int AC, int R, int VEC>
int launch_as(const AudioResampleArgs &a, dim3 grid, unsigned cap, size_t lds, hipStream_t s)
{
    const auto kernel = &audio_resample_kernel<AC, R, VEC>;
    if (lds > 48 * 1024) FMRX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)));
    kernel<<<grid, kThreads, lds, s>>>(a.x, a.pitch, static_cast<unsigned>(a.n), static_cast<unsigned>(a.n_channels), a.up, a.down, a.taps, a.h, a.pos_in,
                                       a.carry_in, a.pos_out, a.carry_out, a.m_max, a.tile_out, cap, a.out_f32, a.out_pcm, a.wrap, a.counts);
    FMRX_LAUNCH_CHECK("audio_resample_kernel<%d,%d,%d>", AC, R, VEC);
    return FMRX_OK;
}

}  // namespace

unsigned audio_resample_tile_out(unsigned up, unsigned down, unsigned taps)
{
    // the most outputs whose window fits kWinMax: span <= (tile_out - 1) down / up + 2
    const uint64_t room = kWinMax - (taps - 1) - 6 - 2;
    const uint64_t t = 1 + room * up / down;
    unsigned tile = static_cast<unsigned>(t < kTileOutMax ? t : kTileOutMax);
    while (tile > 1 && window_cap(up, down, taps, tile) > kWinMax) tile--;
    return tile;
}

int audio_resample_launch(const AudioResampleArgs &a, hipStream_t s)
{
    if (!a.x || !a.h || !a.pos_in || !a.carry_in || !a.pos_out || !a.carry_out || !a.counts) return fail(FMRX_EINVAL, "audio_resample: null buffer");
    if (!a.out_f32 && !a.out_pcm) return fail(FMRX_EINVAL, "audio_resample: neither float nor PCM output");
    if (a.n_channels < 1 || (a.ac != 1 && a.ac != 2) || (a.rows != 1 && a.rows != a.ac)) return fail(FMRX_EINVAL, "audio_resample: n_channels >= 1, audio_channels 1 or 2, rows 1 or audio_channels");
    if (a.n < 1 || a.n > (size_t{1} << 26) || a.pitch < a.n) return fail(FMRX_EINVAL, "audio_resample: 1 .. 2^26 samples per row, in a pitch that holds them");
    if (reinterpret_cast<uintptr_t>(a.x) % sizeof(float)) return fail(FMRX_EINVAL, "audio_resample: the rows must be 4-byte aligned");
    if (a.pos_in == a.pos_out || a.carry_in == a.carry_out) return fail(FMRX_EINVAL, "audio_resample: one state buffer is read, another written");
    if (a.up < 1 || a.up > audio_resample::kMaxUp || a.down < 1 || a.down > audio_resample::kMaxDown || a.taps < audio_resample::kMinTaps ||
        a.taps > audio_resample::kMaxTaps || a.taps % 4 || a.up * a.taps > audio_resample::kMaxTable)
        return fail(FMRX_EINVAL, "audio_resample: up %u, down %u, taps %u", a.up, a.down, a.taps);
    if (a.tile_out < 1 || a.tile_out > kTileOutMax || window_cap(a.up, a.down, a.taps, a.tile_out) > kWinMax)
        return fail(FMRX_EINVAL, "audio_resample: a tile of %u outputs", a.tile_out);
    if (a.m_max < audio_resample::max_out(a.n, a.up, a.down)) return fail(FMRX_EINVAL, "audio_resample: results of %zu outputs per row", a.m_max);
    const size_t tiles = (a.m_max + a.tile_out - 1) / a.tile_out;
    if (tiles > 65535) return fail(FMRX_EINVAL, "audio_resample: %zu tiles per row exceed a grid", tiles);
    const unsigned cap = window_cap(a.up, a.down, a.taps, a.tile_out);
    const size_t lds = (static_cast<size_t>(a.up) * a.taps + static_cast<size_t>(a.rows) * cap) * sizeof(float);
    const bool wide = reinterpret_cast<uintptr_t>(a.x) % 16 == 0 && a.pitch % 4 == 0;
    const dim3 grid(static_cast<unsigned>(a.n_channels), static_cast<unsigned>(tiles));
    if (a.ac == 1) return wide ? launch_as<1, 1, 4>(a, grid, cap, lds, s) : launch_as<1, 1, 1>(a, grid, cap, lds, s);
    if (a.rows == 1) return wide ? launch_as<2, 1, 4>(a, grid, cap, lds, s) : launch_as<2, 1, 1>(a, grid, cap, lds, s);
    return wide ? launch_as<2, 2, 4>(a, grid, cap, lds, s) : launch_as<2, 2, 1>(a, grid, cap, lds, s);
}

}  // namespace fmrx
