// kernels_true_peak.hip -- the kernel of the true-peak meter (include/fmrx.h: fmrx_true_peak_*; defined
// by tests/_true_peak_model.py).
//
// A short FIR and a maximum: parallel in time, so the row is tiled.  The channel rides in the grid's x (banks have more than
// 65 535 receivers), a tile of kTile = 2048 samples of its rows in y; one 1 920-sample bank row is one workgroup.  A workgroup
// stages, per row, the tile and the kCarry = 11 samples in front of it in LDS: sample k0 - 12 + m at dword m, so that the tile's
// 16-byte pieces stay aligned.  In front of the call's first sample stands the channel's carried state.  Rows that are 16-byte
// aligned (the base is, and the pitch is a multiple of 4) are fetched in 16-byte pieces, all others 4 bytes per lane, the same
// arithmetic; no load reaches past sample n of a row or past the last row: the pieces of a 16-byte fetch that would are
// fetched singly, and what lies past n reads 0 and enters no group that counts.
//
// A lane evaluates kRun = 8 consecutive groups per row from registers: five aligned 16-byte LDS reads give it the 19 samples
// they span, true_peak_core.hpp's run<8> the 8 x 3 chains, two neighbouring groups to a packed fma, the 18 distinct taps as
// literals.  The maxima and the over count are reduced across the wave and, through LDS, across the workgroup's four waves.  The
// results are field-major [field][n_channels] and cleared on the stream in front of the launch.  A row of one tile (every bank
// row of 1 920 samples) has one workgroup, which stores them plainly.  The tiles of a longer row meet in one atomicMax per
// reading on the bits of the non-negative float (monotone, +infinity included; a NaN never enters a maximum) and one integer
// atomicAdd: per workgroup, not per wave -- atomics on one address take their turns at the L2, and with one set per wave
// they were what a single long row's time consisted of.
//
// The state is read from one buffer by a call's first tile and written to another by its last (the host swaps them per call),
// out of LDS, where a short call's old entries stand too: no workgroup reads what another writes.  Everything but those
// atomics is a plain vector store.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 4.16; no variant uses scratch.
#include "fmrx_internal.hpp"
#include "true_peak_core.hpp"

namespace fmrx {
namespace {

using f4 = float __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = true_peak::kTile, kRun = true_peak::kRun, kCarry = true_peak::kCarry;
constexpr int kFront = 12;                 // dwords in front of the tile in LDS: the carry and one, a multiple of 4
constexpr int kSpan = kFront + kTile;
static_assert(kTile == kRun * kThreads, "a workgroup's lanes own the tile");
static_assert(kFront >= kCarry && kFront % 4 == 0 && kRun % 4 == 0, "aligned 16-byte pieces");

template <int AC, int VEC>
__global__ __launch_bounds__(kThreads) void true_peak_kernel(const float *__restrict__ x, size_t pitch, unsigned n_audio, unsigned n_channels,
                                                             float limit, const float *__restrict__ state_in, float *__restrict__ state_out,
                                                             unsigned *__restrict__ res)
{
    __shared__ __attribute__((aligned(16))) float s[AC][kSpan];
    __shared__ unsigned red[kWaves][kTruePeakFields];
    const size_t ch = blockIdx.x, N = n_channels;
    const int tid = static_cast<int>(threadIdx.x);
    const long n = static_cast<long>(n_audio);
    const long k0 = static_cast<long>(blockIdx.y) * kTile;   // the tile's first sample
    const long base = k0 - kFront;                           // the sample of dword 0: a multiple of 4

#pragma unroll
    for (int r = 0; r < AC; r++) {
        const float *row = x + (ch * AC + r) * pitch;
        const float *st = state_in + static_cast<size_t>(r * kCarry) * N + ch;
        // sample p of the stream: the row, the carried state in front of it, nothing behind it
        const auto one = [&](long p) -> float { return p >= n ? 0.0f : (p >= 0 ? row[p] : (p >= -kCarry ? st[static_cast<size_t>(p + kCarry) * N] : 0.0f)); };
        if (VEC == 4) {
            for (int q = tid; q < kSpan / 4; q += kThreads) {
                const long p0 = base + 4 * q;
                f4 v;
                if (p0 >= 0 && p0 + 4 <= n) {
                    v = *reinterpret_cast<const f4 *>(row + p0);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) v[i] = one(p0 + i);
                }
                *reinterpret_cast<f4 *>(&s[r][4 * q]) = v;
            }
        } else {
            for (int m = tid; m < kSpan; m += kThreads) s[r][m] = one(base + m);
        }
    }
    __syncthreads();

    // the next call's state: the stream's last kCarry samples, by the workgroup of the call's last tile
    if (k0 + kTile >= n && tid < AC * kCarry) {
        const int r = tid / kCarry, j = tid % kCarry;
        state_out[static_cast<size_t>(r * kCarry + j) * N + ch] = s[r][(n - k0) + (kFront - kCarry) + j];
    }

    // group i of the call reads the samples i - 11 .. i: dwords i - k0 + 1 .. i - k0 + 12
    const long i0 = k0 + static_cast<long>(kRun) * tid;
    const int live = i0 >= n ? 0 : (n - i0 < kRun ? static_cast<int>(n - i0) : kRun);
    true_peak::Row acc[AC];
    if (live > 0) {
#pragma unroll
        for (int r = 0; r < AC; r++) {
            float w[kRun + kFront];
#pragma unroll
            for (int q = 0; q < (kRun + kFront) / 4; q++) {
                const f4 v = *reinterpret_cast<const f4 *>(&s[r][kRun * tid + 4 * q]);
#pragma unroll
                for (int i = 0; i < 4; i++) w[4 * q + i] = v[i];
            }
            float e[kRun + kCarry];
#pragma unroll
            for (int i = 0; i < kRun + kCarry; i++) e[i] = w[i + (kFront - kCarry)];
            true_peak::run<kRun>(e, live, limit, acc[r]);
        }
    }

    // across the wave, then across the workgroup's waves through LDS: field f = 0, 1 true_peak, 2, 3 peak, 4, 5 over, as in res
#pragma unroll
    for (int r = 0; r < AC; r++) {
        unsigned tp = __float_as_uint(acc[r].tp), pk = __float_as_uint(acc[r].pk), over = acc[r].over;   // bits of floats >= +0
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            tp = max(tp, static_cast<unsigned>(__shfl_xor(static_cast<int>(tp), off)));
            pk = max(pk, static_cast<unsigned>(__shfl_xor(static_cast<int>(pk), off)));
            over += static_cast<unsigned>(__shfl_xor(static_cast<int>(over), off));
        }
        if ((tid & 63) == 0) {
            red[tid >> 6][0 + r] = tp;
            red[tid >> 6][2 + r] = pk;
            red[tid >> 6][4 + r] = over;
        }
    }
    __syncthreads();
    if (tid < kTruePeakFields && (tid & 1) < AC) {
        unsigned v = red[0][tid];
#pragma unroll
        for (int w = 1; w < kWaves; w++) v = tid < 4 ? max(v, red[w][tid]) : v + red[w][tid];
        unsigned *out = &res[static_cast<size_t>(tid) * N + ch];
        if (gridDim.y == 1) {   // the row's only tile: a plain store
            *out = v;
        } else if (v != 0) {    // (0 is what the clear left)
            if (tid < 4) atomicMax(out, v);
            else atomicAdd(out, v);
        }
    }
}

}  // namespace

int true_peak_launch(const TruePeakArgs &a, hipStream_t s)
{
    if (!a.x || !a.state_in || !a.state_out || !a.res) return fail(FMRX_EINVAL, "true_peak: null buffer");
    if (a.n_channels < 1 || (a.ac != 1 && a.ac != 2)) return fail(FMRX_EINVAL, "true_peak: n_channels >= 1, audio_channels 1 or 2");
    if (a.n < 1 || a.n > (size_t{1} << 26) || a.pitch < a.n) return fail(FMRX_EINVAL, "true_peak: 1 .. 2^26 samples per row, in a pitch that holds them");
    if (reinterpret_cast<uintptr_t>(a.x) % sizeof(float)) return fail(FMRX_EINVAL, "true_peak: the rows must be 4-byte aligned");
    if (a.state_in == a.state_out) return fail(FMRX_EINVAL, "true_peak: one state buffer is read, another written");
    const bool wide = reinterpret_cast<uintptr_t>(a.x) % 16 == 0 && a.pitch % 4 == 0;
    const dim3 grid(static_cast<unsigned>(a.n_channels), static_cast<unsigned>((a.n + kTile - 1) / kTile));   // at most 2^15 tiles
    const unsigned n = static_cast<unsigned>(a.n), N = static_cast<unsigned>(a.n_channels);
    FMRX_HIP(hipMemsetAsync(a.res, 0, static_cast<size_t>(kTruePeakFields) * N * sizeof(unsigned), s));
    if (a.ac == 2 && wide) {
        true_peak_kernel<2, 4><<<grid, kThreads, 0, s>>>(a.x, a.pitch, n, N, a.limit, a.state_in, a.state_out, a.res);
    } else if (a.ac == 2) {
        true_peak_kernel<2, 1><<<grid, kThreads, 0, s>>>(a.x, a.pitch, n, N, a.limit, a.state_in, a.state_out, a.res);
    } else if (wide) {
        true_peak_kernel<1, 4><<<grid, kThreads, 0, s>>>(a.x, a.pitch, n, N, a.limit, a.state_in, a.state_out, a.res);
    } else {
        true_peak_kernel<1, 1><<<grid, kThreads, 0, s>>>(a.x, a.pitch, n, N, a.limit, a.state_in, a.state_out, a.res);
    }
    FMRX_LAUNCH_CHECK("true_peak_kernel<%d,%d>", a.ac, wide ? 4 : 1);
    return FMRX_OK;
}

}  // namespace fmrx
