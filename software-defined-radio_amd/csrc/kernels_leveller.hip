// kernels_leveller.hip -- the two kernels of the loudness leveller / peak limiter stage (include/fmrx.h: fmrx_leveller_*;
// DESIGN.md section 4.15; defined by tests/_leveller_model.py).
//
// leveller_control_kernel: meter_stage.hpp's control kernel with control_step of leveller_control.hpp on the channel's K-weighted
// sums, where the audio meters' pass left them.
//
// leveller_apply_kernel: the pass over the audio, 4 bytes in and 4 + 2 bytes out per sample.  The channel rides in the grid's x
// (banks have more than 65 535 receivers), a tile of T = 2048 - 2W samples of its rows in y.  A workgroup holds kSpan = 2048
// positions in LDS: 2W in front of its tile (2W - 2 of them the sliding windows' reach, 2 so that the tile starts on a 16-byte
// boundary), then the tile.  A lane owns groups of 4 consecutive positions, group t and group t + 256.
//   1. u = x g and the codes q of every position: from the rows (the positions of the tile in front are computed again, the
//      same bits), or, in front of the call's first sample, from the channel's carried state.  u goes to LDS, q to LDS and
//      stays in the lane's registers.
//   2. The sliding minimum over W positions in log2 W doubling steps, m_2d[i] = min(m_d[i], m_d[i - d]), then the sliding sum
//      the same way with +.  A lane keeps its 8 values in registers and reads the values d in front from LDS: for d = 1, 2 the
//      group in front of its own, for d >= 4 the group d in front, always one aligned 16-byte read -- consecutive lanes read
//      consecutive 16 bytes, no bank conflict.  Two LDS images alternate, so a step costs one barrier; the last step writes
//      nothing.
//   3. y = u[i - (W - 1)] * (s * 2^-24): the delayed u as two aligned 16-byte reads per row, the output as 16-byte stores (rows
//      that allow it; else 4-byte accesses, the same arithmetic) and the PCM through pcm_pack.
// The state is read from one buffer and written to another (the host swaps them per call), each entry by the lane that owns
// its position -- the first tile's lanes for the entries a short call carries forward -- so no workgroup reads what another
// writes.  min_code and limited reach the status row through one pair of vector atomics per wave that limited anything.
#include "device_math.hpp"
#include "leveller_control.hpp"
#include "meter_stage.hpp"

namespace fmrx {
namespace {

using f4 = float __attribute__((ext_vector_type(4)));
using u4 = unsigned __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kGroups = 2;   // groups of 4 positions per lane
constexpr int kSpan = leveller::kSpan;
static_assert(kSpan == 4 * kGroups * kThreads, "a workgroup's lanes own the span");

__global__ __launch_bounds__(meter_stage::kControlThreads) void leveller_control_kernel(leveller::Control c, int ac, const double *__restrict__ k2a,
                                                                                        const double *__restrict__ k2b,
                                                                                        const unsigned long long *__restrict__ n_each,
                                                                                        unsigned long long n_all,
                                                                                        fmrx_leveller_status *__restrict__ st, unsigned n_channels)
{
    meter_stage::control_body(st, n_channels, [&](unsigned i, fmrx_leveller_status &s) {
        leveller::control_step(c, ac, n_each ? n_each[i] : n_all, k2a[i], ac == 2 ? k2b[i] : 0.0, s);
    });
}

__device__ __forceinline__ u4 min4(u4 a, u4 b) { return u4{min(a[0], b[0]), min(a[1], b[1]), min(a[2], b[2]), min(a[3], b[3])}; }

// one doubling step on a lane's group: the values d positions in front of own's, from own and the group `front` in front (d = 1, 2)
template <bool SUM>
__device__ __forceinline__ u4 step_near(u4 own, u4 front, int d)
{
    const u4 sh = d == 1 ? u4{front[3], own[0], own[1], own[2]} : u4{front[2], front[3], own[0], own[1]};
    return SUM ? own + sh : min4(own, sh);
}

// the log2 W doubling steps of a sliding minimum (SUM false) or sum over W positions: own[j] holds the lane's groups, img the
// two LDS images, cur the one that holds own's values; the last step's values stay in own only
template <bool SUM>
__device__ __forceinline__ void slide(u4 (&own)[kGroups], unsigned (*img)[kSpan], int &cur, int W)
{
    for (int d = 1; d < W; d *= 2) {
        u4 next[kGroups];
#pragma unroll
        for (int j = 0; j < kGroups; j++) {
            const int i0 = 4 * (static_cast<int>(threadIdx.x) + j * kThreads);
            if (d < 4) {
                const u4 front = i0 >= 4 ? *reinterpret_cast<const u4 *>(&img[cur][i0 - 4]) : own[j];
                next[j] = step_near<SUM>(own[j], front, d);
            } else {
                const u4 sh = i0 >= d ? *reinterpret_cast<const u4 *>(&img[cur][i0 - d]) : own[j];   // (positions no window of the tile reaches)
                next[j] = SUM ? own[j] + sh : min4(own[j], sh);
            }
        }
        const bool last = 2 * d >= W;
#pragma unroll
        for (int j = 0; j < kGroups; j++) {
            own[j] = next[j];
            if (!last) *reinterpret_cast<u4 *>(&img[cur ^ 1][4 * (static_cast<int>(threadIdx.x) + j * kThreads)]) = next[j];
        }
        if (!last) {
            __syncthreads();
            cur ^= 1;
        }
    }
}

__device__ __forceinline__ unsigned pcm_pair(float lo, float hi, int wrap)
{
    return static_cast<unsigned>(static_cast<uint16_t>(pcm_pack(lo, wrap))) | (static_cast<unsigned>(static_cast<uint16_t>(pcm_pack(hi, wrap))) << 16);
}

template <int AC, bool VEC>
__global__ __launch_bounds__(kThreads) void leveller_apply_kernel(const float *__restrict__ in, float *__restrict__ out, int16_t *__restrict__ pcm,
                                                                  fmrx_leveller_status *st, const uint32_t *__restrict__ state_in,
                                                                  uint32_t *__restrict__ state_out, unsigned n_audio, float inv_n, float ceiling,
                                                                  int W, int lg, int wrap)
{
    static_assert(!VEC || AC == 2, "the 16-byte path is the stereo one");
    __shared__ __attribute__((aligned(16))) float su[AC][kSpan];
    __shared__ __attribute__((aligned(16))) unsigned sq[2][kSpan];
    const size_t c = blockIdx.x;
    const int tid = static_cast<int>(threadIdx.x);
    const long n = static_cast<long>(n_audio);
    const long k0 = static_cast<long>(blockIdx.y) * (kSpan - 2 * W);   // the tile's first sample
    const long base = k0 - 2 * W;                                      // the sample of position 0: a multiple of 4, as every group's first
    const size_t row = c * AC * n_audio;   // the channel's first float; its PCM starts at the same count of int16
    const int nc = 2 * W - 2, nu = W - 1;
    const size_t words = static_cast<size_t>(nu) * (2 + AC);
    const uint32_t *sin = state_in + c * words;
    uint32_t *sout = state_out + c * words;
    const float2 e = *reinterpret_cast<const float2 *>(&st[c].gain0);   // gain0, gain1: 8-byte aligned in a 48-byte row
    const float g0 = e.x, gs = (e.y - g0) * inv_n;

    u4 own[kGroups];
#pragma unroll
    for (int j = 0; j < kGroups; j++) {
        const int i0 = 4 * (tid + j * kThreads);
        const long p0 = base + i0;
        float u[AC][4];
        unsigned q[4];
        if (p0 < 0) {   // in front of the call (the first tile only): the carried state
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const long ci = p0 + i + nc, ui = p0 + i + nu;
                q[i] = ci >= 0 ? leveller::kOne - sin[ci] : leveller::kOne;
#pragma unroll
                for (int r = 0; r < AC; r++) u[r][i] = ui >= 0 ? __uint_as_float(sin[nc + r * nu + ui]) : 0.0f;
            }
        } else {
            float x[AC][4];
#pragma unroll
            for (int r = 0; r < AC; r++) {
                const float *p = in + row + static_cast<size_t>(r) * n_audio + p0;
                if (VEC) {
                    const f4 v = p0 < n ? *reinterpret_cast<const f4 *>(p) : f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int i = 0; i < 4; i++) x[r][i] = v[i];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) x[r][i] = p0 + i < n ? p[i] : 0.0f;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const float g = fmaf(static_cast<float>(static_cast<unsigned>(p0 + i) + 1u), gs, g0);
                q[i] = leveller::kOne;
#pragma unroll
                for (int r = 0; r < AC; r++) {
                    u[r][i] = p0 + i < n ? x[r][i] * g : 0.0f;   // behind the call's end: nothing, no window of the call reaches it
                    q[i] = min(q[i], leveller::code_of(fabsf(u[r][i]), ceiling));
                }
            }
        }
        // the next call's state: the call's last 2W - 2 codes and W - 1 values of u, each written by the lane that owns the
        // position (the tile's own positions; in the first tile also those in front of the call, which a short call carries on)
        if (p0 < 0 ? blockIdx.y == 0 : i0 >= 2 * W) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const long p = p0 + i, ci = p + nc - n, ui = p + nu - n;
                if (p < n && ci >= 0) sout[ci] = leveller::kOne - q[i];
                if (p < n && ui >= 0) {
#pragma unroll
                    for (int r = 0; r < AC; r++) sout[nc + r * nu + ui] = __float_as_uint(u[r][i]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < AC; r++) *reinterpret_cast<f4 *>(&su[r][i0]) = f4{u[r][0], u[r][1], u[r][2], u[r][3]};
        own[j] = u4{q[0], q[1], q[2], q[3]};
        *reinterpret_cast<u4 *>(&sq[0][i0]) = own[j];
    }
    __syncthreads();

    int cur = 0;
    slide<false>(own, sq, cur, W);   // m: valid from position W - 1
    // the minimum's last step left its values in registers only: the sum starts from an image of them
#pragma unroll
    for (int j = 0; j < kGroups; j++) *reinterpret_cast<u4 *>(&sq[cur ^ 1][4 * (tid + j * kThreads)]) = own[j];
    __syncthreads();
    cur ^= 1;
    slide<true>(own, sq, cur, W);    // the sum of W minima: valid from position 2W - 2

    unsigned mn = leveller::kOne, cnt = 0;
#pragma unroll
    for (int j = 0; j < kGroups; j++) {
        const int i0 = 4 * (tid + j * kThreads);
        const long p0 = base + i0;
        if (i0 < 2 * W || p0 >= n) continue;
        float y[AC][4];
        float sf[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned s = own[j][i] >> lg;
            sf[i] = static_cast<float>(s) * 0x1p-24f;
            if (p0 + i < n) {
                mn = min(mn, s);
                cnt += s < leveller::kOne ? 1u : 0u;
            }
        }
#pragma unroll
        for (int r = 0; r < AC; r++) {   // u delayed by W - 1: positions i0 - W + 1 .. i0 - W + 4
            const f4 a = *reinterpret_cast<const f4 *>(&su[r][i0 - W]), b = *reinterpret_cast<const f4 *>(&su[r][i0 - W + 4]);
            y[r][0] = a[1] * sf[0];
            y[r][1] = a[2] * sf[1];
            y[r][2] = a[3] * sf[2];
            y[r][3] = b[0] * sf[3];
        }
        if (out) {
#pragma unroll
            for (int r = 0; r < AC; r++) {
                float *p = out + row + static_cast<size_t>(r) * n_audio + p0;
                if (VEC) {
                    *reinterpret_cast<f4 *>(p) = f4{y[r][0], y[r][1], y[r][2], y[r][3]};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (p0 + i < n) p[i] = y[r][i];
                }
            }
        }
        if (pcm) {
            int16_t *w = pcm + row + static_cast<size_t>(AC) * p0;
            if (VEC) {
                *reinterpret_cast<u4 *>(w) = u4{pcm_pair(y[0][0], y[AC - 1][0], wrap), pcm_pair(y[0][1], y[AC - 1][1], wrap),
                                               pcm_pair(y[0][2], y[AC - 1][2], wrap), pcm_pair(y[0][3], y[AC - 1][3], wrap)};
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (p0 + i < n) {
#pragma unroll
                        for (int r = 0; r < AC; r++) w[AC * i + r] = pcm_pack(y[r][i], wrap);
                    }
            }
        }
    }
    if (__any(cnt != 0)) {   // (wave-uniform) a wave that limited anything: its minimum and count, one pair of atomics
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn = min(mn, static_cast<unsigned>(__shfl_xor(static_cast<int>(mn), off)));
            cnt += static_cast<unsigned>(__shfl_xor(static_cast<int>(cnt), off));
        }
        if ((tid & 63) == 0) {
            atomicMin(&st[c].min_code, mn);
            atomicAdd(&st[c].limited, cnt);
        }
    }
}

}  // namespace

int leveller_control_launch(const leveller::Control &c, int audio_channels, const double *d_k2a, const double *d_k2b,
                            const unsigned long long *d_n_each, unsigned long long n_all, fmrx_leveller_status *d_status, int n_channels,
                            hipStream_t s)
{
    return meter_stage::control_launch("leveller_control_kernel", leveller_control_kernel, n_channels, s, c, audio_channels, d_k2a, d_k2b, d_n_each, n_all,
                                       d_status);
}

int leveller_apply_launch(const LevellerArgs &a, hipStream_t s)
{
    if (!leveller::good_lookahead(a.W)) return fail(FMRX_EINVAL, "leveller: lookahead %d", a.W);
    const size_t tile = static_cast<size_t>(kSpan - 2 * a.W), tiles = (a.n + tile - 1) / tile;
    if (a.n < 1 || tiles > 65535) return fail(FMRX_EINVAL, "leveller: %zu samples per row: 1 .. %zu", a.n, 65535 * tile);
    const auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = a.ac == 2 && a.n % 4 == 0 && al16(a.x) && al16(a.y) && al16(a.pcm);   // a NULL pointer is aligned
    const dim3 grid(static_cast<unsigned>(a.n_channels), static_cast<unsigned>(tiles));
    const unsigned n = static_cast<unsigned>(a.n);
    const int lg = leveller::log2_of(a.W);
    if (a.ac == 1)
        leveller_apply_kernel<1, false><<<grid, kThreads, 0, s>>>(a.x, a.y, a.pcm, a.status, a.state_in, a.state_out, n, a.inv_n, a.ceiling, a.W, lg, a.wrap);
    else if (vec)
        leveller_apply_kernel<2, true><<<grid, kThreads, 0, s>>>(a.x, a.y, a.pcm, a.status, a.state_in, a.state_out, n, a.inv_n, a.ceiling, a.W, lg, a.wrap);
    else
        leveller_apply_kernel<2, false><<<grid, kThreads, 0, s>>>(a.x, a.y, a.pcm, a.status, a.state_in, a.state_out, n, a.inv_n, a.ceiling, a.W, lg, a.wrap);
    FMRX_LAUNCH_CHECK("leveller_apply_kernel<%d,%d>", a.ac, static_cast<int>(vec));
    return FMRX_OK;
}

}  // namespace fmrx
