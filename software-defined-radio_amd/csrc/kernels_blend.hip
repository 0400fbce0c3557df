// kernels_blend.hip -- the two kernels of the stereo blend / soft mute stage (include/fmrx.h: fmrx_blend_*; DESIGN.md section
// 4.12; defined by tests/_blend_model.py).
//
// blend_control_kernel: meter_stage.hpp's control kernel with control_step of blend_control.hpp.  The status row is state and
// result at once -- lamp, drives, targets, smoothed values, the float32 end points (mono0, gain0, mono1, gain1) of this
// call's ramps, the call count.
//
// blend_apply_kernel: the pass over the audio, 8 bytes in, 8 bytes out and 4 bytes of PCM per stereo sample, nothing else.
// The channel rides in the grid's x (banks have more than 65 535 receivers), a piece of the row in its y.  A lane owns groups
// of 4 consecutive samples of both rows: its piece's group t and, where the row is that long, group t + 256; both groups are
// loaded before either is used.  Rows that are 16-byte aligned (stereo, every pointer given, n_audio a multiple of 4 -- one
// decision for the whole launch, taken on the host): per group two 16-byte loads, two 16-byte stores and one 16-byte store
// of the 4 interleaved L,R PCM pairs.  All others (mono rows of any length, an unaligned base, a length that is no multiple
// of 4): the same samples in the same arithmetic with 4-byte loads and stores (2-byte for PCM), the row's last group cut at
// n_audio.  A lane reads its samples before it writes them and no lane touches another's, so d_out may be d_in.
// The channel's four end points come as one 16-byte load from its status row; a[k] and m[k] are one fused multiply-add and
// a clamp each, per sample.
#include "blend_control.hpp"
#include "device_math.hpp"
#include "meter_stage.hpp"

namespace fmrx {
namespace {

using f4 = float __attribute__((ext_vector_type(4)));
using u4 = unsigned __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kGroups = 2;   // groups of 4 samples per lane

__global__ __launch_bounds__(meter_stage::kControlThreads) void blend_control_kernel(blend::Control c, const double *__restrict__ mpx,
                                                                                     const unsigned long long *__restrict__ seg_each,
                                                                                     unsigned long long seg_all,
                                                                                     fmrx_blend_status *__restrict__ st, unsigned n_channels)
{
    meter_stage::control_body(c, mpx, seg_each, seg_all, st, n_channels);
}

// value k of a ramp from v0: clamp(fmaf(k + 1, step, v0), 0, 1)
__device__ __forceinline__ float ramp_at(unsigned k, float step, float v0)
{
    const float x = fmaf(static_cast<float>(k + 1u), step, v0);
    return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
}

__device__ __forceinline__ void blend_pair(float a, float m, float &L, float &R)
{
    const float D = 0.5f * (L - R);
    const float l = a == 0.0f ? L : fmaf(-a, D, L);
    const float r = a == 0.0f ? R : fmaf(a, D, R);
    L = m * l;
    R = m * r;
}

__device__ __forceinline__ unsigned pcm_pair(float lo, float hi, int wrap)
{
    return static_cast<unsigned>(static_cast<uint16_t>(pcm_pack(lo, wrap))) | (static_cast<unsigned>(static_cast<uint16_t>(pcm_pack(hi, wrap))) << 16);
}

template <int AC, bool VEC>
__global__ __launch_bounds__(kThreads) void blend_apply_kernel(const float *in, float *out, int16_t *pcm, const fmrx_blend_status *__restrict__ st,
                                                               unsigned n_audio, float inv_n, int wrap)
{
    static_assert(!VEC || AC == 2, "the 16-byte path is the stereo one");
    const size_t c = blockIdx.x;
    const f4 e = *reinterpret_cast<const f4 *>(&st[c].mono0);   // mono0, gain0, mono1, gain1: 16-byte aligned in an 80-byte row
    const float a0 = e[0], m0 = e[1];
    const float sa = (e[2] - a0) * inv_n, sm = (e[3] - m0) * inv_n;
    const unsigned groups = (n_audio + 3u) / 4u;
    const unsigned g0 = blockIdx.y * (kGroups * kThreads) + threadIdx.x;
    const size_t row = c * AC * n_audio;   // the channel's first float; its PCM starts at the same count of int16
    float x[kGroups][AC][4];
#pragma unroll
    for (int j = 0; j < kGroups; j++) {
        const unsigned g = g0 + j * kThreads;
        if (g >= groups) break;
        const unsigned k0 = 4u * g;
#pragma unroll
        for (int ch = 0; ch < AC; ch++) {
            const float *p = in + row + static_cast<size_t>(ch) * n_audio + k0;
            if (VEC) {
                const f4 v = *reinterpret_cast<const f4 *>(p);
#pragma unroll
                for (int i = 0; i < 4; i++) x[j][ch][i] = v[i];
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) x[j][ch][i] = k0 + i < n_audio ? p[i] : 0.0f;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kGroups; j++) {
        const unsigned g = g0 + j * kThreads;
        if (g >= groups) break;
        const unsigned k0 = 4u * g;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float m = ramp_at(k0 + i, sm, m0);
            if (AC == 2) blend_pair(ramp_at(k0 + i, sa, a0), m, x[j][0][i], x[j][1][i]);
            else x[j][0][i] = m * x[j][0][i];
        }
        if (out) {
#pragma unroll
            for (int ch = 0; ch < AC; ch++) {
                float *p = out + row + static_cast<size_t>(ch) * n_audio + k0;
                if (VEC) {
                    *reinterpret_cast<f4 *>(p) = f4{x[j][ch][0], x[j][ch][1], x[j][ch][2], x[j][ch][3]};
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (k0 + i < n_audio) p[i] = x[j][ch][i];
                }
            }
        }
        if (pcm) {
            int16_t *q = pcm + row + static_cast<size_t>(AC) * k0;
            if (VEC) {
                *reinterpret_cast<u4 *>(q) = u4{pcm_pair(x[j][0][0], x[j][1][0], wrap), pcm_pair(x[j][0][1], x[j][1][1], wrap),
                                               pcm_pair(x[j][0][2], x[j][1][2], wrap), pcm_pair(x[j][0][3], x[j][1][3], wrap)};
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (k0 + i < n_audio) {
#pragma unroll
                        for (int ch = 0; ch < AC; ch++) q[AC * i + ch] = pcm_pack(x[j][ch][i], wrap);
                    }
            }
        }
    }
}

}  // namespace

int blend_control_launch(const blend::Control &c, const double *d_mpx, const unsigned long long *d_seg_each, unsigned long long seg_all,
                         fmrx_blend_status *d_status, int n_channels, hipStream_t s)
{
    return meter_stage::control_launch("blend_control_kernel", blend_control_kernel, n_channels, s, c, d_mpx, d_seg_each, seg_all, d_status);
}

int blend_apply_launch(const float *d_in, float *d_out, int16_t *d_pcm, const fmrx_blend_status *d_status, int n_channels, int audio_channels,
                       size_t n_audio, float inv_n, int wrap, hipStream_t s)
{
    const size_t groups = (n_audio + 3) / 4, per_block = static_cast<size_t>(kGroups) * kThreads;
    const size_t pieces = (groups + per_block - 1) / per_block;
    if (pieces > 65535) return fail(FMRX_EINVAL, "blend: %zu samples per row: at most %zu", n_audio, 65535 * per_block * 4);
    const auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const bool vec = audio_channels == 2 && n_audio % 4 == 0 && al16(d_in) && al16(d_out) && al16(d_pcm);   // a NULL pointer is aligned
    const dim3 grid(static_cast<unsigned>(n_channels), static_cast<unsigned>(pieces));
    const unsigned n = static_cast<unsigned>(n_audio);
    if (audio_channels == 1) blend_apply_kernel<1, false><<<grid, kThreads, 0, s>>>(d_in, d_out, d_pcm, d_status, n, inv_n, wrap);
    else if (vec) blend_apply_kernel<2, true><<<grid, kThreads, 0, s>>>(d_in, d_out, d_pcm, d_status, n, inv_n, wrap);
    else blend_apply_kernel<2, false><<<grid, kThreads, 0, s>>>(d_in, d_out, d_pcm, d_status, n, inv_n, wrap);
    FMRX_LAUNCH_CHECK("blend_apply_kernel<%d,%d>", audio_channels, static_cast<int>(vec));
    return FMRX_OK;
}

}  // namespace fmrx
