// kernels_bank.hip -- the kernels of a receiver bank (bank.hip: every stereo bank, the bit-exact mono banks and the fast mono banks of
// modes 2 and 3), the host-side builders of their tap tables, their launchers, and the resolver from a bank's shapes to those.
// Of the fast mono bank of modes 0/1 (the fused kind: one kernel of kernels_fe_mfma.hip for the whole chain) only the finish is here.
//
// The reference runs one receiver per process (one PARAMS / STATES set, src/project.cpp:455-468); its stereo
// thread body RF_STEREO (src/project.cpp:154-309) is, per block of fm_demod:
//     allPass -> convolveBlockFastFIR (mono) | convolveBlockFIR (pilot 18.5-19.5 kHz) -> fmPLL |
//     convolveBlockFIR (22-54 kHz) -> mixer -> convolveBlockFastFIR (stereo) -> L = st + mono, R = mono - st.
// fmPLL (src/filter.cpp:32-80) is a serial float32 recurrence through sinf / cosf / atan2f: inside ONE channel
// it cannot be cut in time without leaving the reference's trajectory (the recurrence is
// chaotic on the float32 grid of its phase argument).  ACROSS channels it is embarrassingly parallel: every
// channel owns its STATES.  So the bank gives each channel ONE LANE that walks the exact recurrence, 64 channels
// per wave, and runs every other stage as wide kernels over (channel, sample):
//
//   chs_fe_exact_kernel      u8 I/Q -> (u-128)/128 -> rf FIR -> decimate -> discriminator   (src/project.cpp:82-128)
//   chs_bpf_exact_kernel     both band-pass filters of the stereo path in one pass           (:202, :207)
//   pll_channels_kernel      fmPLL, lane = channel (kernels_pll.hip)                          (:237)
//   chs_nco_exact_kernel     the NCO output's cosine, off the recurrence's chain              (src/filter.cpp:72)
//   chs_out_exact_kernel     mixer, both audio FIRs, L/R, PCM                                 (:246-302)
//   chs_finish_kernel        carried state: every row's tail -> its history
//
// "Exact" means the reference's float32 operations in the reference's order -- separately rounded products and
// sums, taps ascending (src/filter.cpp:133-188), glibc 2.35's sinf / cosf / atan2f (glibc_libm.hpp) -- so that
// left and right equal the compiled reference's bit for bit, per channel, for any stream length.  That order
// fixes the arithmetic (2 vector instructions per tap and output, nothing for the matrix cores to do), not the
// schedule: a thread owns R = 8 consecutive outputs and visits its window newest sample first, so that one
// converted sample feeds all the outputs it belongs to while every output still meets its taps in ascending
// order; the taps of a step are one aligned scalar load (s_load_dwordx16) from a step-major table.
//
// Data layout: everything is channel-major rows with the carried history in front:
//   slots   u8  [n_channels][hist_bytes | block_bytes]   raw I/Q as on stdin; the history IS I_state/Q_state/prev_i/prev_q
//   demod   f32 [n_channels][Hd | n_if | pad]            discriminator output; history = state_mono / _stereo / _carrier / _allpass
//   carrier, bpf, trig f32 [n_channels][n_if + pad]      pilot band-pass, 22-54 kHz band-pass, raw trigArg of every PLL step -> NCO output
//   pll     f32 [n_channels][8]                          state_PLL (6), fast banks: the PLL's fr (slot 6) ; nco0 [n_channels] = PLL[0] of this call
//   mixtail f32 [2][n_channels][Hm]                      state_stereofilt, ping-pong
#include <type_traits>

#include "bank_kernels.hpp"
#include "device_math.hpp"
#include "glibc_libm.hpp"

#pragma clang fp contract(off)

namespace fmrx {

namespace {

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// taps of one or two steps: wave-uniform, straight into SGPRs (inline asm keeps the loads where they are written)
#define CHS_TAPS_ISSUE(hp, table, off) asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(hp) : "s"(table), "i"(off))
#define CHS_TAPS_WAIT(hp) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(hp))

// ---- front end, reference order ------------------------------------------------------------------------------
// Thread: outputs k0 .. k0+R-1 (I and Q in the two halves of v_pk_mul_f32 / v_pk_add_f32).  Window sample j
// (j = 0: stream sample k0*D - (T-1)) meets output r with tap n = r*D + (T-1) - j.  Step u visits j = W-1-u, i.e.
// the window newest sample first: for every output the taps then come in ascending n, as in the reference's loop
// (src/filter.cpp:166-177), and each sample is converted once.  Table entry [u][r] = h[n] / 128 (0 where n is
// out of range: those pairs are not executed, the entry only keeps the load shape); the bytes are flipped to
// int8 (u ^ 0x80 = u - 128), so h/128 * (u-128) is the reference's product h * ((u-128)/128) bit for bit (a power
// of two moves no rounding; create() checks that no tap is so small that h/128 would be subnormal).
template <int T, int D>
struct FeX {
    static constexpr int R = kR;
    static constexpr int LEAD = (8 - (T - 1) % 8) % 8;          // samples in front of the window so that it starts 16 B aligned
    static constexpr int W = D * (R - 1) + T;                   // samples one thread needs
    static constexpr int NB = (2 * (W + LEAD) + 15) / 16;       // 16-byte loads per thread
    static constexpr int NG = (W + 1) / 2;                      // scalar-load groups: two steps each
    static constexpr int TILE = 63 * R;                         // new outputs per wave (lane 0 recomputes the R in front)
    static constexpr int HIST = 2 * (T - 1 + LEAD) + 2 * D * R; // bytes of history in front of a block
    static_assert((2 * D * R) % 16 == 0, "thread windows must start 16-byte aligned");
};

template <int T, int D, int G>
__device__ __forceinline__ void fex_step(const uint32_t (&raw)[FeX<T, D>::NB * 4], const float *__restrict__ table,
                                         f2 (&acc)[kR], f16v &hA, f16v &hB)
{
    using C = FeX<T, D>;
    if constexpr (G < C::NG) {
        float hq[16];
        if constexpr (G % 2 == 0) {
            CHS_TAPS_WAIT(hA);
            if constexpr (G + 1 < C::NG) CHS_TAPS_ISSUE(hB, table, (G + 1) * 64);
#pragma unroll
            for (int k = 0; k < 16; k++) hq[k] = hA[k];
        } else {
            CHS_TAPS_WAIT(hB);
            if constexpr (G + 1 < C::NG) CHS_TAPS_ISSUE(hA, table, (G + 1) * 64);
#pragma unroll
            for (int k = 0; k < 16; k++) hq[k] = hB[k];
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int u = 2 * G + e;
            if (u < C::W) {
                const int j = C::W - 1 - u;
                const int bo = 2 * (j + C::LEAD);
                const uint32_t w = raw[bo / 4];
                f2 xs;   // v_cvt_f32_i32_sdwa sext(w) src0_sel:BYTE_n
                if ((bo % 4) == 0) {
                    xs.x = static_cast<float>(static_cast<int8_t>(w & 0xffu));
                    xs.y = static_cast<float>(static_cast<int8_t>((w >> 8) & 0xffu));
                } else {
                    xs.x = static_cast<float>(static_cast<int8_t>((w >> 16) & 0xffu));
                    xs.y = static_cast<float>(static_cast<int8_t>(w >> 24));
                }
#pragma unroll
                for (int r = 0; r < kR; r++) {
                    const int n = r * D + (T - 1) - j;
                    if (n >= 0 && n < T) {
                        const float h = hq[8 * e + r];
                        const f2 prod = xs * (f2){h, h};      // separately rounded product ...
                        acc[r] = acc[r] + prod;               // ... and sum (src/filter.cpp:169, 174)
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kR; r++) asm volatile("" : "+v"(acc[r]));
        fex_step<T, D, G + 1>(raw, table, acc, hA, hB);
    }
}

// One wave per tile of 63*R outputs of one channel; lane 0 recomputes the R outputs in front of the tile (from the
// history in front of the block for the first tile) only to hand IF[k0-1] to lane 1: every IF sample is produced by
// the same instruction sequence wherever it is computed.
// Workgroups are single waves in all three wide kernels: a stereo call runs them next to the PLL's lanes (one long-lived wave
// per CU that keeps its SIMD's vector ALU nearly busy and, being the oldest wave there, wins every issue slot it wants); a
// workgroup of four waves would hold its slot until its wave on that SIMD is through (measured: 2.2 x the kernel time).
template <int T, int D>
__global__ __launch_bounds__(64) void chs_fe_exact_kernel(const uint8_t *__restrict__ slots, long slot_bytes, int hist_bytes,
                                                            long k_lo, long n_if, long ntiles, long wgs_per_channel,
                                                            const float *__restrict__ table, float *__restrict__ demod,
                                                            long dpitch, int Hd)
{
    using C = FeX<T, D>;
    constexpr int R = kR;
    const int lane = threadIdx.x & 63;
    const long c = blockIdx.x / wgs_per_channel;
    const long tile = blockIdx.x % wgs_per_channel;
    if (tile >= ntiles) return;                                  // wave-uniform
    const uint8_t *blk = slots + c * slot_bytes + hist_bytes;
    const long k0 = k_lo + tile * C::TILE + static_cast<long>(lane - 1) * R;   // outputs [k_lo, n_if) of the block: this launch's share
    const long w0 = k0 * D - (T - 1) - C::LEAD;                  // first sample of the 16-byte aligned window
    const u4 *src = reinterpret_cast<const u4 *>(blk + 2 * w0);
    uint32_t raw[C::NB * 4];
    // requested newest chunk first: that is the order the steps consume them in, so the arithmetic starts when the first load is back
#pragma unroll
    for (int i = C::NB - 1; i >= 0; i--) {
        const u4 v = src[i] ^ 0x80808080u;
        raw[4 * i] = v.x;
        raw[4 * i + 1] = v.y;
        raw[4 * i + 2] = v.z;
        raw[4 * i + 3] = v.w;
    }
    f2 acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = (f2){0.0f, 0.0f};
    f16v hA, hB;
    CHS_TAPS_ISSUE(hA, table, 0);
    fex_step<T, D, 0>(raw, table, acc, hA, hB);
    // fmDemod (src/filter.cpp:248-266): IF[k-1] is the previous accumulator, across threads the lane next door
    const float pi = __shfl_up(acc[R - 1].x, 1, 64), pq = __shfl_up(acc[R - 1].y, 1, 64);
    float d[R];
    d[0] = demod_exact(acc[0].x, acc[0].y, pi, pq);
#pragma unroll
    for (int r = 1; r < R; r++) d[r] = demod_exact(acc[r].x, acc[r].y, acc[r - 1].x, acc[r - 1].y);
    if (lane == 0 || k0 >= n_if) return;
    float *out = demod + c * dpitch + Hd + k0;
    if (k0 + R <= n_if) {
        reinterpret_cast<f4 *>(out)[0] = (f4){d[0], d[1], d[2], d[3]};
        reinterpret_cast<f4 *>(out)[1] = (f4){d[4], d[5], d[6], d[7]};
    } else {
#pragma unroll
        for (int r = 0; r < R; r++)
            if (k0 + r < n_if) out[r] = d[r];
    }
}

// ---- both band-pass filters, reference order -------------------------------------------------------------------
// convolveBlockFIR twice on the same input (src/project.cpp:202, 207 -> src/filter.cpp:133-154): the two filters
// ride in the two halves of the packed instructions, acc(st, car) = acc + x * (h_st[n], h_car[n]).  Same scheme as the
// front end with D = 1: window sample i (i = 0: x[k0 - (T-1)]) meets output r with tap n = r + (T-1) - i; step u
// visits i = W-1-u; table entry [u][r] = (h_st[n], h_car[n]).
template <int T>
struct BpX {
    static constexpr int R = kR;
    static constexpr int LEAD = (4 - (T - 1) % 4) % 4;
    static constexpr int W = R + T - 1;
    static constexpr int NW = W + LEAD;                         // floats loaded
    static_assert(NW % 4 == 0, "window must be whole 16-byte chunks");
};

// The taps of consecutive steps overlap: step u needs the pairs P[u .. u+7] of the padded table P[m] = (h_st, h_car)[m - (R-1)]
// (zero outside the filter), i.e. one NEW pair per step.  They are fetched in groups of eight (one s_load_dwordx16 per EIGHT
// steps) into three rotating SGPR groups: at the start of block g the groups g and g+1 are resident and g+2 is requested --
// scalar loads return out of order, so every wait is for all of them, and a load requested eight steps (~500 cycles) ahead
// has long arrived (one load per step, waited for a step later, left the vector ALU idle half the time).
template <int T, bool EXACT, int G>
__device__ __forceinline__ void bpx_block(const float (&w)[BpX<T>::NW], const float *__restrict__ table, f2 (&acc)[kR], f16v &g0,
                                          f16v &g1, f16v &g2)
{
    using C = BpX<T>;
    constexpr int NBLK = (C::W + 7) / 8;
    if constexpr (G < NBLK) {
        // groups G (cur), G + 1 (next) resident after this wait; G + 2 requested behind it into the group G - 1 used
        f16v &cur = G % 3 == 0 ? g0 : (G % 3 == 1 ? g1 : g2);
        f16v &nxt = (G + 1) % 3 == 0 ? g0 : ((G + 1) % 3 == 1 ? g1 : g2);
        f16v &fut = (G + 2) % 3 == 0 ? g0 : ((G + 2) % 3 == 1 ? g1 : g2);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(cur), "+s"(nxt));
        if constexpr (G + 2 <= NBLK) CHS_TAPS_ISSUE(fut, table, (G + 2) * 64);
        float hc[16], hn[16];
#pragma unroll
        for (int k = 0; k < 16; k++) {
            hc[k] = cur[k];
            hn[k] = nxt[k];
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int u = 8 * G + e;
            if (u < C::W) {
                const int i = C::W - 1 - u;
                const float x = w[i + C::LEAD];
#pragma unroll
                for (int r = 0; r < kR; r++) {
                    const int n = r + (T - 1) - i;
                    if (n >= 0 && n < T) {
                        const int m = e + r;                       // pair P[8 G + m]: this group for m < 8, the next one after
                        const float hs = m < 8 ? hc[2 * m] : hn[2 * (m - 8)], hcar = m < 8 ? hc[2 * m + 1] : hn[2 * (m - 8) + 1];
                        if constexpr (EXACT) {
                            const f2 prod = (f2){x, x} * (f2){hs, hcar};
                            acc[r] = acc[r] + prod;
                        } else {   // the fast bank: one fused multiply-add per tap (float32-rounding-equal, as the single-stream kernels)
                            acc[r] = __builtin_elementwise_fma((f2){x, x}, (f2){hs, hcar}, acc[r]);
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < kR; r++) asm volatile("" : "+v"(acc[r]));
        }
        bpx_block<T, EXACT, G + 1>(w, table, acc, g0, g1, g2);
    }
}

template <int T, bool EXACT>
__global__ __launch_bounds__(64) void chs_bpf_kernel(const float *__restrict__ demod, long dpitch, int Hd, long k_lo, long n_if,
                                                             long wgs_per_channel, const float *__restrict__ table,
                                                             float *__restrict__ y_st, float *__restrict__ y_car, long ypitch,
                                                             int8_t *__restrict__ y_car8, long cpitch)
{
    using C = BpX<T>;
    constexpr int R = kR;
    const long c = blockIdx.x / wgs_per_channel;
    const long k0 = k_lo + ((blockIdx.x % wgs_per_channel) * 64 + threadIdx.x) * R;
    if (k0 >= n_if) return;
    const float *x = demod + c * dpitch + Hd;
    const f4 *src = reinterpret_cast<const f4 *>(x + k0 - (T - 1) - C::LEAD);
    float w[C::NW];
#pragma unroll
    for (int i = C::NW / 4 - 1; i >= 0; i--) {                  // newest chunk first: the order the steps consume them in
        const f4 v = src[i];
        w[4 * i] = v.x;
        w[4 * i + 1] = v.y;
        w[4 * i + 2] = v.z;
        w[4 * i + 3] = v.w;
    }
    f2 acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = (f2){0.0f, 0.0f};
    f16v g0, g1, g2;
    CHS_TAPS_ISSUE(g0, table, 0);
    CHS_TAPS_ISSUE(g1, table, 64);
    bpx_block<T, EXACT, 0>(w, table, acc, g0, g1, g2);
    float *ds = y_st + c * ypitch + k0;
    if constexpr (!EXACT) {
        // fast bank: the pilot band-pass output only feeds the PLL's fast recurrence, which reads its SIGN: one signed byte per sample
        // (+1 / -1; 0 = not an ordinary sample: zero, denormal-small or not finite -- kernels_pll.hip: pll_ordinary)
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float v = acc[r].y;
            const bool ord = fabsf(v) > 1e-20f && fabsf(v) < 1e20f;
            const uint32_t code = ord ? (v > 0.0f ? 0x01u : 0xffu) : 0u;
            if (r < 4) lo |= code << (8 * r);
            else hi |= code << (8 * (r - 4));
        }
        int8_t *dc8 = y_car8 + c * cpitch + k0;
        if (k0 + R <= n_if) {
            reinterpret_cast<f4 *>(ds)[0] = (f4){acc[0].x, acc[1].x, acc[2].x, acc[3].x};
            reinterpret_cast<f4 *>(ds)[1] = (f4){acc[4].x, acc[5].x, acc[6].x, acc[7].x};
            *reinterpret_cast<uint2 *>(dc8) = make_uint2(lo, hi);
        } else {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (k0 + r < n_if) {
                    ds[r] = acc[r].x;
                    dc8[r] = static_cast<int8_t>(((r < 4 ? lo : hi) >> (8 * (r % 4))) & 0xff);
                }
        }
    } else {
        float *dc = y_car + c * ypitch + k0;
        if (k0 + R <= n_if) {
            reinterpret_cast<f4 *>(ds)[0] = (f4){acc[0].x, acc[1].x, acc[2].x, acc[3].x};
            reinterpret_cast<f4 *>(ds)[1] = (f4){acc[4].x, acc[5].x, acc[6].x, acc[7].x};
            reinterpret_cast<f4 *>(dc)[0] = (f4){acc[0].y, acc[1].y, acc[2].y, acc[3].y};
            reinterpret_cast<f4 *>(dc)[1] = (f4){acc[4].y, acc[5].y, acc[6].y, acc[7].y};
        } else {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (k0 + r < n_if) {
                    ds[r] = acc[r].x;
                    dc[r] = acc[r].y;
                }
        }
    }
}

// ---- the NCO output ----------------------------------------------------------------------------------------------------
// PLL[k+1] = cosf(trigArg[k]*ncoScale + phaseAdjust) (src/filter.cpp:72) is not on the recurrence's chain: the lanes leave the
// raw trigArg of every step, this kernel turns a chunk's row segment into finished NCO values in place, four per thread
// (glibc's cosf: the branch-free form when the whole wave's arguments are ordinary, i.e. always but in a stream's first 120 samples).
template <bool EXACT>
__global__ __launch_bounds__(256) void chs_nco_kernel(float *__restrict__ trig, long ypitch, long k_lo, long k_hi, long wgs_per_channel,
                                                             float nco_scale, float phase_adjust, const float *__restrict__ bpf,
                                                             const float *__restrict__ nco0, float *__restrict__ mixer, long mpitch, int hm)
{
    __shared__ uint32_t w24[24];
    if (threadIdx.x < 24) w24[threadIdx.x] = glibc235::inv_pio4(threadIdx.x);
    __syncthreads();
    const long c = blockIdx.x / wgs_per_channel;
    const long k = k_lo + ((blockIdx.x % wgs_per_channel) * 256 + threadIdx.x) * 4;
    if (k >= k_hi) return;
    f4 *p = reinterpret_cast<f4 *>(trig + c * ypitch + k);
    const f4 v = *p;
    float a[4], o[4];
#pragma unroll
    for (int i = 0; i < 4; i++) a[i] = v[i] * nco_scale + phase_adjust;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 4; i++) ok = ok && glibc235::sincosf_large_ok(a[i]);
    if (!EXACT) {   // the fast bank: one argument reduction in double, the hardware cosine (kernels_pll.hip: nco_out<kFast>)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const double rev = static_cast<double>(a[i]) * 0.15915494309189533577;
            o[i] = __builtin_amdgcn_cosf(static_cast<float>(rev - rint(rev)));
        }
    } else if (!__any(!ok)) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            float sn;
            glibc235::sincosf_large_flat(a[i], w24, &sn, &o[i]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = glibc235::cosf_glibc(a[i]);
    }
    if (k + 4 <= k_hi) {
        *p = (f4){o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (k + i < k_hi) trig[c * ypitch + k + i] = o[i];
    }
    // The resampling modes read the mixer output (src/project.cpp:246-248: (stereo_filt * PLL) * 2, PLL[g] = the NCO value of step
    // g - 1, PLL[0] = the incoming state's lastOut) as a row of its own (chs_resample_*): written here, rows [hm | n_if], history
    // carried by the finish kernel.  Entry k_lo takes the NCO value the previous chunk's launch left in trig[k_lo - 1].
    if (mixer) {
        const float *bp = bpf + c * ypitch;
        float *mx = mixer + c * mpitch + hm;
        if (k == k_lo) mx[k] = (bp[k] * (k > 0 ? trig[c * ypitch + k - 1] : nco0[c])) * 2.0f;
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (k + 1 + i < k_hi) mx[k + 1 + i] = (bp[k + 1 + i] * o[i]) * 2.0f;
    }
}

// ---- everything behind the PLL ------------------------------------------------------------------------------------
// The mixer (src/project.cpp:246-248), the two audio convolveBlockFastFIR calls of RF_STEREO -- mono branch on the
// all-passed discriminator output (:194, :219), stereo branch on the mixer output (:257) --, the L/R combine (:277-280)
// and the interleaved PCM writer (:292-302), in the reference's evaluation order.  A single-wave workgroup stages the
// window of its 64*R audio outputs as (mono, mixer) pairs in LDS -- the mixer products are formed while staging and never
// go to HBM; the two FIRs share the taps, so they ride in the two halves of the packed instructions.  The FIR is the
// front end's scheme once more: a thread owns R = kRO ADJACENT outputs and visits its window newest sample first, one
// ds_read_b64 per sample feeds every output the sample belongs to (R = 4: 116 LDS reads per 404 tap-output pairs; the
// one-read-per-tap form is bound by LDS bandwidth at twice the time), the taps of two steps are one scalar load.
// Neighbouring lanes' windows start R*D pairs apart; the LDS index j + j / (R*D) makes that an odd number of
// pairs (R = 4: 21 / 25): conflict-free ds_read_b64.  Mono banks (STEREO = false) run the same kernel on the mono half alone.
constexpr int kRO = 4;   // adjacent audio outputs per thread of the output stage (8: 512 outputs and 22 KB of LDS per workgroup -- 7 single-wave
                         // workgroups per CU, whose staging latency then sets the kernel's time; 4: 256 outputs, 11 KB, 14 per CU)
template <int T, int D>
struct OutX {
    static constexpr int R = kRO;
    static constexpr int SPL = 16 / R;                          // steps per scalar load of 16 taps
    static constexpr int W = D * (R - 1) + T;                   // window samples (= steps) per thread
    static constexpr int NG = (W + SPL - 1) / SPL;              // scalar-load groups
    static constexpr int NOUT = 64 * R;                         // audio outputs per workgroup
    static constexpr int WL = D * (NOUT - 1) + T;               // window samples per workgroup
    static constexpr int SEG = R * D;                           // window samples between neighbouring lanes
    static constexpr int LDSN = WL + WL / SEG + 2;              // pairs in LDS
    __host__ __device__ static constexpr int idx(int j) { return j + j / SEG; }
};

template <int T, int D, bool STEREO, bool EXACT, int G>
__device__ __forceinline__ void outx_step(const f2 *__restrict__ wl, const float *__restrict__ table, f2 (&acc)[kRO], f16v &hA, f16v &hB)
{
    using C = OutX<T, D>;
    if constexpr (G < C::NG) {
        float hq[16];
        if constexpr (G % 2 == 0) {
            CHS_TAPS_WAIT(hA);
            if constexpr (G + 1 < C::NG) CHS_TAPS_ISSUE(hB, table, (G + 1) * 64);
#pragma unroll
            for (int k = 0; k < 16; k++) hq[k] = hA[k];
        } else {
            CHS_TAPS_WAIT(hB);
            if constexpr (G + 1 < C::NG) CHS_TAPS_ISSUE(hA, table, (G + 1) * 64);
#pragma unroll
            for (int k = 0; k < 16; k++) hq[k] = hB[k];
        }
#pragma unroll
        for (int e = 0; e < C::SPL; e++) {
            const int u = C::SPL * G + e;
            if (u < C::W) {
                const int jj = C::W - 1 - u;                    // window sample of this thread, newest first
                const f2 w = wl[C::idx(jj)];                    // lane base + compile-time offset
#pragma unroll
                for (int r = 0; r < kRO; r++) {
                    const int n = r * D + (T - 1) - jj;
                    if (n >= 0 && n < T) {
                        const float h = hq[kRO * e + r];
                        if constexpr (!EXACT) {
                            acc[r] = __builtin_elementwise_fma(w, (f2){h, h}, acc[r]);
                        } else if constexpr (STEREO) {
                            const f2 prod = w * (f2){h, h};
                            acc[r] = acc[r] + prod;
                        } else {
                            const float prod = w.x * h;
                            acc[r].x = acc[r].x + prod;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kRO; r++) asm volatile("" : "+v"(acc[r]));
        outx_step<T, D, STEREO, EXACT, G + 1>(wl, table, acc, hA, hB);
    }
}

template <int T, int D, bool STEREO, bool EXACT>
__global__ __launch_bounds__(64) void chs_out_kernel(const float *__restrict__ demod, long dpitch, int Hd, const float *__restrict__ bpf,
                                                            const float *__restrict__ nco, long ypitch, const float *__restrict__ nco0,
                                                            const float *__restrict__ mix_tail_in, float *__restrict__ mix_tail_out, int hm,
                                                            long n_if, long g_hi, int delay, float nco_scale, float phase_adjust,
                                                            const float *__restrict__ table, long wgs_per_channel, float *__restrict__ audio,
                                                            int16_t *__restrict__ pcm, int wrap, long a_lo, long a_hi, long n_out)
{
    using C = OutX<T, D>;
    constexpr int R = kRO;
    __shared__ f2 win[C::LDSN];
    const int t = threadIdx.x;
    const long c = blockIdx.x / wgs_per_channel;
    // this launch: audio outputs [a_lo, a_hi) of the block's n_out, from the IF samples [.., g_hi) that exist by now (a block is
    // walked in chunks so that the PLL's lanes of one chunk run next to the wide kernels of the next: bank.hip, process_stereo)
    const long a0 = a_lo + (blockIdx.x % wgs_per_channel) * C::NOUT;
    const long g0 = D * a0 - (T - 1);                      // IF index of window sample 0
    const float *dm = demod + c * dpitch + Hd;
    const float *bp = STEREO ? bpf + c * ypitch : nullptr, *nc = STEREO ? nco + c * ypitch : nullptr;
    const float *tin = STEREO ? mix_tail_in + c * hm : nullptr;
    float *tout = STEREO ? mix_tail_out + c * hm : nullptr;
    const float first = STEREO ? nco0[c] : 0.0f;
    // D-1 samples past the window are visited too: when the block ends exactly on a tile boundary nobody's window reaches
    // the block's last D-1 samples, and they belong to the tail this call leaves behind
    // Staging in batches of B samples per lane, the next batch's three loads per sample in flight while this one is turned into
    // LDS pairs.  EXACT: `nco` holds finished NCO values (chs_nco_kernel); fast bank: the raw trigArg of the PLL's steps, and the
    // cosine is taken here (one argument reduction in double + the hardware cosine, kernels_pll.hip: nco_out<kFast>).
    constexpr int NJ = (C::WL + D - 1 + 63) / 64, B = kRO == 4 ? 11 : 11, NBATCH = (NJ + B - 1) / B;
    float vm[2][B], va[2][B], vb[2][B];
    auto fetch = [&](int q0, float (&m)[B], float (&a)[B], float (&b)[B]) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < B; q++) {
            const int j = t + (q0 + q) * 64;
            const long g = g0 + j;
            m[q] = 0.0f;
            a[q] = 0.0f;
            b[q] = 0.0f;
            if (j < C::WL + D - 1 && g < g_hi) {
                m[q] = dm[g - delay];                          // history in front of the row: negative indices are valid
                if (STEREO) {
                    a[q] = g >= 0 ? bp[g] : tin[hm + g];
                    if (g > 0) b[q] = nc[g - 1];               // PLL[g] = cos(trigArg[g-1] * ncoScale + phaseAdjust)
                }
            }
        }
    };
    fetch(0, vm[0], va[0], vb[0]);
#pragma unroll
    for (int bi = 0; bi < NBATCH; bi++) {
        if (bi + 1 < NBATCH) fetch((bi + 1) * B, vm[(bi + 1) & 1], va[(bi + 1) & 1], vb[(bi + 1) & 1]);
#pragma unroll
        for (int q = 0; q < B; q++) {
            const int j = t + (bi * B + q) * 64;
            const long g = g0 + j;
            if (j >= C::WL + D - 1) continue;
            float m = 0.0f, x = 0.0f;
            if (g < g_hi) {
                m = vm[bi & 1][q];
                if (STEREO) {
                    if (g >= 0) {
                        float pll = vb[bi & 1][q];
                        if (!EXACT) {
                            const double rev = static_cast<double>(pll * nco_scale + phase_adjust) * 0.15915494309189533577;
                            pll = __builtin_amdgcn_cosf(static_cast<float>(rev - rint(rev)));
                        }
                        if (g == 0) pll = first;               // PLL[0] = the incoming state's lastOut
                        x = (va[bi & 1][q] * pll) * 2.0f;      // the reference's order: (stereo_filt * PLL) * 2
                        if (g >= n_if - hm) tout[g - (n_if - hm)] = x;
                    } else {
                        x = va[bi & 1][q];
                    }
                }
            }
            if (j < C::WL) win[C::idx(j)] = (f2){m, x};
        }
    }
    __syncthreads();
    f2 acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = (f2){0.0f, 0.0f};
    f16v hA, hB;
    CHS_TAPS_ISSUE(hA, table, 0);
    outx_step<T, D, STEREO, EXACT, 0>(win + (C::SEG + 1) * t, table, acc, hA, hB);
    const long k0 = a0 + static_cast<long>(t) * R;
    if (k0 >= a_hi) return;
    if constexpr (STEREO) {
        float l[R], rr[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            l[r] = acc[r].y + acc[r].x;                        // src/project.cpp:278-279: left = stereo + mono, right = mono - stereo
            rr[r] = acc[r].x - acc[r].y;
        }
        if (k0 + R <= a_hi) {
            if (audio) {
                f4 *pl = reinterpret_cast<f4 *>(audio + c * 2 * n_out + k0), *pr = reinterpret_cast<f4 *>(audio + c * 2 * n_out + n_out + k0);
#pragma unroll
                for (int q = 0; q < R / 4; q++) {
                    pl[q] = (f4){l[4 * q], l[4 * q + 1], l[4 * q + 2], l[4 * q + 3]};
                    pr[q] = (f4){rr[4 * q], rr[4 * q + 1], rr[4 * q + 2], rr[4 * q + 3]};
                }
            }
            if (pcm) {
                using s8v = short __attribute__((ext_vector_type(8)));
                s8v *pp = reinterpret_cast<s8v *>(pcm + 2 * (c * n_out + k0));
#pragma unroll
                for (int q = 0; q < R / 4; q++)
                    pp[q] = (s8v){pcm_pack_flat(l[4 * q], wrap), pcm_pack_flat(rr[4 * q], wrap), pcm_pack_flat(l[4 * q + 1], wrap),
                                  pcm_pack_flat(rr[4 * q + 1], wrap), pcm_pack_flat(l[4 * q + 2], wrap), pcm_pack_flat(rr[4 * q + 2], wrap),
                                  pcm_pack_flat(l[4 * q + 3], wrap), pcm_pack_flat(rr[4 * q + 3], wrap)};
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (k0 + r < a_hi) {
                    if (audio) {
                        audio[c * 2 * n_out + k0 + r] = l[r];
                        audio[c * 2 * n_out + n_out + k0 + r] = rr[r];
                    }
                    if (pcm) {
                        pcm[2 * (c * n_out + k0 + r)] = pcm_pack_flat(l[r], wrap);
                        pcm[2 * (c * n_out + k0 + r) + 1] = pcm_pack_flat(rr[r], wrap);
                    }
                }
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; r++)
            if (k0 + r < a_hi) {
                if (audio) audio[c * n_out + k0 + r] = acc[r].x;
                if (pcm) pcm[c * n_out + k0 + r] = pcm_pack_flat(acc[r].x, wrap);
            }
    }
}

// ---- the resampling modes (2, 3) behind the PLL, reference order ----------------------------------------------------------
// RF_STEREO with audio_upsamp > 0 (src/project.cpp:224-231, 262-269): convolveBlockResampleFIR (src/filter.cpp:191-223) on the
// all-passed discriminator output and on the mixer output.  In stream form: output k reads phase ph = (k D) mod U of the taps and
// the input samples n_k, n_k - 1, ... with n_k = (k D - ph) / U:  y = sum_j h[ph + j U] x[n_k - j]  (separately rounded products
// and sums, j ascending), then y += y * U.  A block's outputs restart at phase 0 (the bank accepts blocks with n_if U % D == 0, as
// the reference's own block sizes are).  The mixer output is materialised by the chunk's NCO pass (chs_nco_kernel; rows [Hm | n_if],
// history carried by the finish kernel): the same row serves every output's window.  chs_resample_exact_kernel: one thread per (channel, output) -- any ratio,
// and the outputs chs_resample_lanes_kernel (below: the reference's two ratios at 5-7 x its speed) leaves over.
template <bool STEREO>
__global__ void chs_resample_exact_kernel(const float *__restrict__ demod, long dpitch, int Hd, const float *__restrict__ mixer, long mpitch,
                                          int hm, int delay, const float *__restrict__ h, int taps, int decim, int upsamp,
                                          long wgs_per_channel, float *__restrict__ audio, int16_t *__restrict__ pcm, int wrap, long a_lo,
                                          long a_hi, long n_out)
{
    const long c = blockIdx.x / wgs_per_channel;
    const long k = a_lo + (blockIdx.x % wgs_per_channel) * 256 + threadIdx.x;
    if (k >= a_hi) return;
    const long long m = static_cast<long long>(k) * decim;
    const int ph = static_cast<int>(m % upsamp);
    const long n0 = static_cast<long>((m - ph) / upsamp);
    const float *xm = demod + c * dpitch + Hd + n0 - delay;                    // the all-pass is an index offset
    const float *xs = STEREO ? mixer + c * mpitch + hm + n0 : nullptr;
    float am = 0.0f, as = 0.0f;
    int j = 0;
    for (int n = ph; n < taps; n += upsamp, j++) {
        const float hn = h[n];
        const float pm = hn * xm[-j];
        am = am + pm;
        if (STEREO) {
            const float ps = hn * xs[-j];
            as = as + ps;
        }
    }
    const float gm = am * static_cast<float>(upsamp);                          // y += y * U  (src/filter.cpp:213)
    const float mono = am + gm;
    if (STEREO) {
        const float gs = as * static_cast<float>(upsamp);
        const float st = as + gs;
        const float l = st + mono, r = mono - st;                              // src/project.cpp:278-279
        if (audio) {
            audio[c * 2 * n_out + k] = l;
            audio[c * 2 * n_out + n_out + k] = r;
        }
        if (pcm) {
            pcm[2 * (c * n_out + k)] = pcm_pack_flat(l, wrap);
            pcm[2 * (c * n_out + k) + 1] = pcm_pack_flat(r, wrap);
        }
    } else {
        if (audio) audio[c * n_out + k] = mono;
        if (pcm) pcm[c * n_out + k] = pcm_pack_flat(mono, wrap);
    }
}

// The same resampler with the bank turned the other way: a lane is a CHANNEL.  Output k's phase and window position depend on k
// alone, so for 64 channels at once the taps are wave-uniform -- SGPR operands from a step-major table, as in the exact FIRs
// above -- and only the samples are per lane.  A wave owns kRS = 7 consecutive outputs of 64 channels at a time (both modes' U are
// multiples of 7: groups never straddle a period, the table has U / 7 groups) and visits their common window newest sample first:
// output r meets its taps j ascending (the reference's order, src/filter.cpp:205-212; the fast bank fuses each product and sum
// into one fma, the exact bank rounds them separately) while one sample per lane and step feeds all seven outputs; (mono, stereo) -- in mono banks two neighbouring outputs -- ride in the two halves of the packed instructions.
// Samples reach the lanes through LDS, 32 per channel and batch (below: why not lane = channel for the loads too); the taps of
// four steps are two s_load_dwordx16, requested one iteration ahead.  Outside a group's window the table holds zeros: acc + 0*x
// leaves acc as it is (acc is never -0: it starts at +0 and sums round to nearest), rows are finite, and the rows' histories
// are long enough for the window's rounding up to whole batches (Bank::res_hist).  Against one thread per (channel,
// output) -- 101 gathered taps and 101-202 gathered samples per output, bound by the texture addressers -- 16 384 receivers x 4
// blocks of mode 2: stereo 12 -> 3.2 ms per call, mono 9 -> 1.7 ms (bit-identical outputs).  What bounds it now is the traffic of
// re-reading the windows: neighbouring groups' windows overlap (160 samples per 38 of advance), and 64 channels' windows of 2-3
// waves per SIMD do not fit L2.  The kRW = 3 (mono: 7) waves of a workgroup therefore take NEIGHBOURING groups at the same time
// (each with its own staging area, no barrier): their loads meet in L1 / L2 (mono fast, mode 2: 3.6 -> 3.4 ms per call with 3 waves, 3.0
// with 7; stereo banks stage twice as much per wave and 7 waves leave one workgroup per CU: no gain over 3).
constexpr int kRS = 7;
// waves per workgroup: they take neighbouring groups (overlapping windows) at the same time; mono banks stage half as much per wave
template <bool STEREO> constexpr int kRW = STEREO ? 3 : 7;

template <bool STEREO, bool EXACT>
__global__ __launch_bounds__(64 * kRW<STEREO>) void chs_resample_lanes_kernel(const float *__restrict__ demod, long dpitch, int Hd, const float *__restrict__ mixer,
                                                                 long mpitch, int hm, int delay, const float *__restrict__ table,
                                                                 const int *__restrict__ top_of, int groups_per_period, int groups_per_wave,
                                                                 int iters, int decim, int upsamp, long periods_per_row, int n_channels,
                                                                 float *__restrict__ audio, int16_t *__restrict__ pcm, int wrap, long a_lo,
                                                                 long n_out)
{
    // workgroup (one wave) = (64 channels, period a_lo / U + `period`, groups [g_lo, g_hi) of that period)
    // Grid order: channel group fastest, then period, the part of the period slowest -- the waves resident at any moment walk the
    // SAME groups, whose taps (5 KB per group) then stay in the scalar cache; the whole table (100-300 KB) does not fit there, and
    // with the part fastest every tap load went to L2 (517 -> 455 us per chunk)
    const long n_cg = (n_channels + 63) / 64;
    const long cg = blockIdx.x % n_cg;
    const long rest = blockIdx.x / n_cg;
    const long period = rest % periods_per_row;
    const int g_lo = static_cast<int>(rest / periods_per_row) * groups_per_wave;
    const int g_hi = g_lo + groups_per_wave < groups_per_period ? g_lo + groups_per_wave : groups_per_period;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const long c_raw = cg * 64 + lane;
    const long c = c_raw < n_channels ? c_raw : n_channels - 1;     // spare lanes repeat the last channel (nothing stored)
    const long k_base = a_lo + period * upsamp;                      // first output of this period (a multiple of U: phase 0)
    const long x_base = k_base / upsamp * decim;                     // its window position
    const float fu = static_cast<float>(upsamp);
    typedef float q4 __attribute__((ext_vector_type(4), aligned(4)));   // four consecutive samples of a row, any alignment
    // Samples reach the lanes through LDS, a batch of kSB = 32 per channel at a time.  Loading them lane = channel (each lane its own
    // row) makes every load instruction touch 64 cache lines for 1 KiB: the texture addressers, not the ALUs, then set the kernel's
    // time (804 -> 517 us per chunk).  Instead 8 lanes share a channel's 128 bytes (instruction i: channels 8 i + lane / 8, quad lane % 8):
    // 8-16 lines per instruction; the quads go to LDS as [sample][channel] rows of 66 floats (lanes of one write hit banks
    // channel + 8 quad + 2 j: all different), and a step reads its sample for the lane's OWN channel back: consecutive banks.
    constexpr int kSB = 32, kLP = 66;
    __shared__ float lds_all[kRW<STEREO> * (STEREO ? 2 : 1) * kSB * kLP];
    float *lds = lds_all + wv * ((STEREO ? 2 : 1) * kSB * kLP);   // a wave's own staging area: no barriers
    const int sub = lane >> 3, quad = lane & 7;
    long cl[8];                                                      // the channels this lane loads for (instruction i)
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const long cc = cg * 64 + 8 * i + sub;
        cl[i] = cc < n_channels ? cc : n_channels - 1;
    }
    const long m_off = Hd - delay + x_base, s_off = hm + x_base;     // the all-pass is an index offset
    for (int g = g_lo + wv; g < g_hi; g += kRW<STEREO>) {
        const int top = __builtin_amdgcn_readfirstlane(top_of[g]);  // newest sample of the group's window, relative to x_base
        const uint32_t tbase = static_cast<uint32_t>(g) * static_cast<uint32_t>(iters) * 128u;   // bytes: 4 steps x 8 floats per iteration
        f2 acc[kRS];
#pragma unroll
        for (int r = 0; r < kRS; r++) acc[r] = (f2){0.0f, 0.0f};
        f16v ta, tb, ua, ub;
        asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(ta) : "s"(table), "s"(tbase));
        asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(tb) : "s"(table), "s"(tbase + 64u));
        q4 gm[8], gs[8];                                             // batch in flight: 8 channels' quads per row
        // batch bt = samples top - 32 bt - 31 ... top - 32 bt of every channel
        auto fetch = [&](int bt) __attribute__((always_inline)) {
            const long first = static_cast<long>(top) - kSB * bt - (kSB - 1) + 4 * quad;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                gm[i] = *reinterpret_cast<const q4 *>(demod + cl[i] * dpitch + m_off + first);
                if (STEREO) gs[i] = *reinterpret_cast<const q4 *>(mixer + cl[i] * mpitch + s_off + first);
            }
        };
        auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    lds[(4 * quad + j) * kLP + 8 * i + sub] = gm[i][j];
                    if (STEREO) lds[kSB * kLP + (4 * quad + j) * kLP + 8 * i + sub] = gs[i][j];
                }
        };
        auto four_steps = [&](int t0, const f16v &h0, const f16v &h1) __attribute__((always_inline)) {
            float hq[32];
#pragma unroll
            for (int q = 0; q < 16; q++) {
                hq[q] = h0[q];
                hq[16 + q] = h1[q];
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int sidx = kSB - 1 - (t0 + e);                 // step t of the batch <-> its sample 31 - t (newest first)
                const float xm = lds[sidx * kLP + lane];
                const float xs = STEREO ? lds[kSB * kLP + sidx * kLP + lane] : 0.0f;
                const f2 w = (f2){xm, xs};
                if constexpr (STEREO) {                              // (mono, stereo) of output r in the two halves
#pragma unroll
                    for (int r = 0; r < kRS; r++) {
                        const float h = hq[8 * e + r];
                        if constexpr (!EXACT) {
                            acc[r] = __builtin_elementwise_fma(w, (f2){h, h}, acc[r]);
                        } else {
                            const f2 prod = w * (f2){h, h};
                            acc[r] = acc[r] + prod;
                        }
                    }
                } else {                                             // mono: outputs 2 q, 2 q + 1 in the two halves (the table's eighth tap is 0)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const f2 hh = (f2){hq[8 * e + 2 * q], hq[8 * e + 2 * q + 1]};
                        if constexpr (!EXACT) {
                            acc[q] = __builtin_elementwise_fma((f2){xm, xm}, hh, acc[q]);
                        } else {
                            const f2 prod = (f2){xm, xm} * hh;
                            acc[q] = acc[q] + prod;
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < kRS; r++) asm volatile("" : "+v"(acc[r]));
        };
        const int nb = iters / 8;                                    // batches per group (`iters` is a multiple of 8: host)
        fetch(0);
        for (int bt = 0; bt < nb; bt++) {
            stage();                                                 // (the previous batch's reads are done: one wave, program order)
            if (bt + 1 < nb) fetch(bt + 1);                          // in flight while this batch is multiplied
            const uint32_t tb0 = tbase + static_cast<uint32_t>(bt) * 1024u;   // 8 iterations x 128 bytes
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                // the taps of iteration i + 1 are requested while iteration i runs (the last request of a group reads the next
                // group's first iteration or the table's pad)
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(ta), "+s"(tb));
                asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(ua) : "s"(table), "s"(tb0 + static_cast<uint32_t>(i + 1) * 128u));
                asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(ub) : "s"(table), "s"(tb0 + static_cast<uint32_t>(i + 1) * 128u + 64u));
                four_steps(4 * i, ta, tb);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(ua), "+s"(ub));
                asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(ta) : "s"(table), "s"(tb0 + static_cast<uint32_t>(i + 2) * 128u));
                asm volatile("s_load_dwordx16 %0, %1, %2" : "=&s"(tb) : "s"(table), "s"(tb0 + static_cast<uint32_t>(i + 2) * 128u + 64u));
                four_steps(4 * i + 4, ua, ub);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(ta), "+s"(tb));   // the look-ahead's loads land before the registers are reused
        if (c_raw < n_channels) {
            const long k0 = k_base + static_cast<long>(g) * kRS;
#pragma unroll
            for (int r = 0; r < kRS; r++) {
                const float am = STEREO ? acc[r].x : acc[r / 2][r % 2];
                const float gm = am * fu;                            // y += y * U  (src/filter.cpp:213)
                const float mono = am + gm;
                if constexpr (STEREO) {
                    const float gs = acc[r].y * fu;
                    const float st = acc[r].y + gs;
                    const float l = st + mono, rr = mono - st;       // src/project.cpp:278-279
                    if (audio) {
                        audio[c * 2 * n_out + k0 + r] = l;
                        audio[c * 2 * n_out + n_out + k0 + r] = rr;
                    }
                    if (pcm) {
                        pcm[2 * (c * n_out + k0 + r)] = pcm_pack_flat(l, wrap);
                        pcm[2 * (c * n_out + k0 + r) + 1] = pcm_pack_flat(rr, wrap);
                    }
                } else {
                    if (audio) audio[c * n_out + k0 + r] = mono;
                    if (pcm) pcm[c * n_out + k0 + r] = pcm_pack_flat(mono, wrap);
                }
            }
        }
    }
}

// carried state: per channel, history <- the slot's last hist_bytes bytes; demod history <- the row's last Hd samples
// (create() rejects blocks shorter than either history, so source and destination never overlap)
__global__ void chs_finish_kernel(uint8_t *__restrict__ slots, long slot_bytes, long hist_bytes, float *__restrict__ demod,
                                  long dpitch, int Hd, long n_if, float *__restrict__ mixer, long mpitch, int hm)
{
    const long c = blockIdx.x;
    uint8_t *slot = slots + c * slot_bytes;
    const u4 *src = reinterpret_cast<const u4 *>(slot + slot_bytes - hist_bytes);
    u4 *dst = reinterpret_cast<u4 *>(slot);
    for (long i = threadIdx.x; i < hist_bytes / 16; i += blockDim.x) dst[i] = src[i];
    float *row = demod + c * dpitch;
    for (long i = threadIdx.x; i < Hd; i += blockDim.x) row[i] = row[n_if + i];
    if (mixer) {                                                   // resampling modes: state_stereofilt = the mixer row's tail
        float *mr = mixer + c * mpitch;
        for (long i = threadIdx.x; i < hm; i += blockDim.x) mr[i] = mr[n_if + i];
    }
}

// the fused kind's finish.  Per channel: history <- the slot's last hist_bytes bytes; audio / PCM of the slot, minus the junk in front,
// -> the caller's contiguous per-channel arrays.  Workgroups [c * gx, (c + 1) * gx) serve channel c: the channel rides in the
// grid's x, which has room for any bank (y and z end at 65 535, and a bank may have more receivers than that)
__global__ void channels_finish_kernel(uint8_t *__restrict__ slots, long slot_bytes, long hist_bytes, const float *__restrict__ audio_all,
                                       const int16_t *__restrict__ pcm_all, long slot_audio, long junk_audio, long n_audio,
                                       float *__restrict__ audio_out, int16_t *__restrict__ pcm_out, unsigned gx)
{
    const long c = blockIdx.x / gx;
    const unsigned bx = blockIdx.x - static_cast<unsigned>(c) * gx;
    uint8_t *slot = slots + c * slot_bytes;
    const long t = static_cast<long>(bx) * blockDim.x + threadIdx.x, nt = static_cast<long>(gx) * blockDim.x;
    const long so = c * slot_audio + junk_audio, dof = c * n_audio;   // first element of this channel: source, destination
    // four outputs per access where source and destination allow it (8-byte s16 / 16-byte f32 pieces): true for every reference
    // shape (52 600 / 1 024 elements per slot / channel, 28 in front)
    if (n_audio % 4 == 0 && so % 4 == 0 && dof % 4 == 0 && (!pcm_out || (reinterpret_cast<uintptr_t>(pcm_out) % 8 == 0 &&
        reinterpret_cast<uintptr_t>(pcm_all) % 8 == 0)) && (!audio_out || (reinterpret_cast<uintptr_t>(audio_out) % 16 == 0 &&
        reinterpret_cast<uintptr_t>(audio_all) % 16 == 0))) {
        typedef short s4v __attribute__((ext_vector_type(4)));
        typedef float f4v __attribute__((ext_vector_type(4)));
        for (long k = t; k < n_audio / 4; k += nt) {
            if (audio_out) reinterpret_cast<f4v *>(audio_out + dof)[k] = reinterpret_cast<const f4v *>(audio_all + so)[k];
            if (pcm_out) reinterpret_cast<s4v *>(pcm_out + dof)[k] = reinterpret_cast<const s4v *>(pcm_all + so)[k];
        }
    } else {
        for (long k = t; k < n_audio; k += nt) {
            if (audio_out) audio_out[dof + k] = audio_all[so + k];
            if (pcm_out) pcm_out[dof + k] = pcm_all[so + k];
        }
    }
    // history: 16-byte pieces; source and destination overlap only if the block is shorter than the history, which
    // create() rejects, so a plain copy is safe whatever the order
    const u4 *src = reinterpret_cast<const u4 *>(slot + slot_bytes - hist_bytes);
    u4 *dst = reinterpret_cast<u4 *>(slot);
    if (bx == 0)
        for (long i = threadIdx.x; i < hist_bytes / 16; i += blockDim.x) dst[i] = src[i];
}

__global__ void chs_fill_state_kernel(float *__restrict__ pll, long n)
{
    const long i = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int u = static_cast<int>(i % 8);
    pll[i] = (u == 2 || u == 4) ? 1.0f : 0.0f;                 // state_PLL = {0, 0, 1, 0, 1, 0}  (src/project.cpp:458); fast banks' fr = 0
}

}  // namespace

// ---- host side: tap tables, launchers, and the resolver from a bank's shapes to both ---------------------------------
namespace {

int upload(DevBuf<float> &d, const std::vector<float> &tab)
{
    FMRX_TRY(d.alloc(tab.size()));
    FMRX_HIP(hipMemcpy(d.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    return FMRX_OK;
}

// The step-major table of fex_step / outx_step (C = FeX / OutX): step u visits window sample W-1-u, where output r meets
// tap n = r D + (T-1) - (W-1-u); entry [u][r] = h[n] * scale, 0 where n is out of range; whole scalar loads of 16 entries.
template <template <int, int> class C, int T, int D>
std::vector<float> step_major_table(const float *h, float scale)
{
    using S = C<T, D>;
    std::vector<float> tab(static_cast<size_t>(S::NG) * 16, 0.0f);
    for (int u = 0; u < S::W; u++)
        for (int r = 0; r < S::R; r++) {
            const int n = r * D + (T - 1) - (S::W - 1 - u);
            if (n >= 0 && n < T) tab[static_cast<size_t>(u) * S::R + r] = h[n] * scale;
        }
    return tab;
}

template <int T, int D>
int fe_table_init(Bank &b, const float *h)
{
    for (int n = 0; n < T; n++) {
        const float a = std::fabs(h[n]);
        if (a != 0.0f && !(a >= 7.8886091e-31f && a <= 1.2676506e30f))   // 2^-100 .. 2^100
            return fail(FMRX_EINVAL, "channels (exact): rf tap %d = %g is outside the range in which h/128 * (u-128) is the reference's product", n, h[n]);
    }
    return upload(b.fe_table, step_major_table<FeX, T, D>(h, 0.0078125f));
}

template <int T>
int bpf_table_init(Bank &b, const float *h_st, const float *h_car)
{
    using C = BpX<T>;
    // P[m] = (h_st, h_car)[m - (R-1)], zero outside the filter, in groups of eight pairs; two groups of padding behind the last block
    constexpr int NBLK = (C::W + 7) / 8;
    std::vector<float> tab(static_cast<size_t>(NBLK + 2) * 16, 0.0f);
    for (int m = 0; m < (NBLK + 2) * 8; m++) {
        const int n = m - (kR - 1);
        if (n >= 0 && n < T) {
            tab[2 * static_cast<size_t>(m)] = h_st[n];
            tab[2 * static_cast<size_t>(m) + 1] = h_car[n];
        }
    }
    return upload(b.bpf_table, tab);
}

// The resampling modes' tables: the plain audio taps, and where the ratio allows it the
// step-major taps of chs_resample_lanes_kernel: [group of the period][step][8] (7 outputs + pad), steps newest sample first,
// rounded up to whole iterations of 4 (+ one iteration of zeros that the kernel's look-ahead reads); top_of[group] = the window's
// newest sample relative to the period's first
int resample_table_init(Bank &b, const float *h)
{
    const int U = b.p.audio_upsamp, D = b.p.audio_decim, T = b.p.audio_taps;
    FMRX_TRY(upload(b.h_res, std::vector<float>(h, h + T)));
    if (U <= 0 || U % kRS) return FMRX_OK;                         // other ratios: the one-thread-per-output kernel
    const int G = U / kRS;
    std::vector<int> top(G), n_of(U), ph_of(U);
    int wmax = 0;
    for (int k = 0; k < U; k++) {
        const long m = static_cast<long>(k) * D;
        ph_of[k] = static_cast<int>(m % U);
        n_of[k] = static_cast<int>((m - ph_of[k]) / U);
    }
    for (int g = 0; g < G; g++) {
        top[g] = n_of[g * kRS + kRS - 1];
        for (int r = 0; r < kRS; r++) {
            const int k = g * kRS + r, jmax = (T - 1 - ph_of[k]) / U;   // taps ph, ph + U, ..., ph + jmax U
            const int w = top[g] - (n_of[k] - jmax) + 1;
            if (w > wmax) wmax = w;
        }
    }
    const int iters = ((wmax + 3) / 4 + 7) / 8 * 8;                // whole iterations of 4 steps, in batches of 8 (32 samples)
    // the oldest sample the kernel touches lies 4 iters - 1 behind a group's top: the rows' histories cover it
    for (int g = 0; g < G; g++)
        if (4 * iters - 1 - top[g] > b.res_hist) b.res_hist = 4 * iters - 1 - top[g];
    std::vector<float> tab(static_cast<size_t>(G) * iters * 32 + 32, 0.0f);
    for (int g = 0; g < G; g++)
        for (int st = 0; st < 4 * iters; st++)
            for (int r = 0; r < kRS; r++) {
                const int k = g * kRS + r, j = n_of[k] - (top[g] - st);
                const long n = static_cast<long>(ph_of[k]) + static_cast<long>(j) * U;
                if (j >= 0 && n < T) tab[(static_cast<size_t>(g) * iters * 4 + st) * 8 + r] = h[n];
            }
    FMRX_TRY(upload(b.res_table, tab));
    FMRX_TRY(b.res_top.alloc(G));
    FMRX_HIP(hipMemcpy(b.res_top.p, top.data(), G * sizeof(int), hipMemcpyHostToDevice));
    b.res_groups = G;
    b.res_iters = iters;
    return FMRX_OK;
}

#define CHS_FE_CASES(X) X(101, 10) X(101, 5) X(101, 3) X(151, 10) X(151, 5) X(151, 3) X(13, 10) X(13, 5) X(13, 3)
#define CHS_BPF_CASES(X) X(101) X(151) X(13)
#define CHS_OUT_CASES(X) X(101, 5) X(101, 6) X(13, 5) X(13, 6)

// IF outputs [k_lo, k_hi) of every channel's block
template <int T, int D>
int launch_fe(const Bank &b, long k_lo, long k_hi, hipStream_t s)
{
    using C = FeX<T, D>;
    const long ntiles = (k_hi - k_lo + C::TILE - 1) / C::TILE;   // one workgroup each
    hipLaunchKernelGGL((chs_fe_exact_kernel<T, D>), dim3(static_cast<unsigned>(ntiles * b.n_channels)), dim3(64), 0, s, b.slots.p,
                       static_cast<long>(b.slot_bytes), static_cast<int>(b.hist_bytes), k_lo, k_hi, ntiles, ntiles, b.fe_table.p, b.demod.p,
                       b.dpitch, b.Hd);
    FMRX_LAUNCH_CHECK("chs_fe_exact_kernel");
    return FMRX_OK;
}

// fast banks: the matrix-core front end (kernels_fe_mfma.hip) over the same slots and rows
int launch_fe_mfma(const Bank &b, long k_lo, long k_hi, hipStream_t s)
{
    return fe_mfma_bank_launch(b.fe, b.slots.p, static_cast<long>(b.slots.n), static_cast<long>(b.slot_bytes),
                               static_cast<long>(b.hist_bytes), b.n_channels, k_lo, k_hi, b.demod.p, b.dpitch, b.Hd, s);
}

// (the pilot band-pass output: exact banks keep the float row `carrier`, fast banks the sign row `carrier8`; the other is null)
template <int T, bool EXACT>
int launch_bpf(const Bank &b, long k_lo, long k_hi, hipStream_t s)
{
    const long wgs = (k_hi - k_lo + 64 * kR - 1) / (64 * kR);
    hipLaunchKernelGGL((chs_bpf_kernel<T, EXACT>), dim3(static_cast<unsigned>(wgs * b.n_channels)), dim3(64), 0, s, b.demod.p, b.dpitch,
                       b.Hd, k_lo, k_hi, wgs, b.bpf_table.p, b.bpf.p, b.carrier.p, b.ypitch, b.carrier8.p, b.cpitch);
    FMRX_LAUNCH_CHECK("chs_bpf_kernel");
    return FMRX_OK;
}

// audio outputs [a_lo, a_hi) of every channel's block, from the IF samples [.., g_hi)
template <int T, int D, bool STEREO, bool EXACT>
int launch_out(Bank &b, float *d_audio, int16_t *d_pcm, int wrap, long a_lo, long a_hi, long g_hi, hipStream_t s)
{
    using C = OutX<T, D>;
    if ((reinterpret_cast<uintptr_t>(d_audio) % 16) || (reinterpret_cast<uintptr_t>(d_pcm) % 16) || (STEREO && b.n_audio % 4))
        return fail(FMRX_EINVAL, "channels: output buffers must be 16-byte aligned");
    const long wgs = (a_hi - a_lo + C::NOUT - 1) / C::NOUT;
    hipLaunchKernelGGL((chs_out_kernel<T, D, STEREO, EXACT>), dim3(static_cast<unsigned>(wgs * b.n_channels)), dim3(64), 0, s, b.demod.p,
                       b.dpitch, b.Hd, b.bpf.p, b.trig.p, b.ypitch, b.nco0.p, b.mixtail[b.mix_cur].p, b.mixtail[b.mix_cur ^ 1].p, b.Hm,
                       b.n_if, g_hi, b.delay, kNcoScale, kPhaseAdjust, b.out_table.p, wgs, d_audio, d_pcm, wrap, a_lo, a_hi, b.n_audio);
    FMRX_LAUNCH_CHECK("chs_out_kernel");
    return FMRX_OK;
}

// convolveBlockResampleFIR for the audio outputs [a_lo, a_hi) of every channel (a_lo: a multiple of U): whole periods by the
// lane-per-channel kernel when its table exists, what is left (and every other ratio) by one thread per (channel, output).
// (g_hi: the launchers' common signature; the mixer rows of this chunk were written by its NCO pass, bank_launch_nco)
template <bool STEREO, bool EXACT>
int launch_resample(Bank &b, float *d_audio, int16_t *d_pcm, int wrap, long a_lo, long a_hi, long /*g_hi*/, hipStream_t s)
{
    const fmrx_params &p = b.p;
    long done = a_lo;
    if (b.res_groups > 0 && a_lo % p.audio_upsamp == 0) {
        const long periods = (a_hi - a_lo) / p.audio_upsamp;
        if (periods > 0) {
            const long cgs = (b.n_channels + 63) / 64;
            // a wave takes `gpw` consecutive groups of a period (neighbouring groups share most of their window): as many as leave
            // the chip >= 8 waves per SIMD
            // (tests/test_gpu_mono_banks_exact.py: groups_per_wave() states this rule and derives its multi-group shapes from it)
            int gpw = b.res_groups;
            constexpr int NW = kRW<STEREO>;
            while (gpw > NW && cgs * periods * ((b.res_groups + gpw - 1) / gpw) * NW < 8192) gpw = (gpw + 1) / 2;
            gpw = (gpw + NW - 1) / NW * NW;                        // every wave of a workgroup gets a group
            const long parts = (b.res_groups + gpw - 1) / gpw;
            hipLaunchKernelGGL((chs_resample_lanes_kernel<STEREO, EXACT>), dim3(static_cast<unsigned>(cgs * periods * parts)),
                               dim3(64 * kRW<STEREO>), 0, s, b.demod.p, b.dpitch, b.Hd, STEREO ? b.mixer.p : nullptr, b.mpitch, b.Hm, b.delay, b.res_table.p,
                               b.res_top.p, b.res_groups, gpw, b.res_iters, p.audio_decim, p.audio_upsamp, periods, b.n_channels, d_audio, d_pcm,
                               wrap, a_lo, b.n_audio);
            FMRX_LAUNCH_CHECK("chs_resample_lanes_kernel");
            done = a_lo + periods * p.audio_upsamp;
        }
    }
    if (done < a_hi) {
        const long wr = (a_hi - done + 255) / 256;
        hipLaunchKernelGGL(chs_resample_exact_kernel<STEREO>, dim3(static_cast<unsigned>(wr * b.n_channels)), dim3(256), 0, s, b.demod.p, b.dpitch,
                           b.Hd, STEREO ? b.mixer.p : nullptr, b.mpitch, b.Hm, b.delay, b.h_res.p, p.audio_taps, p.audio_decim, p.audio_upsamp, wr,
                           d_audio, d_pcm, wrap, done, a_hi, b.n_audio);
        FMRX_LAUNCH_CHECK("chs_resample_exact_kernel");
    }
    return FMRX_OK;
}

}  // namespace

// The one place the shape lists are expanded.  Fast banks keep the exact front end's table and history (its tap-range check
// and slot layout hold for them too) and launch the matrix-core front end.  The fast mono bank of modes 0/1 is the fused kind:
// decided here and nowhere else; whether the fused mono kernel has its shapes is asked when its plans exist (bank_create).
bool bank_resolve(const fmrx_params &p, int audio_channels, int exact, BankKernels &k)
{
    const bool stereo = audio_channels == 2;
    k = BankKernels{};
    k.fused = !stereo && !exact && p.audio_upsamp == 0;
    if (k.fused) return true;
#define X(T_, D_) \
    if (p.rf_taps == T_ && p.rf_decim == D_) { k.hist_bytes = FeX<T_, D_>::HIST; k.fe_table = fe_table_init<T_, D_>; k.fe = exact ? launch_fe<T_, D_> : launch_fe_mfma; }
    CHS_FE_CASES(X)
#undef X
#define X(T_) if (stereo && p.stereo_taps == T_) { k.bpf_table = bpf_table_init<T_>; k.bpf = exact ? launch_bpf<T_, true> : launch_bpf<T_, false>; }
    CHS_BPF_CASES(X)
#undef X
#define X(T_, D_)                                                                                                        \
    if (p.audio_upsamp == 0 && p.audio_taps == T_ && p.audio_decim == D_) {                                              \
        k.out_table = [](Bank &b, const float *h) { return upload(b.out_table, step_major_table<OutX, T_, D_>(h, 1.0f)); };  \
        k.out = stereo ? (exact ? launch_out<T_, D_, true, true> : launch_out<T_, D_, true, false>) : launch_out<T_, D_, false, true>; \
    }
    CHS_OUT_CASES(X)
#undef X
    if (p.audio_upsamp > 0 && p.audio_taps >= 2 && p.audio_taps <= 65535) {   // resampling modes: the batched reference-order resampler takes any taps
        k.out_table = resample_table_init;
        k.out = stereo ? (exact ? launch_resample<true, true> : launch_resample<true, false>) : (exact ? launch_resample<false, true> : launch_resample<false, false>);
    }
    return k.fe && k.out && (!stereo || k.bpf);
}

int bank_launch_nco(bool exact, float *trig, long ypitch, int n_rows, long k_lo, long k_hi, const float *bpf, const float *nco0,
                    float *mixer, long mpitch, int hm, hipStream_t s)
{
    const long wgs = (k_hi - k_lo + 1023) / 1024;
    auto go = [&](auto exactc) {
        hipLaunchKernelGGL(chs_nco_kernel<decltype(exactc)::value>, dim3(static_cast<unsigned>(wgs * n_rows)), dim3(256), 0, s, trig, ypitch,
                           k_lo, k_hi, wgs, kNcoScale, kPhaseAdjust, bpf, nco0, mixer, mpitch, hm);
    };
    if (exact) go(std::true_type{});
    else go(std::false_type{});
    FMRX_LAUNCH_CHECK("chs_nco_kernel");
    return FMRX_OK;
}

int bank_launch_finish(const Bank &b, float *d_audio, int16_t *d_pcm, hipStream_t s)
{
    if (b.k.fused) {
        // workgroups per channel: four outputs per thread where the shapes allow it (see the kernel), 8 at the most -- times
        // n_channels they fit the grid's x (2^31 - 1) for every bank whose slots fit a device's memory
        const long g = ((b.n_audio + 3) / 4 + 255) / 256;
        const unsigned gx = static_cast<unsigned>(g < 1 ? 1 : g < 8 ? g : 8);
        hipLaunchKernelGGL(channels_finish_kernel, dim3(gx * static_cast<unsigned>(b.n_channels)), dim3(256), 0, s, b.slots.p,
                           static_cast<long>(b.slot_bytes), static_cast<long>(b.hist_bytes), b.audio_all.p, b.pcm_all.p,
                           static_cast<long>(b.junk_audio) + b.n_audio, static_cast<long>(b.junk_audio), b.n_audio, d_audio, d_pcm, gx);
        FMRX_LAUNCH_CHECK("channels_finish_kernel");
        return FMRX_OK;
    }
    hipLaunchKernelGGL(chs_finish_kernel, dim3(static_cast<unsigned>(b.n_channels)), dim3(64), 0, s, b.slots.p,
                       static_cast<long>(b.slot_bytes), static_cast<long>(b.hist_bytes), b.demod.p, b.dpitch, b.Hd, b.n_if,
                       b.resample && b.audio_channels == 2 ? b.mixer.p : nullptr, b.mpitch, b.Hm);
    FMRX_LAUNCH_CHECK("chs_finish_kernel");
    return FMRX_OK;
}

int bank_launch_fill_state(float *pll, long n, hipStream_t s)
{
    hipLaunchKernelGGL(chs_fill_state_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, s, pll, n);
    FMRX_LAUNCH_CHECK("chs_fill_state_kernel");
    return FMRX_OK;
}

}  // namespace fmrx
