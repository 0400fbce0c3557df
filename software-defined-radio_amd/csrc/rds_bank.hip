// rds_bank.hip -- the RDS chain of N channels per device call: the chain itself (rds_chain.hpp), which the single-stream handle
// (rds.hip: include/fmrx.h fmrx_rds_*) runs with one channel, and the bank around it (fmrx_rds_bank_*).
//
// A receiver bank (bank.hip) demodulates 10^4 - 10^5 stations per call; the chain gives each of them the float64
// arithmetic of the reference's model (rds.hip lists the stages) in a FIXED number of launches, whatever the number of channels
// (tests/_rds_stage_model.py is the model of every stage's order of operations):
//   rdsb_cvt_kernel         f32 demod rows (caller's pitch) -> f64 rows behind their histories
//   rdsb_fir_kernel<0>      54-60 kHz channel band-pass, 151 taps
//   rdsb_fir_kernel<1>      113.5-114.5 kHz band-pass of the squared channel row
//   rdsb_pll_lanes_kernel   the 114 kHz PLL, ONE LANE PER CHANNEL (64 channels per wave)
//   rdsb_mix_kernel         NCO pair, I / Q mixers
//   rdsb_resample_kernel    rational resampler U/D, 101*U taps, gain U, I and Q
//   rdsb_fir_kernel<0>      root-raised-cosine matched filter, I and Q (grid z)
//   rdsb_cdr_kernel         the bank only: clock and data recovery, Manchester and differential decoding, one lane per channel
//                           (the host cdr(), which the single-stream handle calls)
//   rdsb_tail_kernel        carried state: every row's tail -> its history
//   rdsb_station_kernel     the bank with stations on only: the station decoder of rds_station.hpp, one lane per channel
//                           (fmrx_rds_station_*)
// Frame synchronisation stays on the host (fmrx_rds_bank_collect), ~190 new bits per channel and call.
//
// Data layout: channel-major float64 rows, the carried history (raw samples) in front of the block and
// a few samples of padding behind it (the register-window FIRs read up to kR - 2 samples past the block; results discarded):
//   x      [N][Hx | n | pad]     converted discriminator output          ch     [N][Hc | n | pad]    channel band-pass
//   car    [N][n | pad]          carrier band-pass (squared input)       arg    [N][n | pad]         raw trigArg of every PLL step
//   nco_i, nco_q [N][n+1 | pad]  NCO pair, [0] = previous call's last    mi, mq [N][Hm | n | pad]    mixer rows
//   ri, rq [N][Hr | n_out | pad] resampler output                        yi, yq [N][n_out | pad]     matched-filter output
//   state  [N][8]                {integ, phase, fI, fQ, nco_i[n], off, nco_q[n], trigArg}
//   bits   u8 [N][max_bits], n_bits u32 [N], blk i32 [N] (0 until a channel's first call: the CDR's block_count != 0 test)
#include "fmrx_internal.hpp"
#include "rds_chain.hpp"
#include "rds_common.hpp"
#include "rds_station.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

using namespace fmrx;
using namespace fmrx::rds;

namespace {

constexpr int kR = 4;        // consecutive outputs per thread of the FIR kernels
constexpr int kPllB = 32;    // samples per lane and batch of the PLL lanes (two 128-byte lines of a double row)
constexpr int kStB = 32;     // samples per lane and batch of the station lanes

typedef double d2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void rdsb_cvt_kernel(const float *__restrict__ in, long in_pitch, long n, double *__restrict__ x, long xpitch)
{
    const long c = blockIdx.x, i = static_cast<long>(blockIdx.y) * blockDim.x + threadIdx.x;
    if (i < n) x[c * xpitch + i] = static_cast<double>(in[c * in_pitch + i]);
}

// y[k] = sum_j h[j] * f(x[k-j]), f = identity or square, in the order lfilter's transposed form adds them up
// (acc = h[j]*v + acc, j from taps-1 down to 0).
// A thread owns kR consecutive outputs and slides one register window over x: the window of step j is x[k0-j .. k0-j+kR-1],
// one new sample per step, so every sample is loaded (and squared) once for all kR outputs while each output still meets its
// taps in that order.  x, y: the block's first sample of channel 0's row (blockIdx.x = channel); blockIdx.z
// selects the second (x, y) pair (the matched filter runs I and Q in one launch).  Reads x[-(taps-1) .. n+kR-2].
template <bool SQUARE>
__global__ __launch_bounds__(256) void rdsb_fir_kernel(const double *__restrict__ x0, const double *__restrict__ x1, long xpitch, long n,
                                                       const double *__restrict__ h, int taps, double *__restrict__ y0, double *__restrict__ y1,
                                                       long ypitch)
{
    const long c = blockIdx.x, k0 = (static_cast<long>(blockIdx.y) * blockDim.x + threadIdx.x) * kR;
    if (k0 >= n) return;
    const double *x = (blockIdx.z ? x1 : x0) + c * xpitch + k0;
    double *y = (blockIdx.z ? y1 : y0) + c * ypitch + k0;
    double w[kR], acc[kR];
#pragma unroll
    for (int r = 0; r < kR; r++) {
        const double v = x[r - (taps - 1)];
        w[r] = SQUARE ? v * v : v;
        acc[r] = 0.0;
    }
    for (int j = taps - 1; j >= 0; j--) {
        const double hj = h[j];
#pragma unroll
        for (int r = 0; r < kR; r++) acc[r] = hj * w[r] + acc[r];
        if (j) {
#pragma unroll
            for (int r = 0; r + 1 < kR; r++) w[r] = w[r + 1];
            const double v = x[kR - j];
            w[kR - 1] = SQUARE ? v * v : v;
        }
    }
#pragma unroll
    for (int r = 0; r < kR; r++)
        if (k0 + r < n) y[r] = acc[r];
}

// The recurrence of fmPll (fmSupportLib.py:297-353) in float64, ONE LANE PER CHANNEL.  The carrier row
// arrives a batch ahead through registers into LDS and the chain touches LDS only; the state stays in
// registers (the step is written out in the loop: no call, nothing in scratch).  Also: nco[0] <- the incoming state's last NCO
// pair, and the outgoing one computed from the last trigArg.
// Rows are 16-byte aligned (even pitches).
__global__ __launch_bounds__(64) void rdsb_pll_lanes_kernel(const double *__restrict__ car, long apitch, long n, int n_ch, double *__restrict__ arg,
                                                            double *__restrict__ state, double *__restrict__ nco_i, double *__restrict__ nco_q,
                                                            long npitch, double freq, double Fs, double normBandwidth, double ncoScale,
                                                            double phaseAdjust)
{
    __shared__ double lin[kPllB * 64], lout[kPllB * 64];     // [sample][lane]: every lane reads and writes its own column
    const int lane = threadIdx.x;
    const long ch = static_cast<long>(blockIdx.x) * 64 + lane;
    if (ch >= n_ch) return;
    const double Kp = normBandwidth * 2.666, Ki = normBandwidth * normBandwidth * 3.555;
    const double w = 2 * kPi * (freq / Fs);
    double *st = state + 8 * ch;
    double integ = st[0], phase = st[1], fI = st[2], fQ = st[3], off = st[5], last = 0.0;
    nco_i[ch * npitch] = st[4];
    nco_q[ch * npitch] = st[6];
    const double *in = car + ch * apitch;
    double *out = arg + ch * apitch;
    const d2 *in2 = reinterpret_cast<const d2 *>(in);
    d2 *out2 = reinterpret_cast<d2 *>(out);
    const long nb = n / kPllB;
    d2 pre[kPllB / 2];
    if (nb > 0) {
#pragma unroll
        for (int g = 0; g < kPllB / 2; g++) pre[g] = in2[g];
    }
    for (long b = 0; b < nb; b++) {
        // (1) this batch's input -> LDS (requested a batch ago); (2) request the next batch
#pragma unroll
        for (int g = 0; g < kPllB / 2; g++) {
            lin[(2 * g) * 64 + lane] = pre[g].x;
            lin[(2 * g + 1) * 64 + lane] = pre[g].y;
        }
        if (b + 1 < nb) {
#pragma unroll
            for (int g = 0; g < kPllB / 2; g++) pre[g] = in2[(b + 1) * (kPllB / 2) + g];
        }
        // (3) the previous batch's output -> memory (its stores have this whole batch to complete)
        if (b > 0) {
#pragma unroll
            for (int g = 0; g < kPllB / 2; g++) out2[(b - 1) * (kPllB / 2) + g] = (d2){lout[(2 * g) * 64 + lane], lout[(2 * g + 1) * 64 + lane]};
        }
        // (4) the chain: LDS in, LDS out
#pragma unroll 1
        for (int j = 0; j < kPllB; j++) {
            const double xk = lin[j * 64 + lane];
            const double eD = atan2(xk * (-fQ), xk * (+fI));
            integ = integ + Ki * eD;
            phase = phase + Kp * eD + integ;
            off += 1;
            last = w * off + phase;
            sincos(last, &fQ, &fI);
            lout[j * 64 + lane] = last;
        }
    }
    if (nb > 0) {
#pragma unroll
        for (int g = 0; g < kPllB / 2; g++) out2[(nb - 1) * (kPllB / 2) + g] = (d2){lout[(2 * g) * 64 + lane], lout[(2 * g + 1) * 64 + lane]};
    }
    for (long k = nb * kPllB; k < n; k++) {                   // what is left of a block that is not a multiple of the batch
        const double xk = in[k];
        const double eD = atan2(xk * (-fQ), xk * (+fI));
        integ = integ + Ki * eD;
        phase = phase + Kp * eD + integ;
        off += 1;
        last = w * off + phase;
        sincos(last, &fQ, &fI);
        out[k] = last;
    }
    double s, cs;
    sincos(last * ncoScale + phaseAdjust, &s, &cs);          // = nco[n] of this call, the next call's nco[0]
    st[0] = integ; st[1] = phase; st[2] = fI; st[3] = fQ; st[4] = cs; st[5] = off; st[6] = s; st[7] = last;
}

// NCO pair and mixers: nco[i+1] = cos / sin(arg[i]*ncoScale + phaseAdjust); mixer[i] = nco[i] * allpass[i] * 2, allpass = the
// channel row delayed by `delay`.  Thread i computes nco[i+1] and mixer[i+1]; thread 0 also mixer[0] (nco[0]: the PLL lanes).
// ch, mi, mq: the block's first sample of channel 0's row.
__global__ __launch_bounds__(256) void rdsb_mix_kernel(const double *__restrict__ arg, long apitch, long n, const double *__restrict__ ch, long cpitch,
                                                       int delay, double ncoScale, double phaseAdjust, double *__restrict__ nco_i,
                                                       double *__restrict__ nco_q, long npitch, double *__restrict__ mi, double *__restrict__ mq,
                                                       long mpitch)
{
    const long c = blockIdx.x, i = static_cast<long>(blockIdx.y) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *chr = ch + c * cpitch;
    double *ni = nco_i + c * npitch, *nq = nco_q + c * npitch, *mir = mi + c * mpitch, *mqr = mq + c * mpitch;
    double s, cs;
    sincos(arg[c * apitch + i] * ncoScale + phaseAdjust, &s, &cs);
    ni[i + 1] = cs;
    nq[i + 1] = s;
    if (i + 1 < n) {
        const double ap = chr[i + 1 - delay];
        mir[i + 1] = cs * ap * 2;
        mqr[i + 1] = s * ap * 2;
    }
    if (i == 0) {
        const double ap = chr[-delay];
        mir[0] = ni[0] * ap * 2;
        mqr[0] = nq[0] * ap * 2;
    }
}

// convolveBlockResampleFIR of the model (fmSupportLib.py:388-407) in stream form, gain U: one phase walk per output, I and
// Q together (same taps, same window).  mi, mq, ri, rq: the block's first sample of channel 0's row.
__global__ __launch_bounds__(256) void rdsb_resample_kernel(const double *__restrict__ mi, const double *__restrict__ mq, long mpitch, long n_out,
                                                            const double *__restrict__ h, int taps, int decim, int upsamp, double *__restrict__ ri,
                                                            double *__restrict__ rq, long rpitch)
{
    const long c = blockIdx.x, k = static_cast<long>(blockIdx.y) * blockDim.x + threadIdx.x;
    if (k >= n_out) return;
    const long m = k * decim;
    const int ph = static_cast<int>(m % upsamp);
    const long b = m / upsamp;
    const double *xi = mi + c * mpitch + b, *xq = mq + c * mpitch + b;
    double acc_i = 0.0, acc_q = 0.0;
    long j = 0;
    for (int t = ph; t < taps; t += upsamp, j++) {
        const double ht = h[t];
        acc_i = acc_i + ht * xi[-j];
        acc_q = acc_q + ht * xq[-j];
    }
    ri[c * rpitch + k] = acc_i * upsamp;
    rq[c * rpitch + k] = acc_q * upsamp;
}

// Clock and data recovery of the model (fmSupportLib.py:103-249, the host cdr() in rds_common.cpp), ONE LANE PER CHANNEL, on the
// in-phase matched-filter row, then differential decoding in place.  The host function materialises the sampled points and
// re-scans them from the top after every restart; here one pass per attempt carries what the scan reads (the two previous
// points for the three-in-a-row flip, the pair being formed) in registers and writes the Manchester bits as it goes -- an
// attempt that fails is overwritten by the next one, which starts one symbol later behind one more head bit (block_count != 0).
// state {pair0, pair1, start0, prev_size}: what fmrx_rds_process re-makes every block.  blk[c] != 0 after a channel's first call.
__global__ __launch_bounds__(64) void rdsb_cdr_kernel(const double *__restrict__ y, long ypitch, long n, int n_ch, int sps, double pair0_in,
                                                      double pair1_in, long start0, long prev_size, int *__restrict__ blk,
                                                      uint8_t *__restrict__ bits, long max_bits, uint32_t *__restrict__ n_bits)
{
    const long ch = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (ch >= n_ch) return;
    const double *x = y + ch * ypitch;
    uint8_t *out = bits + ch * max_bits;
    const bool counted = blk[ch] != 0;
    double pair0 = pair0_in, pair1 = pair1_in;
    long start = start0, nh = 0;
    auto put = [&](long i, int v) {
        if (i < max_bits) out[i] = static_cast<uint8_t>(v);
    };
    if (prev_size % 2 == 1 && start < n) {   // the point that completes the previous block's pair
        pair1 = x[start];
        put(nh++, pair0 > 0 ? 1 : 0);
        pair0 = pair1;
        start += sps;
    }
    long nm = nh;
    for (;;) {
        double a = 0.0, b = 0.0, s0 = 0.0;   // the two previous points (as flipped by the three-in-a-row rule); samples[0] as mended
        bool failed = false;
        long m = 0;
        nm = nh;
        for (long i = start; i < n; i += sps, m++) {
            const double xi = x[i];
            double p;
            if (m >= 2 && a > 0 && b > 0 && xi > 0) p = -xi;           // the third of three high / low points is flipped
            else if (m >= 2 && a < 0 && b < 0 && xi < 0) p = -xi;
            else p = xi;
            if (m == 0) s0 = p;
            if (m & 1) {                                               // the pair (samples[m-1], samples[m])
                double q0 = b, q1 = p;
                if ((q0 < 0 && q1 < 0) || (q0 > 0 && q1 > 0)) {
                    if (fabs(q0) < 0.3 || fabs(q1) < 0.3) {
                        if (fabs(q0) < 0.3) q0 = -q0;
                        else q1 = -q1;
                    } else {                                           // cannot be mended: re-start one symbol later
                        failed = true;
                        break;
                    }
                }
                if (m == 1) s0 = q0;
                put(nm++, (q0 > 0 && q1 < 0) ? 1 : 0);                // manchestering
            }
            a = b;
            b = p;
        }
        if (!failed) break;
        start += sps;
        if (counted) {
            pair1 = s0;
            put(nh++, pair0 > 0 ? 1 : 0);
            pair0 = pair1;
        }
    }
    if (nm > max_bits) nm = max_bits;                                  // (cannot happen: max_bits = n/sps + 4 > every count)
    for (long i = nm - 1; i > 0; i--) out[i] = out[i] != out[i - 1];    // differential decoding (out[0] stays)
    n_bits[ch] = static_cast<uint32_t>(nm);
    blk[ch] = 1;
}

// The station decoder of rds_station.hpp (fmrx_rds_station_feed_rrc's arithmetic), ONE LANE PER CHANNEL, on the in-phase
// matched-filter row.  The row arrives a batch ahead through registers into LDS, as in rdsb_pll_lanes_kernel; the per-phase
// energies live in LDS for the call (they are indexed by the sample's phase); the decoder's scalars stay in registers.  Station
// records (text as it arrives, the scalars at the end) and group records go out with ordinary vector stores.
// tab: the burst-correction table in global memory (one cached load per failed block; null with correction off); ext: the
// extension records (null = none kept).  A bank without station options passes both null and does what it did before them.
// Dynamic LDS: (kStB + sps) * 64 doubles, [sample][lane] then [phase][lane].  Rows are 16-byte aligned (even pitches).
__global__ __launch_bounds__(64) void rdsb_station_kernel(const double *__restrict__ y, long ypitch, long n, int n_ch, rdsst::Dec *__restrict__ dec,
                                                          double *__restrict__ energy, fmrx_rds_station *__restrict__ st,
                                                          fmrx_rds_group *__restrict__ grp, int max_g, uint32_t *__restrict__ n_g,
                                                          const uint32_t *__restrict__ tab, fmrx_rds_station_ext *__restrict__ ext)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const long ch = static_cast<long>(blockIdx.x) * 64 + lane;
    if (ch >= n_ch) return;
    double *lin = lds + lane, *E = lds + kStB * 64 + lane;
    rdsst::Dec d = dec[ch];
    const int sps = d.sps;
    double *er = energy + ch * rdsst::kMaxSps;
    for (int p = 0; p < sps; p++) E[p * 64] = er[p];
    rdsst::Out o{st + ch, grp + ch * max_g, static_cast<uint32_t>(max_g), 0u, tab, ext ? ext + ch : nullptr};
    const double *row = y + ch * ypitch;
    const d2 *row2 = reinterpret_cast<const d2 *>(row);
    const long nb = n / kStB;
    d2 pre[kStB / 2];
    if (nb > 0) {
#pragma unroll
        for (int g = 0; g < kStB / 2; g++) pre[g] = row2[g];
    }
    for (long b = 0; b < nb; b++) {
#pragma unroll
        for (int g = 0; g < kStB / 2; g++) {
            lin[(2 * g) * 64] = pre[g].x;
            lin[(2 * g + 1) * 64] = pre[g].y;
        }
        if (b + 1 < nb) {
#pragma unroll
            for (int g = 0; g < kStB / 2; g++) pre[g] = row2[(b + 1) * (kStB / 2) + g];
        }
#pragma unroll 1
        for (int j = 0; j < kStB; j++) rdsst::feed_sample(d, E, 64, lin[j * 64], o);
    }
    for (long k = nb * kStB; k < n; k++) rdsst::feed_sample(d, E, 64, row[k], o);
    rdsst::finish(d, st + ch);
    if (ext) rdsst::finish_ext(d, ext + ch);
    dec[ch] = d;
    for (int p = 0; p < sps; p++) er[p] = E[p * 64];
    n_g[ch] = o.n_g;
}

// carried state: per channel, every history <- the last samples of its row's block (blocks are at least as long as each
// history, create() checks: source and destination never overlap)
__global__ __launch_bounds__(256) void rdsb_tail_kernel(double *__restrict__ x, long xpitch, int hx, double *__restrict__ ch, long cpitch, int hc,
                                                        double *__restrict__ mi, double *__restrict__ mq, long mpitch, int hm, double *__restrict__ ri,
                                                        double *__restrict__ rq, long rpitch, int hr, long n, long n_out)
{
    const long c = blockIdx.x;
    double *xr = x + c * xpitch, *cr = ch + c * cpitch, *mir = mi + c * mpitch, *mqr = mq + c * mpitch, *rir = ri + c * rpitch, *rqr = rq + c * rpitch;
    for (int i = threadIdx.x; i < hx; i += blockDim.x) xr[i] = xr[n + i];
    for (int i = threadIdx.x; i < hc; i += blockDim.x) cr[i] = cr[n + i];
    for (int i = threadIdx.x; i < hm; i += blockDim.x) {
        mir[i] = mir[n + i];
        mqr[i] = mqr[n + i];
    }
    for (int i = threadIdx.x; i < hr; i += blockDim.x) {
        rir[i] = rir[n_out + i];
        rqr[i] = rqr[n_out + i];
    }
}

long pitch_of(long n) { return (n + 8 + 3) / 4 * 4; }   // kR - 2 readable samples past the end, 32-byte rows

}  // namespace

// ---- the chain (rds_chain.hpp) ---------------------------------------------------------------------------------------------

int Chain::plan(const char *who, const fmrx_rds_params *pp, int n_ch, size_t max_block)
{
    if (pp->taps < 3 || pp->taps > 65535 || pp->upsamp < 1 || pp->decim < 1 || pp->sps < 1 || pp->rrc_taps < 2 || pp->if_Fs <= 0)
        return fail(FMRX_EINVAL, "%s: bad parameters", who);
    p = *pp;
    n_channels = n_ch;
    block = static_cast<long>(max_block);
    delay = (p.taps - 1) / 2;
    Hx = p.taps - 1;
    Hm = (101 * p.upsamp - 1) / p.upsamp;
    Hc = std::max(p.taps - 1, delay + 1);
    Hr = p.rrc_taps - 1;
    const long n = block, no = static_cast<long>(n_out(max_block));
    xpitch = pitch_of(Hx + n);
    cpitch = pitch_of(Hc + n);
    apitch = pitch_of(n);
    npitch = pitch_of(n + 1);
    mpitch = pitch_of(Hm + n);
    rpitch = pitch_of(Hr + no);
    ypitch = pitch_of(no);
    return FMRX_OK;
}

int Chain::check_block(const char *who, size_t n) const
{
    if (n < static_cast<size_t>(std::max(std::max(Hx, Hc), Hm)) || n_out(n) < static_cast<size_t>(Hr))
        return fail(FMRX_EINVAL, "%s: block of %zu samples is shorter than a filter history (%d / %d / %d input samples, %d resampled)", who, n,
                    Hx, Hc, Hm, Hr);
    return FMRX_OK;
}

int Chain::create(int dev)
{
    device = dev;
    const int rs_taps = 101 * p.upsamp;
    std::vector<double> h(std::max(rs_taps, p.taps));
    auto up = [&](DevBuf<double> &d, int cnt) -> int {
        FMRX_TRY(d.alloc(cnt));
        FMRX_HIP(hipMemcpy(d.p, h.data(), cnt * sizeof(double), hipMemcpyHostToDevice));
        return FMRX_OK;
    };
    design_bpf64(p.taps, p.if_Fs, 54e3, 60e3, h.data());                                // fmMonoBlock.py:138
    FMRX_TRY(up(h_ch, p.taps));
    design_bpf64(p.taps, p.if_Fs, 113.5e3, 114.5e3, h.data());                          // :139
    FMRX_TRY(up(h_car, p.taps));
    design_lpf64(rs_taps, static_cast<double>(p.if_Fs) * p.upsamp, 3e3, h.data());      // :140
    FMRX_TRY(up(h_rs, rs_taps));
    design_rrc64(2375.0 * p.sps, p.rrc_taps, h.data());                                 // :141
    FMRX_TRY(up(h_rrc, p.rrc_taps));
    const size_t N = static_cast<size_t>(n_channels);
    auto rows = [&](DevBuf<double> &d, long pitch) -> int {
        FMRX_TRY(d.alloc(static_cast<size_t>(pitch) * N));
        FMRX_HIP(hipMemset(d.p, 0, d.bytes()));
        return FMRX_OK;
    };
    FMRX_TRY(rows(x, xpitch));
    FMRX_TRY(rows(ch, cpitch));
    FMRX_TRY(rows(car, apitch));
    FMRX_TRY(rows(arg, apitch));
    FMRX_TRY(rows(nco_i, npitch));
    FMRX_TRY(rows(nco_q, npitch));
    FMRX_TRY(rows(mi, mpitch));
    FMRX_TRY(rows(mq, mpitch));
    FMRX_TRY(rows(ri, rpitch));
    FMRX_TRY(rows(rq, rpitch));
    FMRX_TRY(rows(yi, ypitch));
    FMRX_TRY(rows(yq, ypitch));
    return state.alloc(8 * N);
}

int Chain::reset(int lo, int hi)
{
    FMRX_HIP(hipSetDevice(device));
    FMRX_HIP(hipDeviceSynchronize());
    const size_t cnt = static_cast<size_t>(hi - lo);
    auto hist = [&](DevBuf<double> &d, long pitch, int h) -> int {
        FMRX_HIP(hipMemset2D(d.p + lo * pitch, pitch * sizeof(double), 0, h * sizeof(double), cnt));
        return FMRX_OK;
    };
    FMRX_TRY(hist(x, xpitch, Hx));
    FMRX_TRY(hist(ch, cpitch, Hc));
    FMRX_TRY(hist(mi, mpitch, Hm));
    FMRX_TRY(hist(mq, mpitch, Hm));
    FMRX_TRY(hist(ri, rpitch, Hr));
    FMRX_TRY(hist(rq, rpitch, Hr));
    const double start[8] = {0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0};   // fmMonoBlock.py:186
    std::vector<double> init(8 * cnt);
    for (size_t c = 0; c < cnt; c++) std::copy(start, start + 8, init.begin() + 8 * c);
    FMRX_HIP(hipMemcpy(state.p + 8 * lo, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice));
    FMRX_HIP(hipDeviceSynchronize());
    return FMRX_OK;
}

int Chain::run(const float *d_demod, size_t pitch, size_t n_in, hipStream_t s, const CdrRows *cdr)
{
    const long n = static_cast<long>(n_in), no = static_cast<long>(n_out(n_in));
    const unsigned N = static_cast<unsigned>(n_channels), lanes = (N + 63) / 64;
    auto tiles = [](long cnt, long per) { return static_cast<unsigned>((cnt + per - 1) / per); };
    double *xb = x.p + Hx, *chb = ch.p + Hc, *mib = mi.p + Hm, *mqb = mq.p + Hm, *rib = ri.p + Hr, *rqb = rq.p + Hr;
    const double phase_adjust = 3 * kPi / 8;
    hipLaunchKernelGGL(rdsb_cvt_kernel, dim3(N, tiles(n, 256)), dim3(256), 0, s, d_demod, static_cast<long>(pitch), n, xb, xpitch);
    FMRX_LAUNCH_CHECK("rdsb_cvt_kernel");
    hipLaunchKernelGGL(rdsb_fir_kernel<false>, dim3(N, tiles(n, 256 * kR)), dim3(256), 0, s, xb, xb, xpitch, n, h_ch.p, p.taps, chb, chb, cpitch);
    FMRX_LAUNCH_CHECK("rdsb_fir_kernel<false>");
    hipLaunchKernelGGL(rdsb_fir_kernel<true>, dim3(N, tiles(n, 256 * kR)), dim3(256), 0, s, chb, chb, cpitch, n, h_car.p, p.taps, car.p, car.p,
                       apitch);
    FMRX_LAUNCH_CHECK("rdsb_fir_kernel<true>");
    hipLaunchKernelGGL(rdsb_pll_lanes_kernel, dim3(lanes), dim3(64), 0, s, car.p, apitch, n, n_channels, arg.p, state.p, nco_i.p, nco_q.p, npitch,
                       114e3, static_cast<double>(p.if_Fs), 0.002, 0.5, phase_adjust);
    FMRX_LAUNCH_CHECK("rdsb_pll_lanes_kernel");
    hipLaunchKernelGGL(rdsb_mix_kernel, dim3(N, tiles(n, 256)), dim3(256), 0, s, arg.p, apitch, n, chb, cpitch, delay, 0.5, phase_adjust, nco_i.p,
                       nco_q.p, npitch, mib, mqb, mpitch);
    FMRX_LAUNCH_CHECK("rdsb_mix_kernel");
    hipLaunchKernelGGL(rdsb_resample_kernel, dim3(N, tiles(no, 256)), dim3(256), 0, s, mib, mqb, mpitch, no, h_rs.p, 101 * p.upsamp, p.decim,
                       p.upsamp, rib, rqb, rpitch);
    FMRX_LAUNCH_CHECK("rdsb_resample_kernel");
    hipLaunchKernelGGL(rdsb_fir_kernel<false>, dim3(N, tiles(no, 256 * kR), 2), dim3(256), 0, s, rib, rqb, rpitch, no, h_rrc.p, p.rrc_taps, yi.p,
                       yq.p, ypitch);
    FMRX_LAUNCH_CHECK("rdsb_fir_kernel<false>");
    // fmMonoBlock.py:276-280 (fmrx_rds_process): the CDR state is re-made every block
    if (cdr) {
        hipLaunchKernelGGL(rdsb_cdr_kernel, dim3(lanes), dim3(64), 0, s, yi.p, ypitch, no, n_channels, p.sps, 0.0, 0.0, 158L, 0L, cdr->blk,
                           cdr->bits, cdr->max_bits, cdr->n_bits);
        FMRX_LAUNCH_CHECK("rdsb_cdr_kernel");
    }
    hipLaunchKernelGGL(rdsb_tail_kernel, dim3(N), dim3(256), 0, s, x.p, xpitch, Hx, ch.p, cpitch, Hc, mi.p, mq.p, mpitch, Hm, ri.p, rq.p, rpitch, Hr,
                       n, no);
    FMRX_LAUNCH_CHECK("rdsb_tail_kernel");
    last_n = n_in;
    last_out = static_cast<size_t>(no);
    return FMRX_OK;
}

int Chain::tap(const char *who, int channel, int which, double *out, size_t *n)
{
    const long c = channel;
    const double *src = nullptr;
    size_t cnt = 0;
    switch (which) {
    case FMRX_RDS_TAP_CHANNEL: src = ch.p + c * cpitch + Hc; cnt = last_n; break;   // after the tail copy the block region is intact
    case FMRX_RDS_TAP_CARRIER: src = car.p + c * apitch; cnt = last_n; break;
    case FMRX_RDS_TAP_PLL_I: src = nco_i.p + c * npitch; cnt = last_n ? last_n + 1 : 0; break;
    case FMRX_RDS_TAP_PLL_Q: src = nco_q.p + c * npitch; cnt = last_n ? last_n + 1 : 0; break;
    case FMRX_RDS_TAP_RESAMPLED_I: src = ri.p + c * rpitch + Hr; cnt = last_out; break;
    case FMRX_RDS_TAP_RRC_I: src = yi.p + c * ypitch; cnt = last_out; break;
    case FMRX_RDS_TAP_RRC_Q: src = yq.p + c * ypitch; cnt = last_out; break;
    case FMRX_RDS_TAP_PLL_STATE: src = state.p + 8 * c; cnt = 7; break;
    default: return fail(FMRX_EINVAL, "%s: unknown tap %d", who, which);
    }
    *n = cnt;
    if (!out || cnt == 0) return FMRX_OK;
    FMRX_HIP(hipSetDevice(device));
    FMRX_HIP(hipDeviceSynchronize());
    FMRX_HIP(hipMemcpy(out, src, cnt * sizeof(double), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

// ---- the bank: the chain of N channels with a fixed block, bits recovered on the device, stations ---------------------------

struct fmrx_rds_bank {
    Chain c;
    long n_out = 0, max_bits = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    DevBuf<float> in;
    DevBuf<int> blk;
    DevBuf<uint8_t> bits;
    DevBuf<uint32_t> n_bits;
    std::vector<uint8_t> h_bits;
    std::vector<uint32_t> h_n_bits;
    std::vector<std::vector<uint8_t>> decoded;   // per channel: the bits frame synchronisation keeps (fmrx_rds::decoded)
    bool pending = false;                          // a process_dev whose bits have not been collected
    bool fresh = true;                             // no call since create / reset(-1): stations may be switched
    bool stations = false;                         // rdsb_station_kernel runs in process_dev
    long max_g = 0;                                // group records per channel and call
    DevBuf<rdsst::Dec> dec;                        // [N] station decoders' scalars
    DevBuf<double> energy;                         // [N][kMaxSps] their per-phase energies
    DevBuf<fmrx_rds_station> st;                   // [N] station records
    DevBuf<fmrx_rds_group> grp;                    // [N][max_g] the last call's groups
    DevBuf<uint32_t> n_g;                          // [N] how many
    std::vector<uint32_t> h_n_g;
    int max_burst = 0;                             // station options (fmrx_rds_bank_set_station_options)
    DevBuf<uint32_t> tab;                          // [1024] the burst-correction table, where max_burst > 0 was asked for
    DevBuf<fmrx_rds_station_ext> ext;              // [N] extension records, where asked for
};

namespace {

// back to the start-of-stream state, channels [lo, hi)
int bank_reset(fmrx_rds_bank *b, int lo, int hi)
{
    FMRX_TRY(b->c.reset(lo, hi));
    const size_t cnt = static_cast<size_t>(hi - lo);
    FMRX_HIP(hipMemset(b->blk.p + lo, 0, cnt * sizeof(int)));
    for (int c = lo; c < hi; c++) b->decoded[c].clear();
    if (b->dec.p) {                                // the station decoders, as fmrx_rds_station_create leaves them
        std::vector<rdsst::Dec> d(cnt);
        std::vector<fmrx_rds_station> r(cnt);
        for (size_t c = 0; c < cnt; c++) {
            rdsst::init(d[c], b->c.p.sps, b->max_burst);
            rdsst::clear_record(&r[c]);
        }
        if (b->ext.p) {
            std::vector<fmrx_rds_station_ext> x(cnt);
            for (size_t c = 0; c < cnt; c++) rdsst::clear_ext(&x[c], b->max_burst);
            FMRX_HIP(hipMemcpy(b->ext.p + lo, x.data(), cnt * sizeof(fmrx_rds_station_ext), hipMemcpyHostToDevice));
        }
        FMRX_HIP(hipMemcpy(b->dec.p + lo, d.data(), cnt * sizeof(rdsst::Dec), hipMemcpyHostToDevice));
        FMRX_HIP(hipMemcpy(b->st.p + lo, r.data(), cnt * sizeof(fmrx_rds_station), hipMemcpyHostToDevice));
        FMRX_HIP(hipMemset(b->energy.p + lo * rdsst::kMaxSps, 0, cnt * rdsst::kMaxSps * sizeof(double)));
        FMRX_HIP(hipMemset(b->n_g.p + lo, 0, cnt * sizeof(uint32_t)));
    }
    FMRX_HIP(hipDeviceSynchronize());
    return FMRX_OK;
}

}  // namespace

extern "C" {

int fmrx_rds_bank_create(fmrx_rds_bank **out, const fmrx_rds_params *p, int n_channels, size_t block, int device)
{
    if (!out || !p) return fail(FMRX_EINVAL, "rds_bank_create: null argument");
    fmrx_rds_bank *b = new fmrx_rds_bank;
    auto checks = [&]() -> int {                    // before any device call
        FMRX_TRY(b->c.plan("rds_bank_create", p, n_channels, block));
        if (n_channels < 1) return fail(FMRX_EINVAL, "rds_bank_create: n_channels must be >= 1");
        if (block == 0 || block > (1u << 30) || (block * p->upsamp) % p->decim)
            return fail(FMRX_EINVAL, "rds_bank_create: block of %zu samples: block*upsamp must be a multiple of decim %d", block, p->decim);
        FMRX_TRY(b->c.check_block("rds_bank_create", block));
        return require_device();
    };
    int rc = checks();
    if (rc != FMRX_OK) {
        delete b;
        return rc;
    }
    auto body = [&]() -> int {
        FMRX_HIP(hipSetDevice(device));
        b->n_out = static_cast<long>(b->c.n_out(block));
        b->max_bits = b->n_out / p->sps + 4;
        b->max_g = p->sps >= 2 ? static_cast<long>(rdsst::max_groups_for_samples(static_cast<uint64_t>(b->n_out), p->sps)) : 0;
        FMRX_TRY(b->c.create(device));
        const size_t N = static_cast<size_t>(n_channels);
        FMRX_TRY(b->blk.alloc(N));
        FMRX_TRY(b->bits.alloc(static_cast<size_t>(b->max_bits) * N));
        FMRX_TRY(b->n_bits.alloc(N));
        b->h_bits.resize(static_cast<size_t>(b->max_bits) * N);
        b->h_n_bits.resize(N);
        b->decoded.resize(N);
        FMRX_HIP(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking));
        FMRX_HIP(hipEventCreateWithFlags(&b->done, hipEventDisableTiming));
        return bank_reset(b, 0, n_channels);
    };
    rc = body();
    if (rc != FMRX_OK) {
        fmrx_rds_bank_destroy(b);
        return rc;
    }
    *out = b;
    return FMRX_OK;
}

int fmrx_rds_bank_destroy(fmrx_rds_bank *b)
{
    if (!b) return FMRX_OK;
    (void)hipSetDevice(b->c.device);
    (void)hipDeviceSynchronize();
    if (b->stream) (void)hipStreamDestroy(b->stream);
    if (b->done) (void)hipEventDestroy(b->done);
    delete b;
    return FMRX_OK;
}

int fmrx_rds_bank_reset(fmrx_rds_bank *b, int channel)
{
    if (!b) return fail(FMRX_EINVAL, "rds_bank_reset: null handle");
    if (channel >= b->c.n_channels) return fail(FMRX_EINVAL, "rds_bank_reset: channel %d of %d", channel, b->c.n_channels);
    if (b->pending) return fail(FMRX_EINVAL, "rds_bank_reset: the last process_dev has not been collected");
    if (channel < 0) {
        FMRX_TRY(bank_reset(b, 0, b->c.n_channels));
        b->fresh = true;
        return FMRX_OK;
    }
    return bank_reset(b, channel, channel + 1);
}

int fmrx_rds_bank_set_stations(fmrx_rds_bank *b, int on)
{
    if (!b) return fail(FMRX_EINVAL, "rds_bank_set_stations: null handle");
    if (!b->fresh) return fail(FMRX_EINVAL, "rds_bank_set_stations: only before the first call or right after fmrx_rds_bank_reset(b, -1)");
    if (on && (b->c.p.sps < 2 || b->c.p.sps > rdsst::kMaxSps))
        return fail(FMRX_EINVAL, "rds_bank_set_stations: the station decoder takes 2..%d samples per chip, not %d", rdsst::kMaxSps, b->c.p.sps);
    if (on && !b->dec.p) {
        FMRX_HIP(hipSetDevice(b->c.device));
        const size_t N = static_cast<size_t>(b->c.n_channels);
        FMRX_TRY(b->dec.alloc(N));
        FMRX_TRY(b->energy.alloc(N * rdsst::kMaxSps));
        FMRX_TRY(b->st.alloc(N));
        FMRX_TRY(b->grp.alloc(N * static_cast<size_t>(b->max_g)));
        FMRX_HIP(hipMemset(b->grp.p, 0, b->grp.bytes()));
        FMRX_TRY(b->n_g.alloc(N));
        b->h_n_g.resize(N);
        b->stations = true;                         // (bank_reset initialises what is allocated)
        const int rc = bank_reset(b, 0, b->c.n_channels);
        if (rc != FMRX_OK) {
            b->stations = false;
            b->dec.release();
            return rc;
        }
    }
    b->stations = on != 0;
    return FMRX_OK;
}

int fmrx_rds_bank_set_station_options(fmrx_rds_bank *b, int max_burst, int ext)
{
    if (!b) return fail(FMRX_EINVAL, "rds_bank_set_station_options: null handle");
    if (!b->stations) return fail(FMRX_EINVAL, "rds_bank_set_station_options: stations are off (fmrx_rds_bank_set_stations)");
    if (!b->fresh)
        return fail(FMRX_EINVAL, "rds_bank_set_station_options: only before the first call or right after fmrx_rds_bank_reset(b, -1)");
    if (max_burst < 0 || max_burst > rdsst::kMaxBurst)
        return fail(FMRX_EINVAL, "rds_bank_set_station_options: max_burst %d not in 0..%d", max_burst, rdsst::kMaxBurst);
    FMRX_HIP(hipSetDevice(b->c.device));
    if (max_burst > 0 && !b->tab.p) {
        std::vector<uint32_t> t(rdsst::kBurstTableSize);
        if (rdsst::build_burst_table(t.data()) != 367) return fail(FMRX_EINVAL, "rds_bank_set_station_options: correction table");
        FMRX_TRY(b->tab.alloc(t.size()));
        FMRX_HIP(hipMemcpy(b->tab.p, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (ext && !b->ext.p) FMRX_TRY(b->ext.alloc(static_cast<size_t>(b->c.n_channels)));
    if (!ext) b->ext.release();
    b->max_burst = max_burst;
    return bank_reset(b, 0, b->c.n_channels);       // the decoders start over with the option
}

int fmrx_rds_bank_stations_ext(fmrx_rds_bank *b, fmrx_rds_station_ext *ext)
{
    if (!b || !ext) return fail(FMRX_EINVAL, "rds_bank_stations_ext: null argument");
    if (!b->stations || !b->ext.p)
        return fail(FMRX_EINVAL, "rds_bank_stations_ext: the extension records are off (fmrx_rds_bank_set_station_options)");
    FMRX_HIP(hipSetDevice(b->c.device));
    b->pending = false;
    hipStream_t s = b->stream;
    FMRX_HIP(hipStreamWaitEvent(s, b->done, 0));
    FMRX_HIP(hipMemcpyAsync(ext, b->ext.p, static_cast<size_t>(b->c.n_channels) * sizeof(fmrx_rds_station_ext), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipStreamSynchronize(s));
    return FMRX_OK;
}

size_t fmrx_rds_bank_max_groups(const fmrx_rds_bank *b) { return b ? static_cast<size_t>(b->max_g) : 0; }

int fmrx_rds_bank_stations(fmrx_rds_bank *b, fmrx_rds_station *st, fmrx_rds_group *g, size_t *n_g)
{
    if (!b || !st) return fail(FMRX_EINVAL, "rds_bank_stations: null argument");
    if ((g == nullptr) != (n_g == nullptr)) return fail(FMRX_EINVAL, "rds_bank_stations: g and n_g go together");
    if (!b->stations) return fail(FMRX_EINVAL, "rds_bank_stations: stations are off (fmrx_rds_bank_set_stations)");
    FMRX_HIP(hipSetDevice(b->c.device));
    b->pending = false;
    hipStream_t s = b->stream;
    const size_t N = static_cast<size_t>(b->c.n_channels);
    FMRX_HIP(hipStreamWaitEvent(s, b->done, 0));
    FMRX_HIP(hipMemcpyAsync(st, b->st.p, N * sizeof(fmrx_rds_station), hipMemcpyDeviceToHost, s));
    if (g) {
        FMRX_HIP(hipMemcpyAsync(g, b->grp.p, N * static_cast<size_t>(b->max_g) * sizeof(fmrx_rds_group), hipMemcpyDeviceToHost, s));
        FMRX_HIP(hipMemcpyAsync(b->h_n_g.data(), b->n_g.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    }
    FMRX_HIP(hipStreamSynchronize(s));
    if (n_g)
        for (size_t c = 0; c < N; c++) n_g[c] = b->h_n_g[c];
    return FMRX_OK;
}

size_t fmrx_rds_bank_n_out(const fmrx_rds_bank *b) { return b ? static_cast<size_t>(b->n_out) : 0; }
size_t fmrx_rds_bank_max_bits(const fmrx_rds_bank *b) { return b ? static_cast<size_t>(b->max_bits) : 0; }

int fmrx_rds_bank_process_dev(fmrx_rds_bank *b, const float *d_demod, size_t pitch, void *stream)
{
    if (!b || !d_demod) return fail(FMRX_EINVAL, "rds_bank_process_dev: null argument");
    if (pitch < static_cast<size_t>(b->c.block))
        return fail(FMRX_EINVAL, "rds_bank_process_dev: pitch %zu floats is shorter than the block (%ld)", pitch, b->c.block);
    // every frame-sync report depends on the bits of every earlier call: they are never dropped
    if (b->pending) return fail(FMRX_EINVAL, "rds_bank_process_dev: the previous call has not been collected (fmrx_rds_bank_collect)");
    FMRX_HIP(hipSetDevice(b->c.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const CdrRows cdr{b->blk.p, b->bits.p, b->max_bits, b->n_bits.p};
    FMRX_TRY(b->c.run(d_demod, pitch, static_cast<size_t>(b->c.block), s, &cdr));
    if (b->stations) {
        const unsigned lanes = (static_cast<unsigned>(b->c.n_channels) + 63) / 64;
        hipLaunchKernelGGL(rdsb_station_kernel, dim3(lanes), dim3(64), (kStB + b->c.p.sps) * 64 * sizeof(double), s, b->c.yi.p, b->c.ypitch, b->n_out,
                           b->c.n_channels, b->dec.p, b->energy.p, b->st.p, b->grp.p, static_cast<int>(b->max_g), b->n_g.p,
                           b->max_burst > 0 ? b->tab.p : nullptr, b->ext.p);
        FMRX_LAUNCH_CHECK("rdsb_station_kernel");
    }
    FMRX_HIP(hipEventRecord(b->done, s));
    b->pending = true;
    b->fresh = false;
    return FMRX_OK;
}

int fmrx_rds_bank_collect(fmrx_rds_bank *b, double *rrc_i, double *rrc_q, uint8_t *bits, size_t *n_bits, char *offset_type)
{
    if (!b) return fail(FMRX_EINVAL, "rds_bank_collect: null handle");
    if (!b->pending) return fail(FMRX_EINVAL, "rds_bank_collect: no call to collect");
    FMRX_HIP(hipSetDevice(b->c.device));
    b->pending = false;
    hipStream_t s = b->stream;
    const size_t N = static_cast<size_t>(b->c.n_channels), no = static_cast<size_t>(b->n_out), mb = static_cast<size_t>(b->max_bits);
    FMRX_HIP(hipStreamWaitEvent(s, b->done, 0));
    FMRX_HIP(hipMemcpyAsync(b->h_bits.data(), b->bits.p, N * mb, hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipMemcpyAsync(b->h_n_bits.data(), b->n_bits.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    const size_t yp = static_cast<size_t>(b->c.ypitch) * sizeof(double);
    if (rrc_i) FMRX_HIP(hipMemcpy2DAsync(rrc_i, no * sizeof(double), b->c.yi.p, yp, no * sizeof(double), N, hipMemcpyDeviceToHost, s));
    if (rrc_q) FMRX_HIP(hipMemcpy2DAsync(rrc_q, no * sizeof(double), b->c.yq.p, yp, no * sizeof(double), N, hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipStreamSynchronize(s));
    // fmMonoBlock.py:283-297, per channel: frame synchronisation over the bits kept so far
    for (size_t c = 0; c < N; c++) {
        const size_t nb = b->h_n_bits[c];
        const uint8_t *d = b->h_bits.data() + c * mb;
        if (bits) std::memcpy(bits + c * mb, d, nb);
        if (n_bits) n_bits[c] = nb;
        const char *off = frame_sync_append(b->decoded[c], d, nb);
        if (offset_type) std::strcpy(offset_type + 8 * c, off);
    }
    return FMRX_OK;
}

int fmrx_rds_bank_process(fmrx_rds_bank *b, const float *demod, double *rrc_i, double *rrc_q, uint8_t *bits, size_t *n_bits, char *offset_type)
{
    if (!b || !demod) return fail(FMRX_EINVAL, "rds_bank_process: null argument");
    if (b->pending) return fail(FMRX_EINVAL, "rds_bank_process: the previous call has not been collected (fmrx_rds_bank_collect)");
    FMRX_HIP(hipSetDevice(b->c.device));
    const size_t n = static_cast<size_t>(b->c.block), N = static_cast<size_t>(b->c.n_channels);
    FMRX_TRY(b->in.ensure(n * N));
    FMRX_HIP(hipMemcpyAsync(b->in.p, demod, n * N * sizeof(float), hipMemcpyHostToDevice, b->stream));
    FMRX_TRY(fmrx_rds_bank_process_dev(b, b->in.p, n, b->stream));
    return fmrx_rds_bank_collect(b, rrc_i, rrc_q, bits, n_bits, offset_type);
}

int fmrx_rds_bank_read_tap(fmrx_rds_bank *b, int channel, int which, double *out, size_t *n)
{
    if (!b || !n) return fail(FMRX_EINVAL, "rds_bank_read_tap: null argument");
    if (channel < 0 || channel >= b->c.n_channels) return fail(FMRX_EINVAL, "rds_bank_read_tap: channel %d of %d", channel, b->c.n_channels);
    return b->c.tap("rds_bank_read_tap", channel, which, out, n);
}

}  // extern "C"
