// meters.hip -- the signal meters' handle, host arithmetic and C ABI (include/fmrx.h: fmrx_meters_*): per channel of a receiver
// bank, the RF level / CNR / clipping of its input slot and the offset, deviation, pilot and RDS levels of its discriminator
// row.  Kernels: kernels_meters.hip; definition: tests/_meters_model.py.
//
// The handle keeps no signal state: the tone table on the device, the two result arrays a call writes ([n_channels][5]
// 64-bit integers, zeroed on the stream and added to by the RF pass; [n_channels][8] doubles written by the MPX pass), their
// pinned host copies, and meter_stage.hpp's handle base: the event the last call recorded behind the copies.
#include "meter_stage.hpp"

#include <cmath>

using namespace fmrx;

struct fmrx_meters : meter_stage::Handle {
    int n_channels = 0, max_blocks = 1;
    double if_Fs = 0.0;
    DevBuf<double> d_table, d_mpx;
    DevBuf<unsigned long long> d_rf;
    HostBuf<unsigned long long> h_rf;
    HostBuf<double> h_mpx;
    size_t n_iq = 0, n_if = 0;            // of the last call; 0 = that group was not measured
    DevBuf<uint8_t> d_iq;                 // fmrx_meters_process only
    DevBuf<float> d_demod;
};

namespace {

constexpr double kProbesHz[kMetersProbes] = {17000.0, 21000.0, 19000.0, 55812.5, 58187.5};
constexpr int kNoiseLo = 0, kNoiseHi = 1, kPilot = 2, kRdsLo = 3, kRdsHi = 4;
constexpr double kMinIfFs = 120000.0, kTwoPi = 2.0 * 3.14159265358979323846;
constexpr int kMpxBlocksPerCu = 3;   // what the MPX kernel's registers admit per CU (3 waves per SIMD)

void meters_table(double if_Fs, double *re, double *im)
{
    for (int p = 0; p < kMetersProbes; p++)
        for (int k = 0; k < kMetersSegment; k++) {
            const double w = 0.5 - 0.5 * std::cos(kTwoPi * (k + 0.5) / kMetersSegment);
            const double th = kTwoPi * kProbesHz[p] * k / if_Fs;
            re[p * kMetersSegment + k] = w * std::cos(th);
            im[p * kMetersSegment + k] = -(w * std::sin(th));
        }
}

double mean(double a, double n) { return n > 0.0 ? a / n : 0.0; }

}  // namespace

fmrx::MetersMpx fmrx::meters_mpx(const fmrx_meters *m) { return MetersMpx{m->d_mpx.p, m->n_if, m->n_channels, m->device, m->ran}; }

extern "C" {

int fmrx_meters_probes(double hz[8], int *n)
{
    if (!hz || !n) return fail(FMRX_EINVAL, "meters_probes: null argument");
    for (int p = 0; p < 8; p++) hz[p] = p < kMetersProbes ? kProbesHz[p] : 0.0;
    *n = kMetersProbes;
    return FMRX_OK;
}

int fmrx_meters_table(double if_Fs, double *re, double *im)
{
    if (!re || !im) return fail(FMRX_EINVAL, "meters_table: null argument");
    if (!(if_Fs >= kMinIfFs) || !std::isfinite(if_Fs)) return fail(FMRX_EINVAL, "meters_table: if_Fs %g (at least %g: the top probe stays below Nyquist)", if_Fs, kMinIfFs);
    meters_table(if_Fs, re, im);
    return FMRX_OK;
}

int fmrx_meters_derive(double if_Fs, const fmrx_meter *m, fmrx_meter_levels *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "meters_derive: null argument");
    const double n_iq = static_cast<double>(m->n_iq), n_if = static_cast<double>(m->n_if), M = static_cast<double>(m->segments);
    const double M2 = mean(static_cast<double>(m->m2), n_iq), M4 = mean(static_cast<double>(m->m4), n_iq);
    const double S = std::sqrt(std::fmax(0.0, 2.0 * M2 * M2 - M4));
    const double hz = if_Fs / kTwoPi;
    const double noise = (m->probe[kNoiseLo] + m->probe[kNoiseHi]) / 2.0;
    out->level_dbfs = db(M2, 16384.0);
    out->cnr_db = db(S, M2 - S);
    out->clip_fraction = mean(static_cast<double>(m->clipped), 2.0 * n_iq);
    out->dc_i = mean(static_cast<double>(m->sum_i), n_iq);
    out->dc_q = mean(static_cast<double>(m->sum_q), n_iq);
    out->freq_offset_hz = mean(m->sum_x, n_if) * hz;
    out->peak_dev_hz = m->max_abs * hz;
    out->mpx_rms_hz = std::sqrt(mean(m->sum_x2, n_if)) * hz;
    out->pilot_dev_hz = (4.0 * std::sqrt(mean(m->probe[kPilot], M)) / kMetersSegment) * hz;
    out->pilot_db = db(m->probe[kPilot], noise);
    out->rds_db = db((m->probe[kRdsLo] + m->probe[kRdsHi]) / 2.0, 9.0 * noise);
    return FMRX_OK;
}

int fmrx_meters_create(fmrx_meters **out, double if_Fs, int n_channels, int device)
{
    if (!out) return fail(FMRX_EINVAL, "meters_create: null argument");
    if (!(if_Fs >= kMinIfFs) || !std::isfinite(if_Fs))
        return fail(FMRX_EINVAL, "meters_create: if_Fs %g (at least %g: the top probe stays below Nyquist)", if_Fs, kMinIfFs);
    if (n_channels < 1) return fail(FMRX_EINVAL, "meters_create: n_channels must be >= 1");
    return meter_stage::make(out, device, [&](fmrx_meters *m) -> int {
        const size_t N = n_channels;
        m->n_channels = n_channels;
        m->if_Fs = if_Fs;
        int cus = 0;
        FMRX_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        m->max_blocks = kMpxBlocksPerCu * (cus > 0 ? cus : 1);
        std::vector<double> tab(2 * kMetersProbes * kMetersSegment);
        meters_table(if_Fs, tab.data(), tab.data() + kMetersProbes * kMetersSegment);
        FMRX_TRY(m->d_table.alloc(tab.size()));
        FMRX_HIP(hipMemcpy(m->d_table.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        FMRX_TRY(m->d_rf.alloc(N * kMetersRfFields));
        FMRX_TRY(m->d_mpx.alloc(N * kMetersMpxFields));
        FMRX_TRY(m->h_rf.alloc(m->d_rf.n));
        return m->h_mpx.alloc(m->d_mpx.n);
    });
}

int fmrx_meters_destroy(fmrx_meters *m) { return meter_stage::destroy(m); }

int fmrx_meters_process_dev(fmrx_meters *m, const uint8_t *d_iq_first, size_t iq_pitch_bytes, size_t n_iq_bytes, const float *d_demod_row0,
                            size_t demod_pitch, size_t n_if, void *stream)
{
    if (!m) return fail(FMRX_EINVAL, "meters_process_dev: null handle");
    if (d_iq_first) {
        if (n_iq_bytes == 0 || n_iq_bytes % 2 || n_iq_bytes > (size_t{1} << 34))
            return fail(FMRX_EINVAL, "meters_process_dev: %zu I/Q bytes: an even count, 2 .. 2^34", n_iq_bytes);
        if (m->n_channels > 1 && iq_pitch_bytes < n_iq_bytes)
            return fail(FMRX_EINVAL, "meters_process_dev: pitch of %zu bytes is shorter than a channel's %zu bytes", iq_pitch_bytes, n_iq_bytes);
    }
    if (d_demod_row0) {
        if (n_if < static_cast<size_t>(kMetersSegment))
            return fail(FMRX_EINVAL, "meters_process_dev: %zu IF samples: at least one segment of %d", n_if, kMetersSegment);
        if (reinterpret_cast<uintptr_t>(d_demod_row0) % sizeof(float)) return fail(FMRX_EINVAL, "meters_process_dev: d_demod_row0 must be 4-byte aligned");
        if (m->n_channels > 1 && demod_pitch < n_if)
            return fail(FMRX_EINVAL, "meters_process_dev: pitch of %zu floats is shorter than a row's %zu samples", demod_pitch, n_if);
    }
    FMRX_HIP(hipSetDevice(m->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    FMRX_HIP(hipMemsetAsync(m->d_rf.p, 0, m->d_rf.bytes(), s));
    if (d_iq_first) FMRX_TRY(meters_rf_launch(d_iq_first, iq_pitch_bytes, n_iq_bytes, m->n_channels, m->d_rf.p, s));
    if (d_demod_row0) {
        FMRX_TRY(meters_mpx_launch(d_demod_row0, demod_pitch, n_if, m->n_channels, m->d_table.p, m->d_mpx.p, m->max_blocks, s));
    } else {
        FMRX_HIP(hipMemsetAsync(m->d_mpx.p, 0, m->d_mpx.bytes(), s));
    }
    FMRX_HIP(hipMemcpyAsync(m->h_rf.p, m->d_rf.p, m->d_rf.bytes(), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipMemcpyAsync(m->h_mpx.p, m->d_mpx.p, m->d_mpx.bytes(), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipEventRecord(m->done, s));
    m->n_iq = d_iq_first ? n_iq_bytes / 2 : 0;
    m->n_if = d_demod_row0 ? n_if : 0;
    m->ran = true;
    return FMRX_OK;
}

int fmrx_meters_collect(fmrx_meters *m, fmrx_meter *out)
{
    FMRX_TRY(meter_stage::collected("meters_collect", m, out));
    for (size_t c = 0; c < static_cast<size_t>(m->n_channels); c++) {
        const unsigned long long *rf = m->h_rf.p + c * kMetersRfFields;
        const double *mpx = m->h_mpx.p + c * kMetersMpxFields;
        fmrx_meter &r = out[c];
        std::memset(&r, 0, sizeof r);
        r.n_iq = m->n_iq;
        r.sum_i = static_cast<int64_t>(rf[0]);
        r.sum_q = static_cast<int64_t>(rf[1]);
        r.m2 = rf[2];
        r.m4 = rf[3];
        r.clipped = rf[4];
        r.n_if = m->n_if;
        r.segments = m->n_if / kMetersSegment;
        r.sum_x = mpx[0];
        r.sum_x2 = mpx[1];
        r.max_abs = mpx[2];
        for (int p = 0; p < kMetersProbes; p++) r.probe[p] = mpx[3 + p];
    }
    return FMRX_OK;
}

int fmrx_meters_process(fmrx_meters *m, const uint8_t *iq, size_t iq_pitch_bytes, size_t n_iq_bytes, const float *demod, size_t demod_pitch,
                        size_t n_if, fmrx_meter *out)
{
    if (!m || !out) return fail(FMRX_EINVAL, "meters_process: null argument");
    FMRX_HIP(hipSetDevice(m->device));
    const size_t N = m->n_channels;
    if (N == 1) {
        iq_pitch_bytes = n_iq_bytes;
        demod_pitch = n_if;
    }
    if ((iq && iq_pitch_bytes < n_iq_bytes) || (demod && demod_pitch < n_if)) return fail(FMRX_EINVAL, "meters_process: a pitch shorter than its row");
    const size_t dp_iq = (n_iq_bytes + 15) / 16 * 16, dp_x = (n_if + 3) / 4 * 4;   // the device copies' pitches: rows 16-byte aligned
    if (iq && n_iq_bytes) {
        FMRX_TRY(m->d_iq.ensure(dp_iq * N));
        FMRX_HIP(hipMemcpy2D(m->d_iq.p, dp_iq, iq, iq_pitch_bytes, n_iq_bytes, N, hipMemcpyHostToDevice));
    }
    if (demod && n_if) {
        FMRX_TRY(m->d_demod.ensure(dp_x * N));
        FMRX_HIP(hipMemcpy2D(m->d_demod.p, dp_x * sizeof(float), demod, demod_pitch * sizeof(float), n_if * sizeof(float), N, hipMemcpyHostToDevice));
    }
    FMRX_TRY(fmrx_meters_process_dev(m, iq ? m->d_iq.p : nullptr, dp_iq, n_iq_bytes, demod ? m->d_demod.p : nullptr, dp_x, n_if, nullptr));
    return fmrx_meters_collect(m, out);
}

}  // extern "C"
