// rds.hip -- the RDS path: include/fmrx.h fmrx_rds_*.
//
// The reference has this path only as a Python / NumPy model in float64 (model/fmMonoBlock.py:238-296 on top of
// model/fmSupportLib.py; it never reached the C++, report p.8), so float64 is the arithmetic to match and the MI355X's
// full-rate FP64 vector ALUs run it.  Per block of discriminator output (fm_demod, what the front-end kernels produce):
//   rds_channel = band-pass 54-60 kHz (151 taps)                       fmMonoBlock.py:241
//   rds_allpass = delay by 75 samples                                  :245                 an index offset
//   rds_carrier = band-pass 113.5-114.5 kHz of rds_channel^2           :248-251
//   PLL at 114 kHz, ncoScale 0.5, phaseAdjust 3pi/8, bandwidth 0.002   :254                 serial
//   mixer I / Q = NCO * allpass * 2                                    :259, :270
//   rational resampler U/D (247/960 in mode 0), 101*U taps, 3 kHz      :262, :271           gain U, as the model
//   root-raised-cosine matched filter (101 taps)                       :266, :273
// and on the host, as in the model, clock and data recovery, Manchester and differential decoding, frame synchronisation
// (fmSupportLib.py:103-249, 30-100) on the 61 750 Hz output.
//
// The device part is the chain of rds_chain.hpp with ONE channel: the kernels, the row layout and the carried state of the RDS
// bank (rds_bank.hip), 8 launches per block, any block of up to max_block samples per call.  This file holds the handle around
// it (its stream, its input buffer, the host bit recovery with the block counter) and the host primitives of the public ABI.
#include "fmrx_internal.hpp"
#include "rds_chain.hpp"
#include "rds_common.hpp"

#pragma clang fp contract(off)

using namespace fmrx;
using namespace fmrx::rds;

struct fmrx_rds {
    Chain c;                         // one channel
    long block = 0;                  // blocks whose bits have been recovered: the CDR's block_count
    hipStream_t stream = nullptr;
    DevBuf<float> in;
    std::vector<uint8_t> decoded;    // the bits frame synchronisation keeps
};

extern "C" {

int fmrx_rds_band_pass(int taps, double Fs, double Fb, double Fe, double *h)
{
    if (!h || taps < 2) return fail(FMRX_EINVAL, "rds_band_pass: bad arguments");
    design_bpf64(taps, Fs, Fb, Fe, h);
    return FMRX_OK;
}
int fmrx_rds_imp_response(int taps, double Fs, double Fc, double *h)
{
    if (!h || taps < 2) return fail(FMRX_EINVAL, "rds_imp_response: bad arguments");
    design_lpf64(taps, Fs, Fc, h);
    return FMRX_OK;
}
int fmrx_rds_rrc(double Fs, int taps, double *h)
{
    if (!h || taps < 2) return fail(FMRX_EINVAL, "rds_rrc: bad arguments");
    design_rrc64(Fs, taps, h);
    return FMRX_OK;
}
int fmrx_rds_cdr(const double *x, size_t n, int sps, int block_count, double *state4, uint8_t *bits, size_t *n_bits)
{
    if (!x || !state4 || !bits || !n_bits || sps < 1) return fail(FMRX_EINVAL, "rds_cdr: bad arguments");
    *n_bits = cdr(x, n, sps, block_count, state4, bits);
    return FMRX_OK;
}
int fmrx_rds_diff_decode(const uint8_t *in, size_t n, uint8_t *out)
{
    if ((!in || !out) && n) return fail(FMRX_EINVAL, "rds_diff_decode: null buffer");
    for (size_t i = 0; i < n; i++) out[i] = i == 0 ? in[0] : (in[i] != in[i - 1]);
    return FMRX_OK;
}
int fmrx_rds_frame_sync(const uint8_t *bits, size_t n, char *offset_type, size_t *next_index)
{
    if ((!bits && n) || !offset_type || !next_index) return fail(FMRX_EINVAL, "rds_frame_sync: null argument");
    std::strcpy(offset_type, frame_sync(bits, n, next_index));
    return FMRX_OK;
}

int fmrx_rds_mode_params(int mode, fmrx_rds_params *p)
{
    if (!p) return fail(FMRX_EINVAL, "rds_mode_params: null");
    // model/fmMonoBlock.py:72-90: the model defines the RDS rates for modes 0 and 2 only
    if (mode == 0) *p = fmrx_rds_params{240000, 151, 247, 960, 26, 101};
    else if (mode == 2) *p = fmrx_rds_params{240000, 151, 817, 1920, 43, 101};
    else return fail(FMRX_EINVAL, "rds_mode_params: the reference's model defines RDS parameters for modes 0 and 2 only");
    return FMRX_OK;
}

int fmrx_rds_create(fmrx_rds **out, const fmrx_rds_params *p, size_t max_block, int device)
{
    if (!out || !p) return fail(FMRX_EINVAL, "rds_create: null argument");
    fmrx_rds *r = new fmrx_rds;
    int rc = r->c.plan("rds_create", p, 1, max_block);
    if (rc == FMRX_OK) rc = require_device();
    if (rc != FMRX_OK) {
        delete r;
        return rc;
    }
    auto body = [&]() -> int {
        FMRX_HIP(hipSetDevice(device));
        FMRX_TRY(r->c.create(device));
        FMRX_TRY(r->in.alloc(max_block));
        FMRX_HIP(hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking));
        return fmrx_rds_reset(r);
    };
    rc = body();
    if (rc != FMRX_OK) {
        fmrx_rds_destroy(r);
        return rc;
    }
    *out = r;
    return FMRX_OK;
}

int fmrx_rds_reset(fmrx_rds *r)
{
    if (!r) return fail(FMRX_EINVAL, "rds_reset: null handle");
    FMRX_TRY(r->c.reset(0, 1));
    r->decoded.clear();
    r->block = 0;
    return FMRX_OK;
}

int fmrx_rds_destroy(fmrx_rds *r)
{
    if (!r) return FMRX_OK;
    (void)hipSetDevice(r->c.device);
    if (r->stream) {
        (void)hipStreamSynchronize(r->stream);
        (void)hipStreamDestroy(r->stream);
    }
    delete r;
    return FMRX_OK;
}

size_t fmrx_rds_n_out(const fmrx_rds *r, size_t n) { return r ? r->c.n_out(n) : 0; }

int fmrx_rds_process_dev(fmrx_rds *r, const float *d_demod, size_t n, void *stream)
{
    if (!r || !d_demod) return fail(FMRX_EINVAL, "rds_process_dev: null argument");
    const size_t max_n = static_cast<size_t>(r->c.block);
    if (n == 0 || n > max_n) return fail(FMRX_EINVAL, "rds_process_dev: block of %zu samples (max %zu)", n, max_n);
    if ((n * r->c.p.upsamp) % r->c.p.decim)
        return fail(FMRX_EINVAL, "rds_process_dev: n*upsamp = %zu not a multiple of decim %d", n * r->c.p.upsamp, r->c.p.decim);
    FMRX_TRY(r->c.check_block("rds_process_dev", n));
    FMRX_HIP(hipSetDevice(r->c.device));
    return r->c.run(d_demod, n, n, static_cast<hipStream_t>(stream), nullptr);   // the bits are recovered on the host (fmrx_rds_process)
}

int fmrx_rds_process(fmrx_rds *r, const float *fm_demod, size_t n, double *rrc_i, double *rrc_q, uint8_t *bits, size_t *n_bits,
                     char *offset_type)
{
    if (!r || !fm_demod) return fail(FMRX_EINVAL, "rds_process: null argument");
    if (n > static_cast<size_t>(r->c.block)) return fail(FMRX_EINVAL, "rds_process: block of %zu samples (max %ld)", n, r->c.block);
    FMRX_HIP(hipSetDevice(r->c.device));
    hipStream_t s = r->stream;
    FMRX_HIP(hipMemcpyAsync(r->in.p, fm_demod, n * sizeof(float), hipMemcpyHostToDevice, s));
    FMRX_TRY(fmrx_rds_process_dev(r, r->in.p, n, s));
    const size_t no = r->c.last_out;
    std::vector<double> yi(no);
    FMRX_HIP(hipMemcpyAsync(yi.data(), r->c.yi.p, no * sizeof(double), hipMemcpyDeviceToHost, s));
    if (rrc_q) FMRX_HIP(hipMemcpyAsync(rrc_q, r->c.yq.p, no * sizeof(double), hipMemcpyDeviceToHost, s));
    FMRX_HIP(hipStreamSynchronize(s));
    if (rrc_i) std::memcpy(rrc_i, yi.data(), no * sizeof(double));
    // fmMonoBlock.py:276-297: clock and data recovery (its state is re-made every block there), differential decoding,
    // frame synchronisation over the bits kept so far
    double st[4] = {0.0, 0.0, 158.0, 0.0};
    std::vector<uint8_t> b(no / r->c.p.sps + 4), d;
    const size_t nb = cdr(yi.data(), no, r->c.p.sps, static_cast<int>(r->block), st, b.data());
    d.resize(nb);
    for (size_t i = 0; i < nb; i++) d[i] = i == 0 ? b[0] : (b[i] != b[i - 1]);
    if (bits) std::memcpy(bits, d.data(), nb);
    if (n_bits) *n_bits = nb;
    const char *off = frame_sync_append(r->decoded, d.data(), nb);
    if (offset_type) std::strcpy(offset_type, off);
    r->block++;
    return FMRX_OK;
}

int fmrx_rds_read_tap(fmrx_rds *r, int which, double *out, size_t *n)
{
    if (!r || !n) return fail(FMRX_EINVAL, "rds_read_tap: null argument");
    return r->c.tap("rds_read_tap", 0, which, out, n);
}

}  // extern "C"
