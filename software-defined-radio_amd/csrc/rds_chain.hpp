// rds_chain.hpp -- the float64 RDS signal chain of N channels on the device, from discriminator rows to the matched-filter
// rows: what the single-stream handle (rds.hip, N = 1) and the RDS bank (rds_bank.hip) both run.  Defined in rds_bank.hip next to
// its kernels, where the data layout is described (not installed).
#pragma once
#include "fmrx_internal.hpp"

namespace fmrx {
namespace rds {

// where rdsb_cdr_kernel puts a call's bits; a handle that recovers its bits on the host passes none
struct CdrRows {
    int *blk;            // [N] 0 until a channel's first call
    uint8_t *bits;       // [N][max_bits]
    long max_bits;
    uint32_t *n_bits;    // [N]
};

struct Chain {
    fmrx_rds_params p{};
    int n_channels = 0, device = 0;
    long block = 0;                                // the largest block: the rows' pitches are made for it
    int Hx = 0, Hc = 0, Hm = 0, Hr = 0, delay = 0;
    long xpitch = 0, cpitch = 0, apitch = 0, npitch = 0, mpitch = 0, rpitch = 0, ypitch = 0;
    DevBuf<double> h_ch, h_car, h_rs, h_rrc, x, ch, car, arg, nco_i, nco_q, mi, mq, ri, rq, yi, yq, state;
    size_t last_n = 0, last_out = 0;               // samples per row of the last run (0 before the first)

    size_t n_out(size_t n) const { return n * p.upsamp / p.decim; }

    // Host only, before any device call: the parameters, the history sizes, the pitches for blocks of up to `block` samples.
    int plan(const char *who, const fmrx_rds_params *p, int n_channels, size_t block);
    // n is at least as long as every carried history (each is refreshed by a copy of its row's tail to its front)
    int check_block(const char *who, size_t n) const;
    // the four filter designs, the rows, the start-of-stream state
    int create(int device);
    // back to the start-of-stream state, channels [lo, hi)
    int reset(int lo, int hi);
    // One block of n <= block samples per channel, asynchronous on `stream`: d_demod f32 rows `pitch` floats apart.
    int run(const float *d_demod, size_t pitch, size_t n, hipStream_t stream, const CdrRows *cdr);
    // FMRX_RDS_TAP_* of one channel after the last run; out == NULL: the count only
    int tap(const char *who, int channel, int which, double *out, size_t *n);
};

}  // namespace rds
}  // namespace fmrx
