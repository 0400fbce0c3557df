// rds_common.hpp -- host helpers of the RDS path shared by the single-stream handle (rds.hip) and the RDS bank
// (rds_bank.hip): the float64 coefficient design and the model's bit recovery (not installed).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fmrx {
namespace rds {

constexpr double kPi = 3.141592653589793;   // math.pi / np.pi

// fmSupportLib.py:358-385, 251-287
void design_lpf64(int n, double Fs, double Fc, double *h);
void design_bpf64(int n, double Fs, double Fb, double Fe, double *h);
void design_rrc64(double Fs, int n, double *h);

// fmSupportLib.py:103-249: clock and data recovery incl. Manchester decoding.  state = {pair0, pair1, start, prev_size}
// (in/out); bits: room for n/sps + 2.  Returns the number of bits.
size_t cdr(const double *x, size_t n, int sps, int block_count, double *state, uint8_t *bits);

// fmSupportLib.py:30-100: the last offset word recognised in bits[0, n) ("A", "B", "C", "C_apos", "D" or " ") and the index
// the next call starts from
const char *frame_sync(const uint8_t *bits, size_t n, size_t *next_index);

// fmMonoBlock.py:283-297: frame synchronisation over the bits kept so far.  Appends a block's nb decoded bits to `kept`, returns
// the offset word frame_sync finds in them and drops the bits in front of the index the next block starts from.
const char *frame_sync_append(std::vector<uint8_t> &kept, const uint8_t *bits, size_t nb);

}  // namespace rds
}  // namespace fmrx
