// rds_common.cpp -- host helpers of the RDS path (rds_common.hpp): the model's float64 coefficient design and its bit
// recovery, used by the single-stream handle (rds.hip) and the RDS bank (rds_bank.hip).
#include "rds_common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace fmrx {
namespace rds {

namespace {
int symbol_to_bit(const double *pair) { return pair[0] > 0 ? 1 : 0; }
}  // namespace

// ---- host: coefficient design, float64 (fmSupportLib.py:358-385, 251-287) ----------------------------------------
void design_lpf64(int n, double Fs, double Fc, double *h)
{
    const double norm = Fc / (Fs / 2), c = (n - 1) / 2.0;
    for (int i = 0; i < n; i++) {
        double v;
        if (i == c) v = norm;
        else {
            const double a = kPi * norm * (i - c);
            v = norm * (std::sin(a) / a);
        }
        const double w = std::sin(i * kPi / n);
        h[i] = v * (w * w);
    }
}
void design_bpf64(int n, double Fs, double Fb, double Fe, double *h)
{
    const double center = ((Fe + Fb) / 2) / (Fs / 2), width = (Fe - Fb) / (Fs / 2), c = (n - 1) / 2.0;
    for (int i = 0; i < n; i++) {
        double v;
        if (i == c) v = width;
        else {
            const double a = kPi * width / 2 * (i - c);
            v = width * (std::sin(a) / a);
        }
        v = v * std::cos(i * kPi * center);
        const double w = std::sin(i * kPi / n);
        h[i] = v * (w * w);
    }
}
void design_rrc64(double Fs, int n, double *h)
{
    const double T = 1 / 2375.0, beta = 0.90;
    for (int k = 0; k < n; k++) {
        const double t = (k - n / 2.0) / Fs;
        if (t == 0.0) h[k] = 1.0 + beta * ((4 / kPi) - 1);
        else if (t == -T / (4 * beta) || t == T / (4 * beta))
            h[k] = (beta / std::sqrt(2.0)) * (((1 + 2 / kPi) * (std::sin(kPi / (4 * beta)))) + ((1 - 2 / kPi) * (std::cos(kPi / (4 * beta)))));
        else
            h[k] = (std::sin(kPi * t * (1 - beta) / T) + 4 * beta * (t / T) * std::cos(kPi * t * (1 + beta) / T)) /
                   (kPi * t * (1 - (4 * beta * t / T) * (4 * beta * t / T)) / T);
    }
}

// ---- host: bit recovery (fmSupportLib.py:103-249, 30-100) -----------------------------------------------------------
// state = {pair0, pair1, start, prev_size}; bits: room for n/sps + 2
size_t cdr(const double *x, size_t n, int sps, int block_count, double *state, uint8_t *bits)
{
    double pair[2] = {state[0], state[1]};
    const long start0 = static_cast<long>(state[2]), prev_size = static_cast<long>(state[3]);
    long start = start0;
    std::vector<uint8_t> head;
    std::vector<double> pts(n, 0.0), samples;
    long size = 0;
    for (;;) {
        std::fill(pts.begin(), pts.end(), 0.0);
        size = 0;
        for (long i = start; i < static_cast<long>(n); i += sps) {
            if (i == start && start == start0 && prev_size % 2 == 1) {   // the point that completes the previous block's pair
                pair[1] = x[i];
                head.push_back(static_cast<uint8_t>(symbol_to_bit(pair)));
                pair[0] = pair[1];
                start += sps;                                            // (the scan goes on from where it is)
                continue;
            }
            const bool far = i >= start + 2L * sps;
            const double a = far ? pts[i - 2L * sps] : 0.0, b = far ? pts[i - sps] : 0.0;
            if (far && a > 0 && b > 0 && x[i] > 0) pts[i] = -x[i];       // the third of three high / low points is flipped
            else if (far && a < 0 && b < 0 && x[i] < 0) pts[i] = -x[i];
            else pts[i] = x[i];
            size++;
        }
        samples.assign(static_cast<size_t>(size), 0.0);
        for (long i = start; i < static_cast<long>(n); i += sps) samples[(i - start) / sps] = pts[i];
        bool again = false;
        for (size_t i = 0; i + 1 < samples.size(); i += 2) {
            if ((samples[i] < 0 && samples[i + 1] < 0) || (samples[i] > 0 && samples[i + 1] > 0)) {
                if (std::fabs(samples[i]) < 0.3 || std::fabs(samples[i + 1]) < 0.3) {
                    if (std::fabs(samples[i]) < 0.3) samples[i] = -samples[i];
                    else samples[i + 1] = -samples[i + 1];
                } else {                                                 // cannot be mended: re-start one symbol later
                    start += sps;
                    if (block_count != 0) {
                        pair[1] = samples[0];
                        head.push_back(static_cast<uint8_t>(symbol_to_bit(pair)));
                        pair[0] = pair[1];
                    }
                    again = true;
                    break;
                }
            }
        }
        if (!again) break;
    }
    pair[0] = samples.empty() ? pair[0] : samples.back();
    const long last_index = (size - 1) * sps + start;
    state[0] = pair[0];
    state[1] = pair[1];
    state[2] = static_cast<double>(sps - (static_cast<long>(n) - last_index));
    state[3] = static_cast<double>(size);
    size_t nb = 0;
    for (uint8_t b : head) bits[nb++] = b;
    for (size_t i = 0; i + 1 < samples.size(); i += 2) bits[nb++] = (samples[i] > 0 && samples[i + 1] < 0) ? 1 : 0;   // manchestering
    return nb;
}

const char *frame_sync(const uint8_t *bits, size_t n, size_t *next_index)
{
    static const unsigned parity[26] = {0x200, 0x100, 0x080, 0x040, 0x020, 0x010, 0x008, 0x004, 0x002, 0x001, 0x2DC, 0x16E, 0x0B7,
                                        0x287, 0x39F, 0x313, 0x355, 0x376, 0x1BB, 0x201, 0x3DC, 0x1EE, 0x0F7, 0x2A7, 0x38F, 0x31B};
    const char *off = " ";
    size_t i = 0;
    while (i + 26 < n) {
        unsigned s = 0;
        for (int k = 0; k < 26; k++)
            if (bits[i + k] == 1) s ^= parity[k];
        const char *hit = s == 0x3D8 ? "A" : s == 0x3D4 ? "B" : s == 0x25C ? "C" : s == 0x3CC ? "C_apos" : s == 0x258 ? "D" : nullptr;
        if (hit) {
            off = hit;
            if (n - (i + 26) < 26) break;
            i += 26;
        } else {
            i += 1;
        }
    }
    *next_index = off[0] == ' ' ? i : i + 26;
    return off;
}

const char *frame_sync_append(std::vector<uint8_t> &kept, const uint8_t *bits, size_t nb)
{
    kept.insert(kept.end(), bits, bits + nb);
    size_t next = 0;
    const char *off = frame_sync(kept.data(), kept.size(), &next);
    kept.erase(kept.begin(), kept.begin() + static_cast<long>(std::min(next, kept.size())));
    return off;
}

}  // namespace rds
}  // namespace fmrx
