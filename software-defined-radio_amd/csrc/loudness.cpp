// loudness.cpp -- gated loudness by ITU-R BS.1770-4 over the audio meters' 100 ms bins (include/fmrx.h: fmrx_loudness_*;
// DESIGN.md section 4.14; tests/_audio_meters_model.py: gated()).  Host only: an integrator over what fmrx_audio_meters_collect
// returns.  Per channel it keeps the last 30 bin energies (rows summed) for the momentary and short-term readings, and the
// energies of the gating blocks -- 4 consecutive bins, hop one bin -- up to max_blocks for the integrated one.
#include "fmrx_internal.hpp"

#include <cmath>

using namespace fmrx;

namespace {

constexpr int kBlockBins = 4, kShortBins = 30;
constexpr double kOffset = -0.691, kAbsGate = -70.0, kRelGate = -10.0;

struct Channel {
    double last[kShortBins] = {};    // a ring: bin b lies at last[b % 30]
    uint64_t bins = 0;               // pushed since create / reset
    std::vector<double> blocks;      // block energies, in order
    bool full = false;
};

}  // namespace

struct fmrx_loudness {
    size_t bin_len = 0, max_blocks = 0;
    double fs2 = 0.0;
    std::vector<Channel> ch;
};

namespace {

// mean square -> LKFS by the dB edge rule: -99 where there is nothing
double lkfs(double z)
{
    if (!(z > 0.0)) return -99.0;
    const double v = kOffset + 10.0 * std::log10(z / 1.0);
    return v < -99.0 ? -99.0 : (v > 99.0 ? 99.0 : v);
}

}  // namespace

extern "C" {

int fmrx_loudness_create(fmrx_loudness **out, int n_channels, size_t bin_len, size_t max_blocks, double full_scale)
{
    if (!out) return fail(FMRX_EINVAL, "loudness_create: null argument");
    if (n_channels < 1 || bin_len < 1 || max_blocks < 1) return fail(FMRX_EINVAL, "loudness_create: n_channels, bin_len and max_blocks must be >= 1");
    if (!(full_scale > 0.0) || !std::isfinite(full_scale)) return fail(FMRX_EINVAL, "loudness_create: full_scale %g", full_scale);
    fmrx_loudness *l = new fmrx_loudness;
    l->bin_len = bin_len;
    l->max_blocks = max_blocks;
    l->fs2 = full_scale * full_scale;
    l->ch.resize(n_channels);
    *out = l;
    return FMRX_OK;
}

int fmrx_loudness_destroy(fmrx_loudness *l)
{
    delete l;
    return FMRX_OK;
}

int fmrx_loudness_reset(fmrx_loudness *l, int channel)
{
    if (!l) return fail(FMRX_EINVAL, "loudness_reset: null handle");
    if (channel >= static_cast<int>(l->ch.size())) return fail(FMRX_EINVAL, "loudness_reset: channel %d of %zu", channel, l->ch.size());
    for (size_t c = 0; c < l->ch.size(); c++)
        if (channel < 0 || static_cast<size_t>(channel) == c) l->ch[c] = Channel();
    return FMRX_OK;
}

int fmrx_loudness_push(fmrx_loudness *l, const fmrx_audio_meter *recs, const double *bins, size_t max_bins)
{
    if (!l || !recs || !bins) return fail(FMRX_EINVAL, "loudness_push: null argument");
    for (size_t c = 0; c < l->ch.size(); c++)
        if (recs[c].bins_done > max_bins) return fail(FMRX_EINVAL, "loudness_push: channel %zu closed %llu bins, the rows hold %zu", c, (unsigned long long)recs[c].bins_done, max_bins);
    for (size_t c = 0; c < l->ch.size(); c++) {
        Channel &k = l->ch[c];
        const double *b = bins + c * 2 * max_bins;
        for (size_t i = 0; i < recs[c].bins_done; i++) {
            k.last[k.bins % kShortBins] = b[i] + b[max_bins + i];
            k.bins++;
            if (k.bins < kBlockBins) continue;
            if (k.blocks.size() >= l->max_blocks) {
                k.full = true;
                continue;
            }
            const uint64_t j = k.bins - kBlockBins;
            k.blocks.push_back(((k.last[j % kShortBins] + k.last[(j + 1) % kShortBins]) + k.last[(j + 2) % kShortBins]) + k.last[(j + 3) % kShortBins]);
            if (k.blocks.size() == l->max_blocks) k.full = true;
        }
    }
    return FMRX_OK;
}

int fmrx_loudness_read(const fmrx_loudness *l, int channel, fmrx_loudness_levels *out)
{
    if (!l || !out) return fail(FMRX_EINVAL, "loudness_read: null argument");
    if (channel < 0 || channel >= static_cast<int>(l->ch.size())) return fail(FMRX_EINVAL, "loudness_read: channel %d of %zu", channel, l->ch.size());
    const Channel &k = l->ch[channel];
    const double L = static_cast<double>(l->bin_len);
    std::memset(out, 0, sizeof *out);
    out->momentary = out->short_term = out->integrated = -99.0;
    out->blocks = k.blocks.size();
    out->full = k.full;
    if (k.bins >= kBlockBins) {
        const uint64_t j = k.bins - kBlockBins;
        const double e = ((k.last[j % kShortBins] + k.last[(j + 1) % kShortBins]) + k.last[(j + 2) % kShortBins]) + k.last[(j + 3) % kShortBins];
        out->momentary = lkfs(e / (kBlockBins * L) / l->fs2);
    }
    if (k.bins >= kShortBins) {
        double s = 0.0;
        for (uint64_t j = k.bins - kShortBins; j < k.bins; j++) s = s + k.last[j % kShortBins];
        out->short_term = lkfs(s / (kShortBins * L) / l->fs2);
    }
    // the gates, on mean squares: a block is in where its loudness is above the gate's
    const double scale = kBlockBins * L, t_abs = std::pow(10.0, (kAbsGate - kOffset) / 10.0);
    double s = 0.0;
    size_t m = 0;
    for (double e : k.blocks) {
        const double z = e / scale / l->fs2;
        if (z > t_abs) {
            s = s + z;
            m++;
        }
    }
    if (m == 0) return FMRX_OK;
    const double t_rel = (s / static_cast<double>(m)) * std::pow(10.0, kRelGate / 10.0);
    s = 0.0;
    m = 0;
    for (double e : k.blocks) {
        const double z = e / scale / l->fs2;
        if (z > t_abs && z > t_rel) {
            s = s + z;
            m++;
        }
    }
    if (m) out->integrated = lkfs(s / static_cast<double>(m));
    return FMRX_OK;
}

}  // extern "C"
