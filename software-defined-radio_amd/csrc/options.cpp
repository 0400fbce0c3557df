// options.cpp -- the run-time options (include/fmrx.h describes them): one row per option.  fmrx_set_option, fmrx_get_option,
// fmrx_pipeline_set_option and the one-time read of the environment all walk this table, so a value is checked the same way
// wherever it comes from.  The built-in default of an option is its member initialiser in Options (fmrx_internal.hpp).
#include "fmrx_internal.hpp"

#include <cctype>
#include <cerrno>
#include <climits>

namespace fmrx {
namespace {

struct OptionRow {
    const char *name;            // the environment variable is FMRX_ + this name in capitals
    int Options::*i; long Options::*l;   // the member: an int or a long
    long lo, hi;                 // inclusive range
    bool not_zero;               // 0 is refused inside the range
    struct { const char *name; long value; } named[2];   // values that also go by a name
};
constexpr OptionRow kOptions[] = {
    {"fe_variant", &Options::fe_variant, nullptr, 0, 1, false, {{"mfma", 0}, {"valu", 1}}},   // front end: matrix-core / vector-ALU kernels
    {"fused_min_audio", nullptr, &Options::fused_min_audio, LONG_MIN, LONG_MAX, false, {}},   // audio samples per call from which the fused mono kernel runs
    {"resample_l2", &Options::resample_l2, nullptr, INT_MIN, INT_MAX, false, {}},             // 1 = L2-table resampler kernel even for large calls
    {"resample_exact", &Options::resample_exact, nullptr, INT_MIN, INT_MAX, false, {}},       // 1 = the pipeline's resampler keeps the reference's rounding sequence
    {"resample_chains", &Options::resample_chains, nullptr, INT_MIN, INT_MAX, false, {}},     // workgroups per XCD and tile group, matrix-core resampler (0 = all resident)
    {"overlap_calls", &Options::overlap_calls, nullptr, INT_MIN, INT_MAX, false, {}},         // 1 / 2 = stereo stages of consecutive calls on internal streams, a call apart
    {"pll_warmup", &Options::pll_warmup, nullptr, INT_MIN, INT_MAX, false, {}},               // parallel PLL: warm-up samples per lane (-1 = built-in)
    {"pll_segment", &Options::pll_segment, nullptr, INT_MIN, INT_MAX, false, {}},             //   samples per lane (-1 = built-in)
    {"pll_start", &Options::pll_start, nullptr, INT_MIN, INT_MAX, false, {}},                 //   lanes start from 1 = the linear system's state, 0 = the block's state plus drift
    {"pll_mode", &Options::pll_mode, nullptr, 0, 2, false, {}},                               // stereo PLL: 0 = parallel in time, 1 = serial, 2 = serial with glibc math
    {"demod", &Options::demod, nullptr, 0, 1, false, {{"discriminator", 0}, {"arctan", 1}}},  // the C++ reference's fmDemod / the model's fmDemodArctan
    {"tuner_variant", &Options::tuner_variant, nullptr, 0, 1, false, {{"mfma", 0}, {"generic", 1}}},   // wideband tuner kernel; read when a tuner is created
    {"deemph_warmup", &Options::deemph_warmup, nullptr, -1, 1 << 20, false, {}},              // parallel de-emphasis: warm-up samples per lane (-1 = built-in)
    {"deemph_segment", &Options::deemph_segment, nullptr, -1, 1 << 20, true, {}},             //   samples per lane (-1 = built-in; 0 samples is no shape)
    {"deemph_mode", &Options::deemph_mode, nullptr, 0, 1, false, {}},                         // de-emphasis: 0 = parallel in time, 1 = one lane per row, serially
};

const OptionRow *find_option(const char *name)
{
    for (const OptionRow &r : kOptions)
        if (name && std::strcmp(name, r.name) == 0) return &r;
    fail(FMRX_EINVAL, "unknown option '%s'", name ? name : "(null)");
    return nullptr;
}

std::string allowed_values(const OptionRow &r)
{
    std::string s = std::to_string(r.lo) + " .. " + std::to_string(r.hi) + (r.not_zero ? " except 0" : "");
    for (const auto &nv : r.named)
        if (nv.name) s += std::string(", ") + nv.name + " = " + std::to_string(nv.value);
    return s;
}

// a row's name for a value, or a whole base-10 integer
bool parse_value(const OptionRow &r, const char *text, long *value)
{
    for (const auto &nv : r.named)
        if (nv.name && std::strcmp(text, nv.name) == 0) return *value = nv.value, true;
    char *end = nullptr;
    errno = 0;
    *value = std::strtol(text, &end, 10);
    return !std::isspace(static_cast<unsigned char>(text[0])) && end != text && *end == '\0' && errno != ERANGE;
}

}  // namespace

int set_option_in(Options &o, const char *name, long value)
{
    const OptionRow *r = find_option(name);
    if (!r) return FMRX_EINVAL;
    if (value < r->lo || value > r->hi || (r->not_zero && value == 0))
        return fail(FMRX_EINVAL, "option %s: %ld refused (allowed: %s)", r->name, value, allowed_values(*r).c_str());
    if (r->l) o.*(r->l) = value;
    else o.*(r->i) = static_cast<int>(value);
    return FMRX_OK;
}

int get_option_in(const Options &o, const char *name, long *value)
{
    const OptionRow *r = find_option(name);
    if (!r) return FMRX_EINVAL;
    if (!value) return fail(FMRX_EINVAL, "option %s: null result pointer", r->name);
    *value = r->l ? o.*(r->l) : o.*(r->i);
    return FMRX_OK;
}

// built-in values, overridden once by the environment (first use; thread-safe static initialisation)
Options &default_options()
{
    static Options o = [] {
        Options d;
        for (const OptionRow &r : kOptions) {
            std::string var = std::string("FMRX_") + r.name;
            for (char &c : var) c = static_cast<char>(std::toupper(static_cast<unsigned char>(c)));
            const char *e = std::getenv(var.c_str());
            long v = 0;
            if (e && !(parse_value(r, e, &v) && set_option_in(d, r.name, v) == FMRX_OK))
                std::fprintf(stderr, "libfmrx: %s=%s ignored (allowed: %s)\n", var.c_str(), e, allowed_values(r).c_str());
        }
        return d;
    }();
    return o;
}

std::mutex &options_mutex()
{
    static std::mutex m;
    return m;
}

Options options_snapshot()
{
    std::lock_guard<std::mutex> lock(options_mutex());
    return default_options();
}

}  // namespace fmrx
