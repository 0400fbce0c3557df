// capi.hip -- the extern "C" layer of libfmrx.so (include/fmrx.h): library
// functions and the host-buffer stage API, one entry point per reference
// primitive (include/filter.h:18-43, include/iofunc.h:36 under /root/reference).
//
// Every stage function: validate (the reference's unchecked preconditions
// become FMRX_EINVAL) -> H2D into per-thread scratch (Stage) -> HIP kernel(s) -> D2H.
// No stage has a CPU implementation: without a device they return FMRX_ENODEV.
#include "fmrx_internal.hpp"
#include "rds_station.hpp"
#include <vector>

#include "build_id.hpp"   // FMRX_SRC_HASH: written by the Makefile (SHA-256 over the library's sources)

namespace fmrx {

// ---- error plumbing ----------------------------------------------------------
static thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int require_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(FMRX_ENODEV, "no usable HIP device (%s); libfmrx has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    }
    return FMRX_OK;
}

namespace {

// Per-thread device scratch of the stage functions: one set of slots, each its own allocation (so growing one never moves
// another, and each keeps hipMalloc's alignment), grown on demand and typed by whoever asks.  A call makes one Stage and gets
// slot k for its k-th request.  The host-buffer functions are synchronous and share the first kHostSlots; the two device-pointer
// functions, whose kernel may still run when the next call on this thread begins, each own a slot behind those.
constexpr int kHostSlots = 6, kDeemphDevSlot = 6, kStreamReadSlot = 7, kStageSlots = 8;
using StageSlot = DevBuf<unsigned char>;
thread_local StageSlot g_slots[kStageSlots];

inline int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    if (bytes) FMRX_HIP(hipMemcpy(dst, src, bytes, kind));
    return FMRX_OK;
}
inline int h2d(void *dst, const void *src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyHostToDevice); }
inline int d2h(void *dst, const void *src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToHost); }
inline int sync0()
{
    FMRX_HIP(hipStreamSynchronize(nullptr));
    return FMRX_OK;
}

template <typename T>
struct Dev {
    T *p = nullptr;
    size_t n = 0;   // elements asked for
};
struct Stage {
    int k, end;
    explicit Stage(int first = 0, int count = kHostSlots) : k(first), end(first + count) {}
    // device buffer for n outputs
    template <typename T>
    int out(Dev<T> &d, size_t n)
    {
        if (k >= end) return fail(FMRX_EINVAL, "stage scratch: no slot %d for this call", k);
        StageSlot &slot = g_slots[k++];
        FMRX_TRY(slot.ensure(n * sizeof(T)));
        d = {reinterpret_cast<T *>(slot.p), n};
        return FMRX_OK;
    }
    // device buffer filled from this host array
    template <typename T>
    int in(Dev<T> &d, const T *host, size_t n)
    {
        FMRX_TRY(out(d, n));
        return h2d(d.p, host, n * sizeof(T));
    }
    // part of a buffer (the [history | block] layouts): n elements to d
    template <typename T>
    static int put(T *d, const T *host, size_t n) { return h2d(d, host, n * sizeof(T)); }
    // copy back: the whole buffer, or its first n elements
    template <typename T>
    static int back(T *host, const Dev<T> &d, size_t n = SIZE_MAX) { return d2h(host, d.p, (n < d.n ? n : d.n) * sizeof(T)); }
};

}  // namespace
}  // namespace fmrx

using namespace fmrx;

extern "C" {

const char *fmrx_version(void)
{
    return "fmrx 0.3 (gfx950) src:" FMRX_SRC_HASH;
}

// The process-wide defaults may be changed by one thread while another creates a handle (which copies them): writers and the
// copy go through one mutex (options_snapshot); per-block paths only ever read a handle's own copy.
int fmrx_set_option(const char *name, long value)
{
    std::lock_guard<std::mutex> lock(options_mutex());
    return set_option_in(default_options(), name, value);
}

int fmrx_get_option(const char *name, long *value)
{
    std::lock_guard<std::mutex> lock(options_mutex());
    return get_option_in(default_options(), name, value);
}
const char *fmrx_last_error(void) { return g_err; }

int fmrx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int fmrx_set_device(int device)
{
    FMRX_TRY(require_device());
    FMRX_HIP(hipSetDevice(device));
    return FMRX_OK;
}

int fmrx_host_alloc(void **out, size_t bytes)
{
    if (!out || bytes == 0) return fail(FMRX_EINVAL, "host_alloc: bad arguments");
    FMRX_TRY(require_device());
    FMRX_HIP(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return FMRX_OK;
}

int fmrx_host_free(void *p)
{
    if (p) FMRX_HIP(hipHostFree(p));
    return FMRX_OK;
}

// ---- element-wise stages ---------------------------------------------------------
int fmrx_u8_to_f32(const uint8_t *raw, size_t n, float *out)
{
    if ((!raw || !out) && n) return fail(FMRX_EINVAL, "u8_to_f32: null buffer");
    FMRX_TRY(require_device());
    Stage st;
    Dev<uint8_t> u;
    Dev<float> a;
    FMRX_TRY(st.in(u, raw, n));
    FMRX_TRY(st.out(a, n));
    FMRX_TRY(k_u8_to_f32(u.p, n, a.p, nullptr));
    return st.back(out, a);
}

int fmrx_deinterleave(const float *iq, size_t n_pairs, float *I, float *Q)
{
    if ((!iq || !I || !Q) && n_pairs) return fail(FMRX_EINVAL, "deinterleave: null buffer");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b, c;
    FMRX_TRY(st.in(a, iq, 2 * n_pairs));
    FMRX_TRY(st.out(b, n_pairs));
    FMRX_TRY(st.out(c, n_pairs));
    FMRX_TRY(k_deinterleave(a.p, n_pairs, b.p, c.p, nullptr));
    FMRX_TRY(st.back(I, b));
    return st.back(Q, c);
}

int fmrx_pcm16(const float *audio, size_t n, int16_t *out, int wrap)
{
    if ((!audio || !out) && n) return fail(FMRX_EINVAL, "pcm16: null buffer");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a;
    Dev<int16_t> s16;
    FMRX_TRY(st.in(a, audio, n));
    FMRX_TRY(st.out(s16, n));
    FMRX_TRY(k_pcm16(a.p, n, s16.p, wrap, nullptr));
    return st.back(out, s16);
}

// ---- FIR family -----------------------------------------------------------------------
// device layout for a block with carried history: [history | block], kernels get
// a pointer to the block and read history at negative indices.
static int fir_common(float *y, size_t n_out, const float *x, size_t n, const float *h, size_t taps,
                      const float *state, size_t n_hist, size_t n_tail_zero, unsigned decim)
{
    Stage st;
    Dev<float> a, dh, b;
    FMRX_TRY(st.out(a, n_hist + n + n_tail_zero));
    if (state) FMRX_TRY(st.put(a.p, state, n_hist));
    else FMRX_HIP(hipMemset(a.p, 0, n_hist * sizeof(float)));
    FMRX_TRY(st.put(a.p + n_hist, x, n));
    if (n_tail_zero) FMRX_HIP(hipMemset(a.p + n_hist + n, 0, n_tail_zero * sizeof(float)));
    FMRX_TRY(st.in(dh, h, taps));
    FMRX_TRY(st.out(b, n_out));
    FMRX_TRY(k_fir_generic(a.p + n_hist, n_out, dh.p, static_cast<int>(taps), static_cast<int>(decim), b.p, nullptr));
    return st.back(y, b);
}

int fmrx_convolve_fir(float *y, const float *x, size_t n, const float *h, size_t taps)
{
    if (!y || !x || !h || taps == 0 || n == 0) return fail(FMRX_EINVAL, "convolve_fir: bad arguments");
    if (taps > 65535) return fail(FMRX_EINVAL, "convolve_fir: taps %zu > 65535", taps);
    FMRX_TRY(require_device());
    // full convolution = block FIR over [0^(taps-1) | x | 0^(taps-1)]
    return fir_common(y, n + taps - 1, x, n, h, taps, nullptr, taps - 1, taps - 1, 1);
}

static int block_fir(const char *name, float *y, const float *x, size_t n, const float *h, size_t taps, float *state,
                     unsigned decim)
{
    if (!y || !x || !h || !state || taps == 0) return fail(FMRX_EINVAL, "%s: null buffer", name);
    if (decim == 0) return fail(FMRX_EINVAL, "%s: decim must be >= 1", name);
    if (taps > 65535) return fail(FMRX_EINVAL, "%s: taps %zu > 65535 (unsigned short in the reference)", name, taps);
    if (n < taps - 1)
        return fail(FMRX_EINVAL, "%s: block of %zu samples is shorter than taps-1 = %zu (state refresh would read before the block)",
                    name, n, taps - 1);
    FMRX_TRY(require_device());
    FMRX_TRY(fir_common(y, n / decim, x, n, h, taps, state, taps - 1, 0, decim));
    // state <- last taps-1 samples of x (src/filter.cpp:148-153, 182-187): a host copy in the reference too
    std::memcpy(state, x + n - (taps - 1), (taps - 1) * sizeof(float));
    return FMRX_OK;
}

int fmrx_convolve_block_fir(float *y, const float *x, size_t n, const float *h, size_t taps, float *state)
{
    return block_fir("convolve_block_fir", y, x, n, h, taps, state, 1);
}

int fmrx_convolve_block_fast_fir(float *y, const float *x, size_t n, const float *h, size_t taps, float *state,
                                 unsigned decim)
{
    return block_fir("convolve_block_fast_fir", y, x, n, h, taps, state, decim);
}

int fmrx_convolve_block_resample_fir(float *y, const float *x, size_t n, const float *h, size_t taps, float *state,
                                     unsigned decim, unsigned upsamp)
{
    if (!y || !x || !h || !state || taps == 0) return fail(FMRX_EINVAL, "convolve_block_resample_fir: null buffer");
    if (decim == 0 || upsamp == 0) return fail(FMRX_EINVAL, "convolve_block_resample_fir: decim and upsamp must be >= 1");
    if (taps > 65535) return fail(FMRX_EINVAL, "convolve_block_resample_fir: taps %zu > 65535", taps);
    if (n * upsamp < taps - 1)
        return fail(FMRX_EINVAL, "convolve_block_resample_fir: n*upsamp = %zu < taps-1 = %zu", n * upsamp, taps - 1);
    FMRX_TRY(require_device());
    // The reference keeps its state in the UPSAMPLED index space: stream sample
    // x[-d] (d = 1..H) lives in state[taps-1 - d*upsamp]  (src/filter.cpp:207, 218-222).
    const size_t H = (taps - 1) / upsamp;
    std::vector<float> hist(H ? H : 1, 0.0f);
    for (size_t d = 1; d <= H; d++) hist[H - d] = state[taps - 1 - d * upsamp];
    Stage st;
    Dev<float> a, b;
    const size_t Hp = (H + 3) / 4 * 4;   // keeps the block 16-byte aligned behind its history
    FMRX_TRY(st.out(a, Hp + n));
    FMRX_TRY(st.out(b, (n * upsamp) / decim));
    FMRX_TRY(st.put(a.p + (Hp - H), hist.data(), H));
    FMRX_TRY(st.put(a.p + Hp, x, n));
    // polyphase-table kernels (bit-exact: the reference's operations in its order, kernels_resample.hip);
    // the LDS-resident-table form from 65 536 outputs per call unless the option resample_l2 is set
    // the plan (polyphase table, tap images: several device allocations and copies) is kept per thread and rebuilt only when
    // the filter changes: a block-streaming caller passes the same taps every call (src/project.cpp:353)
    struct PlanCache {
        ResamplePlan plan;
        std::vector<float> h;
        unsigned decim = 0, upsamp = 0;
    };
    static thread_local PlanCache pc;
    if (pc.decim != decim || pc.upsamp != upsamp || pc.h.size() != taps || std::memcmp(pc.h.data(), h, taps * sizeof(float)) != 0) {
        pc.decim = pc.upsamp = 0;                              // invalid until the new plan is complete
        FMRX_TRY(resample_plan_init(pc.plan, h, static_cast<int>(taps), static_cast<int>(decim), static_cast<int>(upsamp)));
        pc.h.assign(h, h + taps);
        pc.decim = decim;
        pc.upsamp = upsamp;
    }
    FMRX_TRY(resample_launch(pc.plan, a.p + Hp, n, 0, b.p, options_snapshot(), nullptr, false, /*exact=*/true));
    FMRX_TRY(sync0());
    FMRX_TRY(st.back(y, b));
    // state refresh exactly as src/filter.cpp:218-222 (host copy): k = U-1; for
    // i = U*n-(taps-1); i < U*n-U; i += U: state[k] = x[i/U + 1]; k += U
    {
        const long U = upsamp, ns = static_cast<long>(taps) - 1, N = static_cast<long>(n);
        long k = U - 1;
        for (long i = U * N - ns; i < U * N - U; i += U) {
            state[k] = x[(i / U) + 1];
            k += U;
        }
    }
    return FMRX_OK;
}

int fmrx_upsample(const float *x, size_t n, float *xu, int up)
{
    if ((!x || !xu) && n) return fail(FMRX_EINVAL, "upsample: null buffer");
    if (up < 1) return fail(FMRX_EINVAL, "upsample: rate must be >= 1");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b;
    FMRX_TRY(st.in(a, x, n));
    FMRX_TRY(st.out(b, n * up));
    FMRX_TRY(k_upsample(a.p, n, b.p, up, nullptr));
    return st.back(xu, b);
}

int fmrx_downsample(float *out, size_t *n_out, const float *in, size_t n, unsigned short ds)
{
    if (!out || !in || !n_out) return fail(FMRX_EINVAL, "downsample: null buffer");
    if (ds == 0) return fail(FMRX_EINVAL, "downsample: factor must be >= 1");
    FMRX_TRY(require_device());
    // size rule of src/filter.cpp:240: ceil(n / (float)ds), evaluated in float
    const size_t ny = static_cast<size_t>(ceilf(static_cast<float>(n) / static_cast<float>(ds)));
    *n_out = ny;
    Stage st;
    Dev<float> a, b;
    FMRX_TRY(st.out(a, n + ds));
    FMRX_TRY(st.put(a.p, in, n));
    FMRX_TRY(st.out(b, ny));
    FMRX_TRY(k_downsample(a.p, ny, b.p, ds, nullptr));
    return st.back(out, b);
}

// ---- demod / stereo helpers -----------------------------------------------------------
int fmrx_fm_demod(float *out, const float *I, const float *Q, size_t n, float *prev_i, float *prev_q)
{
    if (!out || !I || !Q || !prev_i || !prev_q) return fail(FMRX_EINVAL, "fm_demod: null buffer");
    if (n == 0) return FMRX_OK;
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b, c;
    FMRX_TRY(st.in(a, I, n));
    FMRX_TRY(st.in(b, Q, n));
    FMRX_TRY(st.out(c, n));
    FMRX_TRY(k_fm_demod_planar(a.p, b.p, n, *prev_i, *prev_q, c.p, nullptr));
    FMRX_TRY(st.back(out, c));
    *prev_i = I[n - 1];
    *prev_q = Q[n - 1];
    return FMRX_OK;
}

int fmrx_fm_demod_arctan(double *out, const double *I, const double *Q, size_t n, double *prev_phase)
{
    if (!out || !I || !Q || !prev_phase) return fail(FMRX_EINVAL, "fm_demod_arctan: null buffer");
    if (n == 0) return FMRX_OK;
    FMRX_TRY(require_device());
    Stage st;
    Dev<double> di, dq, dout;
    FMRX_TRY(st.in(di, I, n));
    FMRX_TRY(st.in(dq, Q, n));
    FMRX_TRY(st.out(dout, n));
    // the phase in front of the block only matters modulo 2 pi (np.unwrap's mod takes care of the turns it has accumulated)
    FMRX_TRY(k_fm_demod_arctan_planar(di.p, dq.p, n, *prev_phase, dout.p, nullptr));
    FMRX_TRY(st.back(out, dout));
    double ph = *prev_phase;                                // the model's running (unwrapped) phase: prev + the steps, in order
    for (size_t k = 0; k < n; k++) ph += out[k];
    *prev_phase = ph;
    return FMRX_OK;
}

int fmrx_all_pass(const float *in, size_t n, float *state, size_t nstate, float *out)
{
    if (!in || !state || !out) return fail(FMRX_EINVAL, "all_pass: null buffer");
    if (n < nstate) return fail(FMRX_EINVAL, "all_pass: block of %zu samples shorter than the delay %zu", n, nstate);
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b, c;
    FMRX_TRY(st.in(a, in, n));
    FMRX_TRY(st.in(b, state, nstate));
    FMRX_TRY(st.out(c, n));
    FMRX_TRY(k_all_pass(a.p, n, b.p, nstate, c.p, nullptr));
    FMRX_TRY(st.back(out, c));
    std::memcpy(state, in + n - nstate, nstate * sizeof(float));
    return FMRX_OK;
}

int fmrx_fm_pll(const float *in, size_t n, float *nco_out, float *state, float freq, float Fs, float ncoScale,
                float phaseAdjust, float normBandwidth)
{
    if (!in || !nco_out || !state) return fail(FMRX_EINVAL, "fm_pll: null buffer");
    if (!(Fs > 0)) return fail(FMRX_EINVAL, "fm_pll: Fs must be positive");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b, c;
    FMRX_TRY(st.in(a, in, n));
    FMRX_TRY(st.out(b, n + 1));
    FMRX_TRY(st.in(c, state, 6));
    FMRX_TRY(k_fm_pll(a.p, n, b.p, c.p, freq, Fs, ncoScale, phaseAdjust, normBandwidth, 0, nullptr));
    FMRX_TRY(st.back(nco_out, b));
    return st.back(state, c);
}

// The parallel-in-time PLL exactly as pll_stage (pipeline.hip) runs it for a warm pipeline, with what it left in its scratch
// area.  The host contract of k_fm_pll_parallel lives here: the device input is a fresh allocation (16-byte aligned) with 16
// zero floats behind in[n-1]; the scratch area starts zeroed (no drift record, diagnostics of this call alone).
int fmrx_fm_pll_parallel(const float *in, size_t n, float *nco_out, float *state, float freq, float Fs, float ncoScale,
                         float phaseAdjust, float normBandwidth, double off_hint, fmrx_pll_parallel_info *info, float *records,
                         uint64_t *mask)
{
    if ((!in && n) || !nco_out || !state) return fail(FMRX_EINVAL, "fm_pll_parallel: null buffer");
    if (!(Fs > 0)) return fail(FMRX_EINVAL, "fm_pll_parallel: Fs must be positive");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b, c, d;
    FMRX_TRY(st.out(a, n + 16));
    FMRX_TRY(st.out(b, n + 17));
    FMRX_TRY(st.out(c, 8));
    FMRX_TRY(st.out(d, pll_parallel_scratch_floats(n)));
    FMRX_TRY(st.put(a.p, in, n));
    FMRX_HIP(hipMemset(a.p + n, 0, 16 * sizeof(float)));
    FMRX_HIP(hipMemset(d.p, 0, d.n * sizeof(float)));
    FMRX_TRY(st.put(c.p, state, 6));
    const float trig_offset = state[5];
    const Options o = options_snapshot();
    PllParallelShape sh{};
    FMRX_TRY(k_fm_pll_parallel(a.p, n, b.p, c.p, freq, Fs, ncoScale, phaseAdjust, normBandwidth, d.p, o, nullptr, off_hint, 3, nullptr,
                               &sh));
    FMRX_TRY(st.back(nco_out, b, n + 1));
    FMRX_TRY(st.back(state, c, 6));
    const size_t nseg = static_cast<size_t>(sh.nseg);
    if (info) {
        unsigned hdr[8];
        FMRX_TRY(d2h(hdr, d.p, sizeof(hdr)));
        info->L = sh.L;
        info->W = sh.W;
        info->lti = sh.lti ? 1 : 0;
        info->nseg = nseg;
        info->repaired = hdr[2];
        std::memcpy(&info->max_dphase, &hdr[3], sizeof(float));
        std::memcpy(&info->max_dinteg, &hdr[4], sizeof(float));
        pll_parallel_tolerances(trig_offset, n, freq, Fs, normBandwidth, sh.lti, &info->tol_phase, &info->tol_integ);
    }
    if (nseg == 0) return FMRX_OK;
    if (records) {
        std::vector<float> seg(nseg * 16);
        FMRX_TRY(d2h(seg.data(), d.p + 8, seg.size() * sizeof(float)));
        for (size_t i = 0; i < nseg; i++) {
            float *r = records + i * FMRX_PLL_RECORD_FLOATS;
            for (int u = 0; u < 6; u++) r[u] = seg[i * 16 + u];
            r[6] = seg[i * 16 + 8];
            r[7] = seg[i * 16 + 9];
            r[8] = seg[i * 16 + 10];
        }
    }
    if (mask) FMRX_TRY(d2h(mask, d.p + 8 + (nseg + 1) * 16, (nseg / 64 + 1) * sizeof(uint64_t)));
    return FMRX_OK;
}

int fmrx_stereo_mix(const float *stereo_filt, const float *pll, size_t n, float *mixer)
{
    if ((!stereo_filt || !pll || !mixer) && n) return fail(FMRX_EINVAL, "stereo_mix: null buffer");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b, c;
    FMRX_TRY(st.in(a, stereo_filt, n));
    FMRX_TRY(st.in(b, pll, n));
    FMRX_TRY(st.out(c, n));
    FMRX_TRY(k_mix(a.p, b.p, n, c.p, nullptr));
    return st.back(mixer, c);
}

int fmrx_stereo_combine(const float *stereo_final, const float *mono, size_t n, float *left, float *right)
{
    if ((!stereo_final || !mono || !left || !right) && n) return fail(FMRX_EINVAL, "stereo_combine: null buffer");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b, c, d;
    FMRX_TRY(st.in(a, stereo_final, n));
    FMRX_TRY(st.in(b, mono, n));
    FMRX_TRY(st.out(c, n));
    FMRX_TRY(st.out(d, n));
    FMRX_TRY(k_combine(a.p, b.p, n, c.p, d.p, nullptr));
    FMRX_TRY(st.back(left, c));
    return st.back(right, d);
}

// ---- de-emphasis (no counterpart in the reference) -------------------------------------------
int fmrx_deemph_design(double fs, double tau_us, float *p, float *b0)
{
    if (!p || !b0) return fail(FMRX_EINVAL, "deemph_design: null argument");
    if (!(fs > 0.0) || !(tau_us > 0.0)) return fail(FMRX_EINVAL, "deemph_design: fs and tau must be positive");
    // bilinear transform of 1 / (1 + s tau), pre-warped at the corner; float64 throughout, rounded to float32 at the end
    const double tau = tau_us * 1e-6;
    const double a = 1.0 / (2.0 * fs * tau);
    if (!(a < 0.78539816339744830962)) return fail(FMRX_EINVAL, "deemph_design: 1 / (2 fs tau) = %g must be below pi / 4 (0 < p < 1)", a);
    const double k = -tan(a);
    const double pd = (1.0 + k) / (1.0 - k);
    *p = static_cast<float>(pd);
    *b0 = static_cast<float>((1.0 - pd) / 2.0);
    return FMRX_OK;
}

int fmrx_deemph(float *y, const float *x, size_t rows, size_t n, size_t pitch, float p, float b0, float *state, unsigned *missed)
{
    if (!y || !x || !state) return fail(FMRX_EINVAL, "deemph: null buffer");
    if (pitch < n) return fail(FMRX_EINVAL, "deemph: pitch %zu < n %zu", pitch, n);
    if (missed) *missed = 0;
    if (rows == 0 || n == 0) return FMRX_OK;
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> dx, dy, dstate;
    Dev<unsigned long long> cnt;
    FMRX_TRY(st.in(dx, x, rows * pitch));
    FMRX_TRY(st.in(dy, y, rows * pitch));   // (what lies between the rows of y stays the caller's)
    FMRX_TRY(st.in(dstate, state, 2 * rows));
    FMRX_TRY(st.out(cnt, 1));
    FMRX_HIP(hipMemset(cnt.p, 0, sizeof(unsigned long long)));
    FMRX_TRY(fmrx_deemph_dev(dy.p, dx.p, rows, n, pitch, p, b0, dstate.p, cnt.p, nullptr));
    FMRX_TRY(sync0());
    FMRX_TRY(st.back(y, dy));
    FMRX_TRY(st.back(state, dstate));
    unsigned long long m = 0;
    FMRX_TRY(st.back(&m, cnt));
    if (missed) *missed = static_cast<unsigned>(m);
    return FMRX_OK;
}

int fmrx_deemph_dev(float *d_y, const float *d_x, size_t rows, size_t n, size_t pitch, float p, float b0, float *d_state,
                    unsigned long long *d_missed, void *stream)
{
    if (!d_y || !d_x || !d_state || !d_missed) return fail(FMRX_EINVAL, "deemph_dev: null buffer");
    if (pitch < n) return fail(FMRX_EINVAL, "deemph_dev: pitch %zu < n %zu", pitch, n);
    FMRX_TRY(require_device());
    const Options o = options_snapshot();
    Dev<float> seg;                          // (grows with the shape: a device-wide wait then, not per call)
    FMRX_TRY(Stage(kDeemphDevSlot, 1).out(seg, deemph_scratch_floats(rows, n, o)));
    DeemphArgs a;
    a.x = d_x;
    a.y = d_y;
    a.pitch_x = a.pitch_y = static_cast<long>(pitch);
    a.rows = rows;
    a.n = n;
    a.p = p;
    a.b0 = b0;
    a.state = d_state;
    a.seg = seg.p;
    a.missed = d_missed;
    return deemph_launch(a, o, false, static_cast<hipStream_t>(stream), nullptr);
}

// ---- diagnostics ---------------------------------------------------------------------------
int fmrx_diag_libm(int fn, const float *a, const float *b, size_t n, float *out)
{
    if (fn < 0 || fn > 6)
        return fail(FMRX_EINVAL, "diag_libm: fn must be 0 (sinf), 1 (cosf), 2 (atan2f), 3..5 (their branch-free forms) or 6 (rcp)");
    if ((!a || !out || (fn % 3 == 2 && !b)) && n) return fail(FMRX_EINVAL, "diag_libm: null buffer");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> da, db, dc;
    FMRX_TRY(st.in(da, a, n));
    FMRX_TRY(fn % 3 == 2 ? st.in(db, b, n) : st.out(db, n));
    FMRX_TRY(st.out(dc, n));
    FMRX_TRY(k_libm_eval(fn, da.p, db.p, n, dc.p, nullptr));
    return st.back(out, dc);
}

int fmrx_diag_demod_fast(float *out, const float *iq, size_t n, float prev_i, float prev_q, int bounded)
{
    if ((!out || !iq) && n) return fail(FMRX_EINVAL, "diag_demod_fast: null buffer");
    if (bounded != 0 && bounded != 1) return fail(FMRX_EINVAL, "diag_demod_fast: bounded must be 0 or 1");
    if (n == 0) return FMRX_OK;
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> dz, dp, dc;
    const float prev[2] = {prev_i, prev_q};
    FMRX_TRY(st.in(dz, iq, 2 * n));
    FMRX_TRY(st.in(dp, prev, 2));
    FMRX_TRY(st.out(dc, n));
    FMRX_TRY(k_fm_demod_if(dz.p, n, dp.p, nullptr, dc.p, bounded ? 2 : 1, nullptr));
    return st.back(out, dc);
}

int fmrx_diag_stream_read_dev(const void *d_buf, size_t bytes, int method, void *stream)
{
    if (!d_buf || method < 0 || (method & ~0x10000) > 4096) return fail(FMRX_EINVAL, "diag_stream_read_dev: bad arguments");
    FMRX_TRY(require_device());
    Dev<unsigned> sink;
    FMRX_TRY(Stage(kStreamReadSlot, 1).out(sink, 4));
    return k_stream_read(d_buf, bytes, method, sink.p, static_cast<hipStream_t>(stream));
}

int fmrx_estimate_psd(float *freq, float *psd, const float *samples, size_t n, float Fs, int nfft)
{
    if (!freq || !psd || !samples) return fail(FMRX_EINVAL, "estimate_psd: null buffer");
    if (nfft < 2 || nfft % 2 || nfft > 65536) return fail(FMRX_EINVAL, "estimate_psd: nfft must be even and in 2..65536");
    if (n < static_cast<size_t>(nfft)) return fail(FMRX_EINVAL, "estimate_psd: %zu samples < nfft %d", n, nfft);
    if (!(Fs > 0)) return fail(FMRX_EINVAL, "estimate_psd: Fs must be positive");
    FMRX_TRY(require_device());
    Stage st;
    Dev<float> a, b, c, d;
    const size_t nseg = n / nfft, half = nfft / 2;
    FMRX_TRY(st.out(a, n));
    FMRX_TRY(st.put(a.p, samples, nseg * nfft));
    FMRX_TRY(st.out(b, nseg * half));
    FMRX_TRY(st.out(c, half));
    FMRX_TRY(st.out(d, half));
    FMRX_TRY(k_estimate_psd(a.p, n, Fs, nfft, b.p, c.p, d.p, nullptr));
    FMRX_TRY(st.back(freq, c));
    return st.back(psd, d);
}

// ---- fused front end as a stage ----------------------------------------------------------
struct fmrx_fe_plan {
    FePlan plan;
};

int fmrx_fe_plan_create(fmrx_fe_plan **out, const float *h, size_t taps, unsigned decim)
{
    if (!out || !h) return fail(FMRX_EINVAL, "fe_plan_create: null argument");
    if (taps < 2 || taps > 65535) return fail(FMRX_EINVAL, "fe_plan_create: taps %zu not in 2..65535", taps);
    if (decim == 0) return fail(FMRX_EINVAL, "fe_plan_create: decim must be >= 1");
    FMRX_TRY(require_device());
    fmrx_fe_plan *p = new fmrx_fe_plan;
    int rc = fe_plan_init(p->plan, h, static_cast<int>(taps), static_cast<int>(decim));
    if (rc != FMRX_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return FMRX_OK;
}

int fmrx_fe_plan_destroy(fmrx_fe_plan *plan)
{
    delete plan;
    return FMRX_OK;
}

int fmrx_fe_plan_is_specialised(const fmrx_fe_plan *plan) { return plan && plan->plan.fast ? 1 : 0; }
size_t fmrx_fe_plan_history_bytes(const fmrx_fe_plan *plan) { return plan ? plan->plan.hist_bytes : 0; }

int fmrx_fe_run_dev(const fmrx_fe_plan *plan, const uint8_t *d_iq, size_t n_samples, const uint8_t *d_hist, float *d_if,
                    int force_generic, void *stream)
{
    if (!plan || !d_iq || !d_if) return fail(FMRX_EINVAL, "fe_run_dev: null argument");
    return fe_launch(plan->plan, d_iq, n_samples, d_hist, d_if, options_snapshot(), static_cast<hipStream_t>(stream),
                     force_generic != 0);
}

int fmrx_fe_fir_decim_u8(const uint8_t *iq, size_t n_samples, const float *h, size_t taps, unsigned decim, uint8_t *hist,
                         float *if_i, float *if_q, int force_generic)
{
    if (!iq || !h) return fail(FMRX_EINVAL, "fe_fir_decim_u8: null buffer");
    if (taps < 2 || taps > 65535) return fail(FMRX_EINVAL, "fe_fir_decim_u8: taps %zu not in 2..65535", taps);
    if (decim == 0) return fail(FMRX_EINVAL, "fe_fir_decim_u8: decim must be >= 1");
    if (hist && n_samples < taps - 1)
        return fail(FMRX_EINVAL, "fe_fir_decim_u8: block of %zu samples shorter than taps-1 = %zu", n_samples, taps - 1);
    FMRX_TRY(require_device());
    FePlan plan;
    FMRX_TRY(fe_plan_init(plan, h, static_cast<int>(taps), static_cast<int>(decim)));
    Stage st;
    Dev<uint8_t> u, uh;
    Dev<float> a, b, c;
    const size_t n_out = n_samples / decim;
    const size_t hb = plan.hist_bytes, live = 2 * (taps - 1);
    FMRX_TRY(st.in(u, iq, 2 * n_samples));
    FMRX_TRY(st.out(uh, hb));
    FMRX_TRY(st.out(a, 2 * n_out));
    FMRX_TRY(st.out(b, n_out));
    FMRX_TRY(st.out(c, n_out));
    if (hist) {
        FMRX_TRY(k_fill_u8(uh.p, hb, 128, nullptr));
        FMRX_TRY(st.put(uh.p + (hb - live), hist, live));
    }
    FMRX_TRY(fe_launch(plan, u.p, n_samples, hist ? uh.p : nullptr, a.p, options_snapshot(), nullptr, force_generic != 0));
    FMRX_TRY(k_split_if(a.p, n_out, b.p, c.p, nullptr));
    if (if_i) FMRX_TRY(st.back(if_i, b));
    if (if_q) FMRX_TRY(st.back(if_q, c));
    FMRX_TRY(sync0());
    if (hist) std::memcpy(hist, iq + 2 * n_samples - live, live);  // carry: the last taps-1 samples, as bytes
    return FMRX_OK;
}

}  // extern "C"

// ---- RDS station decoder on the host (rds_station.hpp; the bank's rdsb_station_kernel runs the same functions) ----------
struct fmrx_rds_station_decoder {
    fmrx::rdsst::Dec d;
    double E[fmrx::rdsst::kMaxSps];
    fmrx_rds_station rec;
    fmrx_rds_station_ext ext;
    int max_burst = 0;
    bool fed = false;                              // something has been fed since create / reset: the option is fixed
};

namespace {
// the correction table of rds_station.hpp, built at the first use
const uint32_t *burst_table()
{
    static const std::vector<uint32_t> tab = [] {
        std::vector<uint32_t> t(fmrx::rdsst::kBurstTableSize);
        if (fmrx::rdsst::build_burst_table(t.data()) != 367) std::abort();   // (the code's own property: cannot happen)
        return t;
    }();
    return tab.data();
}

void station_reset(fmrx_rds_station_decoder *d, int sps)
{
    fmrx::rdsst::init(d->d, sps, d->max_burst);
    for (double &e : d->E) e = 0.0;
    fmrx::rdsst::clear_record(&d->rec);
    fmrx::rdsst::clear_ext(&d->ext, d->max_burst);
    d->fed = false;
}

template <typename F>
int station_feed(fmrx_rds_station_decoder *d, size_t n, fmrx_rds_group *g, size_t max_g, size_t *n_g, fmrx_rds_station *st, F each)
{
    if (!d || !st) return fail(FMRX_EINVAL, "rds_station_feed: null argument");
    if ((g == nullptr) != (n_g == nullptr)) return fail(FMRX_EINVAL, "rds_station_feed: g and n_g go together");
    fmrx::rdsst::Out o{&d->rec, g, g ? static_cast<uint32_t>(std::min<size_t>(max_g, 0xFFFFFFFFu)) : 0u, 0u,
                       d->max_burst ? burst_table() : nullptr, &d->ext};
    if (n) d->fed = true;
    for (size_t i = 0; i < n; i++) each(i, o);
    fmrx::rdsst::finish(d->d, &d->rec);
    fmrx::rdsst::finish_ext(d->d, &d->ext);
    *st = d->rec;
    if (n_g) *n_g = o.n_g;
    return FMRX_OK;
}
}  // namespace

extern "C" {

int fmrx_rds_station_create(fmrx_rds_station_decoder **out, int sps)
{
    if (!out) return fail(FMRX_EINVAL, "rds_station_create: null argument");
    if (sps < 2 || sps > fmrx::rdsst::kMaxSps) return fail(FMRX_EINVAL, "rds_station_create: sps %d not in 2..%d", sps, fmrx::rdsst::kMaxSps);
    fmrx_rds_station_decoder *d = new fmrx_rds_station_decoder;
    station_reset(d, sps);
    *out = d;
    return FMRX_OK;
}

int fmrx_rds_station_destroy(fmrx_rds_station_decoder *d)
{
    delete d;
    return FMRX_OK;
}

int fmrx_rds_station_reset(fmrx_rds_station_decoder *d)
{
    if (!d) return fail(FMRX_EINVAL, "rds_station_reset: null handle");
    station_reset(d, d->d.sps);
    return FMRX_OK;
}

size_t fmrx_rds_station_max_groups(const fmrx_rds_station_decoder *d, size_t n_samples)
{
    return d ? fmrx::rdsst::max_groups_for_samples(n_samples, d->d.sps) : 0;
}

int fmrx_rds_station_feed_rrc(fmrx_rds_station_decoder *d, const double *rrc_i, size_t n, fmrx_rds_group *g, size_t max_g, size_t *n_g,
                              fmrx_rds_station *st)
{
    if (n && !rrc_i) return fail(FMRX_EINVAL, "rds_station_feed_rrc: null row");
    return station_feed(d, n, g, max_g, n_g, st, [&](size_t i, fmrx::rdsst::Out &o) { fmrx::rdsst::feed_sample(d->d, d->E, 1, rrc_i[i], o); });
}

int fmrx_rds_station_feed_bits(fmrx_rds_station_decoder *d, const uint8_t *bits, size_t n, fmrx_rds_group *g, size_t max_g, size_t *n_g,
                               fmrx_rds_station *st)
{
    if (n && !bits) return fail(FMRX_EINVAL, "rds_station_feed_bits: null bits");
    return station_feed(d, n, g, max_g, n_g, st, [&](size_t i, fmrx::rdsst::Out &o) { fmrx::rdsst::feed_bit(d->d, bits[i] ? 1 : 0, o); });
}

int fmrx_rds_station_set_correction(fmrx_rds_station_decoder *d, int max_burst)
{
    if (!d) return fail(FMRX_EINVAL, "rds_station_set_correction: null handle");
    if (max_burst < 0 || max_burst > fmrx::rdsst::kMaxBurst)
        return fail(FMRX_EINVAL, "rds_station_set_correction: max_burst %d not in 0..%d", max_burst, fmrx::rdsst::kMaxBurst);
    if (d->fed) return fail(FMRX_EINVAL, "rds_station_set_correction: only on a decoder fed nothing since create or reset");
    d->max_burst = max_burst;
    station_reset(d, d->d.sps);
    return FMRX_OK;
}

int fmrx_rds_station_ext_get(const fmrx_rds_station_decoder *d, fmrx_rds_station_ext *ext)
{
    if (!d || !ext) return fail(FMRX_EINVAL, "rds_station_ext_get: null argument");
    *ext = d->ext;
    return FMRX_OK;
}

int fmrx_rds_block_correct(uint32_t word26, int offset, int max_burst, uint16_t *info, int *burst_len)
{
    if (offset < 0 || offset > 4 || max_burst < 0 || max_burst > fmrx::rdsst::kMaxBurst || (word26 >> 26)) return -1;
    uint32_t w = word26;
    const uint32_t sx = fmrx::rdsst::syndrome(w) ^ fmrx::rdsst::syndrome_of_offset(offset);
    const int len = sx ? fmrx::rdsst::correct_block(w, sx, max_burst, burst_table()) : 0;
    if (info) *info = static_cast<uint16_t>(w >> 10);
    if (burst_len) *burst_len = len;
    return sx == 0 ? 0 : len ? 1 : 2;
}

}  // extern "C"
