// meter_stage.hpp -- what the handles of a bank's meter chain share.  Handle: the device, the event the last call recorded and
// the wait on it, with make / destroy and the guard of a collect, for the signal meters (meters.hip) and all below.  OnAudio: a
// handle on a bank's audio rows, with the checks of a create and of a reset, each closed by a synchronise.  On it, two kinds.
// Stage: what the stages that sit behind a meters handle on a bank's audio share (blend.hip, highcut.hip, leveller.hip and their
// kernel files): the argument checks, the device call, the host call, status and reset, and the control kernel's body.  A stage
// adds its control structure, its kernels' own buffers, its launch(handle, Call) and its source of control data: the type Source
// that a call hands to launch, from_handle (what the meters handle in front left on the device, if it fits the stage) and
// from_records (the host's records, uploaded).  Mpx is that source for the stages behind the signal meters.
// Reader: what the meters that only read the audio rows share (audio_meters.hip, true_peak.hip, audio_spectrum.hip, audio_features.hip, audio_resample.hip): the checks
// of a call, the device call, the host call and its staging, their field-major arrays [fields][n_channels], the checks of a derive.
// A reader adds its
// buffers, its launch(handle, rows, pitch, n, stream) (the kernel and the asynchronous copies of its results), the unpacking of
// its records and its host arithmetic.
//
// Ordering: a call records the handle's `done` event on its stream; whatever touches the handle's rows from the host
// (reset, status_get, state_get, collect, the host call, a change of settings) waits for it first.  What a create or a reset clears
// on the null stream is clear before it returns, so that a call on any stream, non-blocking ones included, finds it so.
#pragma once
#include "fmrx_internal.hpp"

namespace fmrx {
namespace meter_stage {

struct Handle {
    int device = 0;
    hipEvent_t done = nullptr;
    bool ran = false;
    // behind the handle's last call, whatever stream that was on
    int wait()
    {
        FMRX_HIP(hipSetDevice(device));
        if (ran) FMRX_HIP(hipEventSynchronize(done));
        return FMRX_OK;
    }
    ~Handle()
    {
        if (done) (void)hipEventDestroy(done);
    }
};

// a new handle of type H (a Handle) on `device`: body(h) fills it, the event is made; nothing is left behind where either fails
template <class H, class Body>
int make(H **out, int device, Body body)
{
    FMRX_TRY(require_device());
    FMRX_HIP(hipSetDevice(device));
    H *h = new H;
    h->device = device;
    const auto all = [&]() -> int {
        FMRX_TRY(body(h));
        FMRX_HIP(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
        return FMRX_OK;
    };
    const int rc = all();
    if (rc != FMRX_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return FMRX_OK;
}

template <class H>
int destroy(H *h)
{
    if (!h) return FMRX_OK;
    (void)hipSetDevice(h->device);
    if (h->ran) (void)hipEventSynchronize(h->done);
    delete h;
    return FMRX_OK;
}

// in front of a collect: there is a call, and it is done
inline int collected(const char *who, Handle *h, const void *out)
{
    if (!h || !out) return fail(FMRX_EINVAL, "%s: null argument", who);
    if (!h->ran) return fail(FMRX_EINVAL, "%s: no call to collect", who);
    return h->wait();
}

// a handle on a bank's audio rows [n_channels][audio_channels][n_audio]
struct OnAudio : Handle {
    int n_channels = 0, audio_channels = 0;
    size_t n_audio = 0;
    size_t rows() const { return static_cast<size_t>(n_channels) * audio_channels; }
};

// a new handle of type H (an OnAudio): the common checks, then init(h) for the type's own part; what that clears on the null
// stream is clear before this returns
template <class H, class Init>
int create_on_audio(const char *who, H **out, int n_channels, int audio_channels, size_t n_audio, int device, Init init)
{
    if (!out) return fail(FMRX_EINVAL, "%s: null argument", who);
    if (n_channels < 1) return fail(FMRX_EINVAL, "%s: n_channels must be >= 1", who);
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "%s: audio_channels %d: 1 or 2", who, audio_channels);
    if (n_audio < 1 || n_audio > (size_t{1} << 26)) return fail(FMRX_EINVAL, "%s: n_audio %zu: 1 .. 2^26", who, n_audio);
    return make(out, device, [&](H *h) -> int {
        h->n_channels = n_channels;
        h->audio_channels = audio_channels;
        h->n_audio = n_audio;
        FMRX_TRY(init(h));
        FMRX_HIP(hipStreamSynchronize(nullptr));
        return FMRX_OK;
    });
}

// channel < 0: all of them.  clear(): the memsets of the type's carried state
template <class Clear>
int reset_on_audio(const char *who, OnAudio *h, int channel, Clear clear)
{
    if (!h) return fail(FMRX_EINVAL, "%s: null handle", who);
    if (channel >= h->n_channels) return fail(FMRX_EINVAL, "%s: channel %d of %d", who, channel, h->n_channels);
    FMRX_TRY(h->wait());
    FMRX_TRY(clear());
    FMRX_HIP(hipStreamSynchronize(nullptr));   // the rows are clear before this returns: a call on any stream, non-blocking ones included, finds them so
    return FMRX_OK;
}

// one status row per channel on the device -- state and result at once --, and, for the host call only, device copies of the
// host's rows
template <class Status>
struct Stage : OnAudio {
    float inv_n = 0.0f;
    DevBuf<Status> d_status;
    DevBuf<float> d_in, d_out;                // the host call only
    DevBuf<int16_t> d_pcm;
};

// what a stage's launch gets: its source of control data, the rows, the stream
template <class Source>
struct Call {
    Source src;
    const float *d_in;
    float *d_out;
    int16_t *d_pcm;
    int wrap;
    hipStream_t s;
};

constexpr size_t kSlack = 16;   // bytes in front of a device copy, so that it can take its host pointer's address modulo 16

inline int check_rows(const char *who, const float *in, const float *out, const int16_t *pcm, int pcm_policy)
{
    if (!in) return fail(FMRX_EINVAL, "%s: null input", who);
    if (!out && !pcm) return fail(FMRX_EINVAL, "%s: neither float nor PCM output", who);
    if (reinterpret_cast<uintptr_t>(in) % sizeof(float) || reinterpret_cast<uintptr_t>(out) % sizeof(float) || reinterpret_cast<uintptr_t>(pcm) % sizeof(int16_t))
        return fail(FMRX_EINVAL, "%s: float rows must be 4-byte aligned, PCM 2-byte", who);
    if (pcm_policy != FMRX_PCM_WRAP && pcm_policy != FMRX_PCM_SATURATE) return fail(FMRX_EINVAL, "%s: pcm_policy %d", who, pcm_policy);
    return FMRX_OK;
}

// a new handle of type H (a Stage): the common checks, the status rows zeroed, then init(h) for the stage's own part
template <class H, class Init>
int create(const char *who, H **out, int n_channels, int audio_channels, size_t n_audio, int device, Init init)
{
    return create_on_audio(who, out, n_channels, audio_channels, n_audio, device, [&](H *h) -> int {
        h->inv_n = static_cast<float>(1.0 / static_cast<double>(n_audio));
        FMRX_TRY(h->d_status.alloc(n_channels));
        FMRX_HIP(hipMemset(h->d_status.p, 0, h->d_status.bytes()));
        return init(h);
    });
}

// channel < 0: all of them.  extra(): what else the stage clears
template <class Status, class Extra>
int reset(const char *who, Stage<Status> *h, int channel, Extra extra)
{
    return reset_on_audio(who, h, channel, [&]() -> int {
        if (channel < 0) FMRX_HIP(hipMemset(h->d_status.p, 0, h->d_status.bytes()));
        else FMRX_HIP(hipMemset(h->d_status.p + channel, 0, sizeof(Status)));
        return extra();
    });
}

template <class Status>
int status_get(const char *who, Stage<Status> *h, Status *out)
{
    if (!h || !out) return fail(FMRX_EINVAL, "%s: null argument", who);
    FMRX_TRY(h->wait());
    FMRX_HIP(hipMemcpy(out, h->d_status.p, static_cast<size_t>(h->n_channels) * sizeof(Status), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

template <class H>
using Launch = int (*)(H *, const Call<typename H::Source> &);

template <class H>
int run(H *h, Launch<H> launch, const Call<typename H::Source> &c)
{
    FMRX_TRY(launch(h, c));
    FMRX_HIP(hipEventRecord(h->done, c.s));
    h->ran = true;
    return FMRX_OK;
}

// the device call: behind the call of the meters handle m on `stream`
template <class H, class Meters>
int process_dev(const char *who, H *h, Launch<H> launch, const Meters *m, const float *d_in, float *d_out, int16_t *d_pcm16, int pcm_policy,
                void *stream)
{
    if (!h || !m) return fail(FMRX_EINVAL, "%s: null handle", who);
    FMRX_TRY(check_rows(who, d_in, d_out, d_pcm16, pcm_policy));
    typename H::Source src;
    FMRX_TRY(H::from_handle(who, h, m, &src));
    FMRX_HIP(hipSetDevice(h->device));
    return run(h, launch, {src, d_in, d_out, d_pcm16, pcm_policy == FMRX_PCM_WRAP ? 1 : 0, static_cast<hipStream_t>(stream)});
}

// the host call: records and rows go to the device, the stage runs on the null stream, the results come back
template <class H, class Record>
int process(const char *who, H *h, Launch<H> launch, const Record *recs, const float *in, float *out, int16_t *pcm16, int pcm_policy)
{
    if (!h || !recs) return fail(FMRX_EINVAL, "%s: null argument", who);
    FMRX_TRY(check_rows(who, in, out, pcm16, pcm_policy));
    FMRX_TRY(h->wait());   // this call runs on the null stream
    typename H::Source src;
    FMRX_TRY(H::from_records(h, recs, &src));
    // the device copies: at their host pointers' addresses modulo 16 (hipMalloc's are 256-byte aligned)
    const auto at = [](auto *base, const void *host) { return reinterpret_cast<decltype(base)>(reinterpret_cast<char *>(base) + (reinterpret_cast<uintptr_t>(host) & 15)); };
    const size_t total = h->rows() * h->n_audio;
    FMRX_TRY(h->d_in.ensure(total + kSlack / sizeof(float)));
    float *d_in = at(h->d_in.p, in), *d_out = nullptr;
    int16_t *d_pcm = nullptr;
    FMRX_HIP(hipMemcpy(d_in, in, total * sizeof(float), hipMemcpyHostToDevice));
    if (out == in) d_out = d_in;
    else if (out) {
        FMRX_TRY(h->d_out.ensure(total + kSlack / sizeof(float)));
        d_out = at(h->d_out.p, out);
    }
    if (pcm16) {
        FMRX_TRY(h->d_pcm.ensure(total + kSlack / sizeof(int16_t)));
        d_pcm = at(h->d_pcm.p, pcm16);
    }
    FMRX_TRY(run(h, launch, {src, d_in, d_out, d_pcm, pcm_policy == FMRX_PCM_WRAP ? 1 : 0, nullptr}));
    FMRX_HIP(hipEventSynchronize(h->done));
    if (out) FMRX_HIP(hipMemcpy(out, d_out, total * sizeof(float), hipMemcpyDeviceToHost));
    if (pcm16) FMRX_HIP(hipMemcpy(pcm16, d_pcm, total * sizeof(int16_t), hipMemcpyDeviceToHost));
    return FMRX_OK;
}

// ---- the readers: meters of a bank's audio rows that keep their state and results field-major on the device
struct Reader : OnAudio {
    size_t n = 0;            // samples per row of the last call
    DevBuf<float> d_rows;    // the host call only
};

// a reader's launch: its kernel on rows [n_channels][audio_channels][pitch] of n samples, then the asynchronous copies of its results
template <class H>
using Read = int (*)(H *, const float *d_audio, size_t pitch, size_t n, hipStream_t s);

inline int check_read(const char *who, const Reader *h, const float *audio, size_t row_pitch, size_t n)
{
    if (!h || !audio) return fail(FMRX_EINVAL, "%s: null argument", who);
    if (n < 1 || n > h->n_audio) return fail(FMRX_EINVAL, "%s: %zu samples per row (1 .. the handle's n_audio %zu)", who, n, h->n_audio);
    if (row_pitch < n) return fail(FMRX_EINVAL, "%s: pitch of %zu floats is shorter than a row's %zu samples", who, row_pitch, n);
    return FMRX_OK;
}

// the device call, asynchronous on `stream`
template <class H>
int read_dev(const char *who, H *h, Read<H> launch, const float *d_audio, size_t row_pitch, size_t n, void *stream)
{
    FMRX_TRY(check_read(who, h, d_audio, row_pitch, n));
    FMRX_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    FMRX_TRY(launch(h, d_audio, row_pitch, n, s));
    FMRX_HIP(hipEventRecord(h->done, s));
    h->n = n;
    h->ran = true;
    return FMRX_OK;
}

// the host call: the rows go to the device, the reader runs on the null stream, collect() unpacks into `out`
template <class H, class Collect>
int read_host(const char *who, H *h, Read<H> launch, const float *audio, size_t row_pitch, size_t n, const void *out, Collect collect)
{
    FMRX_TRY(check_read(who, h, audio, row_pitch, n));
    if (!out) return fail(FMRX_EINVAL, "%s: null argument", who);
    FMRX_TRY(h->wait());   // this call runs on the null stream
    const size_t dp = (n + 3) / 4 * 4;   // the device copy's rows are 16-byte aligned
    FMRX_TRY(h->d_rows.ensure(dp * h->rows()));
    FMRX_HIP(hipMemcpy2D(h->d_rows.p, dp * sizeof(float), audio, row_pitch * sizeof(float), n * sizeof(float), h->rows(), hipMemcpyHostToDevice));
    FMRX_TRY(read_dev(who, h, launch, h->d_rows.p, dp, n, nullptr));
    return collect();
}

// field-major arrays [fields][n_channels]: all of it (channel < 0) or one channel's column cleared, on the null stream
template <class T>
int clear_fields(T *d, int fields, int n_channels, int channel)
{
    const size_t N = n_channels;
    if (channel < 0) FMRX_HIP(hipMemset(d, 0, fields * N * sizeof(T)));
    else FMRX_HIP(hipMemset2D(d + channel, N * sizeof(T), 0, sizeof(T), fields));
    return FMRX_OK;
}

template <class T>
T field(const T *a, int n_channels, int k, size_t c) { return a[static_cast<size_t>(k) * n_channels + c]; }   // field k of channel c

// what the readers' derive functions share (host only)
inline int check_derive(const char *who, const void *m, const void *out, int audio_channels, double full_scale)
{
    if (!m || !out) return fail(FMRX_EINVAL, "%s: null argument", who);
    if (audio_channels != 1 && audio_channels != 2) return fail(FMRX_EINVAL, "%s: audio_channels must be 1 or 2", who);
    if (!(full_scale > 0.0) || !std::isfinite(full_scale)) return fail(FMRX_EINVAL, "%s: full_scale %g", who, full_scale);
    return FMRX_OK;
}

inline double over_fraction(const uint64_t over[2], uint64_t n, int audio_channels)
{
    return n > 0 ? (static_cast<double>(over[0]) + static_cast<double>(over[1])) / (static_cast<double>(n) * audio_channels) : 0.0;
}

// ---- the signal meters as a stage's source: the MPX results [n_channels][kMetersMpxFields] and the segments of every channel
// (or seg_all for all of them where d_seg_each is NULL)
struct Mpx {
    const double *d_mpx;
    const unsigned long long *d_seg_each;
    unsigned long long seg_all;
};

template <class Status>
struct MpxStage : Stage<Status> {
    using Source = Mpx;
    DevBuf<double> d_mpx;                     // the host call only
    DevBuf<unsigned long long> d_segcount;

    // what the meters' last call left on the device, if it fits the stage
    static int from_handle(const char *who, const MpxStage *h, const fmrx_meters *m, Mpx *src)
    {
        const MetersMpx v = meters_mpx(m);
        if (!v.ran || v.n_if == 0) return fail(FMRX_EINVAL, "%s: the meters' last call measured no discriminator rows", who);
        if (v.n_channels != h->n_channels || v.device != h->device)
            return fail(FMRX_EINVAL, "%s: the meters have %d channels on device %d, the stage %d on %d", who, v.n_channels, v.device, h->n_channels,
                        h->device);
        *src = Mpx{v.d_mpx, nullptr, v.n_if / kMetersSegment};
        return FMRX_OK;
    }

    static int from_records(MpxStage *h, const fmrx_meter *recs, Mpx *src)
    {
        const size_t N = h->n_channels;
        std::vector<double> mpx(N * kMetersMpxFields, 0.0);
        std::vector<unsigned long long> seg(N);
        for (size_t c = 0; c < N; c++) {
            double *o = mpx.data() + c * kMetersMpxFields;
            o[0] = recs[c].sum_x;
            o[1] = recs[c].sum_x2;
            o[2] = recs[c].max_abs;
            for (int p = 0; p < kMetersProbes; p++) o[3 + p] = recs[c].probe[p];
            seg[c] = recs[c].segments;
        }
        FMRX_TRY(h->d_mpx.ensure(mpx.size()));
        FMRX_TRY(h->d_segcount.ensure(N));
        FMRX_HIP(hipMemcpy(h->d_mpx.p, mpx.data(), mpx.size() * sizeof(double), hipMemcpyHostToDevice));
        FMRX_HIP(hipMemcpy(h->d_segcount.p, seg.data(), N * sizeof(unsigned long long), hipMemcpyHostToDevice));
        *src = Mpx{h->d_mpx.p, h->d_segcount.p, 0};
        return FMRX_OK;
    }
};

// ---- the control kernel: one lane per channel loads the channel's status row, runs step(channel, row) on it -- the stage's
// control_step on what its source holds for the channel -- and stores it
constexpr int kControlThreads = 256;

template <class Status, class Step>
__device__ __forceinline__ void control_body(Status *__restrict__ st, unsigned n_channels, Step step)
{
    const unsigned i = blockIdx.x * kControlThreads + threadIdx.x;
    if (i >= n_channels) return;
    Status s = st[i];
    step(i, s);
    st[i] = s;
}

// behind Mpx: control_step (found through the control structure's namespace) on the channel's probe powers, where the meters' MPX
// pass left them
template <class Control, class Status>
__device__ __forceinline__ void control_body(const Control &c, const double *__restrict__ mpx, const unsigned long long *__restrict__ seg_each,
                                             unsigned long long seg_all, Status *__restrict__ st, unsigned n_channels)
{
    control_body(st, n_channels, [&](unsigned i, Status &s) {
        control_step(c, mpx + static_cast<size_t>(i) * kMetersMpxFields + 3, seg_each ? seg_each[i] : seg_all, s);   // behind sum_x, sum_x2, max_abs
    });
}

// kernel(args..., n_channels) on a grid of one lane per channel
template <class... Params, class... Args>
int control_launch(const char *name, void (*kernel)(Params...), int n_channels, hipStream_t s, const Args &...args)
{
    const unsigned grid = (static_cast<unsigned>(n_channels) + kControlThreads - 1) / kControlThreads;
    kernel<<<grid, kControlThreads, 0, s>>>(args..., static_cast<unsigned>(n_channels));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FMRX_EHIP, "launch %s: %s", name, hipGetErrorString(e));
    return FMRX_OK;
}

}  // namespace meter_stage
}  // namespace fmrx
