// kernels_deemph.hip -- the 50 / 75 us de-emphasis filter (no counterpart in the reference, which has no such stage).
//
// The definition (tests/_deemph_model.py).  Per row, state (x_prev, y_prev), both +0 at the start of a stream:
//     u = x[n] + x_prev;  v = b0 * u;  y = fmaf(p, y_prev, v);  if |y| < 2^-126: y = +0
// with p, b0 from fmrx_deemph_design.  The flush is part of the definition: without it the state of a row in digital silence
// sticks at the smallest subnormal (RN(p * 2^-149) = 2^-149) and a lane that starts from zero never meets it again.
//
// One kernel family on rows [rows][n] with a row pitch -- a pipeline has 1 or 2 rows, a bank n_channels * audio_channels:
//   deemph_segments_kernel  parallel in time.  A lane owns one (row, segment of L samples): it starts W samples early with y = +0
//                           and the true x_prev (the input is known), or at sample 0 from the carried state where its warm-up
//                           would begin in front of the call; it remembers the y it has reached at its segment's start, writes
//                           its L outputs (f32 and PCM) and leaves its end y.  p < 1 makes the recurrence a contraction: after
//                           W steps the lane's y has the true one's bits, unless the input stepped by many orders of magnitude.
//   deemph_verify_kernel    one workgroup per row (64 .. 1024 lanes, by the row's segments).  Segment c is right iff the bits of its start y equal segment c-1's true end y
//                           (two NaNs count as equal: payloads are not part of the definition).  With every segment's start equal
//                           to its predecessor's speculative end, all of them are true by induction from the exact segment 0: the
//                           lanes check that in parallel.  A miss is walked again by one lane from the true state, outputs and
//                           PCM rewritten, until a recomputed y has the stored one's bits -- everything behind is identical.  The
//                           row's carried state is the last segment's true end.  Misses are counted.
//   deemph_serial_kernel    one lane per row walks the whole row (option deemph_mode = 1, set_force_generic; what the segment
//                           kernels are measured against).
// The stage is out of place: the repair reads x again.
//
// Staging (segment kernel): 64 lanes per workgroup, in batches of 32 steps.  Lanes are L samples apart, so a batch is staged
// through LDS: 32 consecutive lanes of the wave read one lane's 32 consecutive floats (128 contiguous bytes per half wave; which
// row, and where that lane starts, comes from its own registers by v_readlane: an LDS lookup there cost two round trips per
// element), each lane then walks its own LDS row -- row stride 33 words, so the 64 lanes of a step hit 32 different banks twice (the minimum
// for a 64-lane ds_read_b32) -- and leaves y in place; the same mapping stores the batch, packing PCM on the way.  v = b0 * (x +
// x_prev) does not depend on y: only the fused multiply-add and the flush are on the dependent chain.
//
// Resources (-Rpass-analysis=kernel-resource-usage, gfx950): segments 56 VGPRs, 8 448 bytes of LDS; verify 15 VGPRs, 8 bytes; serial
// 28 VGPRs, none; no kernel uses scratch.
#include "device_math.hpp"
#include "fmrx_internal.hpp"

namespace fmrx {
namespace {

constexpr int kLanes = 64, kBatch = 32, kStride = kBatch + 1;

__device__ __forceinline__ float deemph_step(float x, float x_prev, float y_prev, float p, float b0)
{
    const float v = b0 * (x + x_prev);
    const float y = __builtin_fmaf(p, y_prev, v);
    return __builtin_fabsf(y) < 1.17549435e-38f ? 0.0f : y;
}

__device__ __forceinline__ bool deemph_same(float a, float b)
{
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}

// PCM of row r, sample k: [row / ac][k][row % ac] -- mono rows (ac = 1), the pipeline's interleaved stereo (2 rows, ac = 2) and
// a bank's [N][n][ac] are all this one layout: sample k of a row sits k * ac behind the row's first
__device__ __forceinline__ long deemph_pcm_row(long row, int n, int ac) { return (row / ac) * n * ac + row % ac; }
__device__ __forceinline__ void deemph_pcm(int16_t *pcm_row, int k, int ac, float y, int wrap)
{
    pcm_row[static_cast<long>(k) * ac] = pcm_pack(y, wrap);
}

// lane (2 it + half)'s value of v: both halves of the wave ask for one lane each, so two scalar reads and a select -- no LDS
// lookup (and its latency) in the staging loops
__device__ __forceinline__ int deemph_pick(int v, int it, int half)
{
    const int a = __builtin_amdgcn_readlane(v, 2 * it), b = __builtin_amdgcn_readlane(v, 2 * it + 1);
    return half ? b : a;
}

__global__ __launch_bounds__(kLanes) void deemph_segments_kernel(const float *__restrict__ x, long pitch_x, float *__restrict__ y,
                                                                 long pitch_y, int16_t *__restrict__ pcm, int ac, int wrap, long rows,
                                                                 int n, int nseg, int L, int W, float p, float b0,
                                                                 const float *__restrict__ state, float *__restrict__ seg)
{
    __shared__ float buf[kLanes * kStride];
    const int tid = threadIdx.x;
    const long total = rows * nseg;
    const long t = static_cast<long>(blockIdx.x) * kLanes + tid;
    const bool ok = t < total;
    const long row = ok ? t / nseg : 0;
    const int c = ok ? static_cast<int>(t - row * nseg) : 0;
    const int g0 = c * L - W;                      // where the warm-up would begin; <= 0: the lane starts at sample 0, exact
    // what the staging loops need of every lane: its row, where it starts (a lane past the end: so early that it never meets
    // sample 0), and its row's place in the PCM
    const int lane_row = static_cast<int>(row), lane_g0 = ok ? g0 : -(1 << 30);
    const long pcm_row = deemph_pcm_row(row, n, ac);
    const int pcm_lo = static_cast<int>(pcm_row), pcm_hi = static_cast<int>(pcm_row >> 32);
    const int steps = W + L;
    float yp = 0.0f, xp = 0.0f, ystart = 0.0f;
    if (ok) {
        if (g0 <= 0) {
            xp = state[2 * row];
            yp = state[2 * row + 1];
        } else {
            xp = x[row * pitch_x + g0 - 1];
        }
    }
    const int e = tid & (kBatch - 1), half = tid >> 5;
    for (int j0 = 0; j0 < steps; j0 += kBatch) {
        float in[kLanes / 2];   // all of the batch's loads in flight at once, then LDS
#pragma unroll
        for (int it = 0; it < kLanes / 2; it++) {
            const long r = deemph_pick(lane_row, it, half);
            const int j = j0 + e, g = deemph_pick(lane_g0, it, half) + j;
            in[it] = 0.0f;
            if (j < steps && g >= 0 && g < n) in[it] = x[r * pitch_x + g];
        }
#pragma unroll
        for (int it = 0; it < kLanes / 2; it++) buf[(2 * it + half) * kStride + e] = in[it];
        __syncthreads();
        float xs[kBatch];   // the lane's row in registers: the LDS latency stays off the dependent chain
#pragma unroll
        for (int i = 0; i < kBatch; i++) xs[i] = buf[tid * kStride + i];
#pragma unroll
        for (int i = 0; i < kBatch; i++) {
            const int j = j0 + i, g = g0 + j;
            const bool act = ok && j < steps && g >= 0 && g < n;
            ystart = j == W ? yp : ystart;
            const float yv = deemph_step(xs[i], xp, yp, p, b0);
            yp = act ? yv : yp;
            xp = act ? xs[i] : xp;
            xs[i] = yp;
        }
#pragma unroll
        for (int i = 0; i < kBatch; i++) buf[tid * kStride + i] = xs[i];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kLanes / 2; it++) {
            const long r = deemph_pick(lane_row, it, half);
            const int j = j0 + e, g = deemph_pick(lane_g0, it, half) + j;
            const long po = (static_cast<long>(deemph_pick(pcm_hi, it, half)) << 32) | static_cast<unsigned>(deemph_pick(pcm_lo, it, half));
            const float v = buf[(2 * it + half) * kStride + e];
            if (j >= W && j < steps && g >= 0 && g < n) {
                y[r * pitch_y + g] = v;
                if (pcm) deemph_pcm(pcm + po, g, ac, v, wrap);
            }
        }
        __syncthreads();
    }
    if (ok) {
        seg[t] = ystart;
        seg[total + t] = yp;
    }
}

constexpr int kScan = 8;      // segments every lane checks per pass
constexpr int kVerifyMax = 1024;   // lanes per row at most

// (seg is read and written here: no __restrict__, no const)
__global__ __launch_bounds__(kVerifyMax) void deemph_verify_kernel(const float *__restrict__ x, long pitch_x, float *y, long pitch_y,
                                                               int16_t *pcm, int ac, int wrap, long rows, int n, int nseg, int L,
                                                               float p, float b0, float *__restrict__ state, float *seg,
                                                               unsigned long long *missed)
{
    __shared__ int first, resume;
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const float *xr = x + row * pitch_x;
    float *yr = y + row * pitch_y;
    float *start = seg + row * nseg, *end = seg + rows * nseg + row * nseg;
    int16_t *pcm_row = pcm ? pcm + deemph_pcm_row(row, n, ac) : nullptr;
    unsigned miss = 0;
    int from = 1;
    while (from < nseg) {
        const int nt = blockDim.x;
        const int hi = from + kScan * nt < nseg ? from + kScan * nt : nseg;
        if (tid == 0) first = nseg;
        __syncthreads();
        int found = nseg;
#pragma unroll
        for (int u = kScan - 1; u >= 0; u--) {   // (no early exit: the loads of a pass are independent)
            const int c = from + u * nt + tid;
            if (c < hi && !deemph_same(start[c], end[c - 1])) found = c;
        }
        if (found < nseg) atomicMin(&first, found);
        __syncthreads();
        const int f = first;
        __syncthreads();   // (everybody has read it before lane 0 writes it again)
        if (f >= nseg) {
            from = hi;
            continue;
        }
        if (tid == 0) {
            // everything in front of segment f is true: walk f again from its predecessor's end, and on through the segments
            // behind it for as long as the walk does not meet the stored values
            int c = f;
            float yv = end[c - 1];
            for (;;) {
                miss++;
                const int g_lo = c * L, g_hi = g_lo + L < n ? g_lo + L : n;
                float xp = xr[g_lo - 1];
                bool met = false;
                for (int g = g_lo; g < g_hi && !met; g += 8) {
                    float xs[8], ys[8];   // eight samples' loads in flight at once: the walk itself is a dependent chain
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        xs[i] = g + i < g_hi ? xr[g + i] : 0.0f;
                        ys[i] = g + i < g_hi ? yr[g + i] : 0.0f;
                    }
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        if (met || g + i >= g_hi) break;
                        yv = deemph_step(xs[i], xp, yv, p, b0);
                        xp = xs[i];
                        if (deemph_same(yv, ys[i])) {
                            met = true;
                        } else {
                            yr[g + i] = yv;
                            if (pcm_row) deemph_pcm(pcm_row, g + i, ac, yv, wrap);
                        }
                    }
                }
                c++;
                if (met || c >= nseg) {
                    if (!met) end[c - 1] = yv;
                    break;
                }
                end[c - 1] = yv;
                if (deemph_same(start[c], yv)) {   // the next segment started from exactly this: it and its end are true
                    c++;
                    break;
                }
            }
            resume = c;
        }
        __syncthreads();
        from = resume;
    }
    if (tid == 0) {
        state[2 * row] = xr[n - 1];
        state[2 * row + 1] = end[nseg - 1];
        if (miss) atomicAdd(missed, static_cast<unsigned long long>(miss));
    }
}

__global__ __launch_bounds__(kLanes) void deemph_serial_kernel(const float *__restrict__ x, long pitch_x, float *__restrict__ y,
                                                               long pitch_y, int16_t *__restrict__ pcm, int ac, int wrap, long rows,
                                                               int n, float p, float b0, float *__restrict__ state)
{
    const long row = static_cast<long>(blockIdx.x) * kLanes + threadIdx.x;
    if (row >= rows) return;
    const float *xr = x + row * pitch_x;
    float *yr = y + row * pitch_y;
    float xp = state[2 * row], yp = state[2 * row + 1];
    int16_t *pcm_row = pcm ? pcm + deemph_pcm_row(row, n, ac) : nullptr;
    for (int g = 0; g < n; g += 8) {
        float xs[8];
#pragma unroll
        for (int i = 0; i < 8; i++) xs[i] = g + i < n ? xr[g + i] : 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (g + i >= n) break;
            yp = deemph_step(xs[i], xp, yp, p, b0);
            xp = xs[i];
            yr[g + i] = yp;
            if (pcm_row) deemph_pcm(pcm_row, g + i, ac, yp, wrap);
        }
    }
    state[2 * row] = xp;
    state[2 * row + 1] = yp;
}

}  // namespace

DeemphShape deemph_shape(const Options &o, size_t n)
{
    DeemphShape s;
    s.L = o.deemph_segment < 0 ? kDeemphSegment : o.deemph_segment;
    s.W = o.deemph_warmup < 0 ? kDeemphWarmup : o.deemph_warmup;
    s.nseg = static_cast<long>((n + s.L - 1) / s.L);
    return s;
}

size_t deemph_scratch_floats(size_t rows, size_t n, const Options &o) { return 2 * rows * static_cast<size_t>(deemph_shape(o, n).nseg) + 2; }

int deemph_launch(const DeemphArgs &a, const Options &o, bool serial, hipStream_t s, unsigned long long *segments)
{
    if (a.rows == 0 || a.n == 0) return FMRX_OK;
    if (!a.x || !a.y || !a.state) return fail(FMRX_EINVAL, "deemph: null buffer");
    if (a.x == a.y) return fail(FMRX_EINVAL, "deemph: the stage is out of place (the repair reads x again)");
    if (a.n > (static_cast<size_t>(1) << 30) || a.rows > (static_cast<size_t>(1) << 30))
        return fail(FMRX_EINVAL, "deemph: at most 2^30 samples per row and 2^30 rows");
    if (a.pitch_x < static_cast<long>(a.n) || a.pitch_y < static_cast<long>(a.n)) return fail(FMRX_EINVAL, "deemph: pitch smaller than n");
    if (a.ac < 1 || a.rows % a.ac) return fail(FMRX_EINVAL, "deemph: rows %zu are not whole groups of %d PCM channels", a.rows, a.ac);
    const long rows = static_cast<long>(a.rows);
    const int n = static_cast<int>(a.n);
    if (serial || o.deemph_mode == 1) {
        hipLaunchKernelGGL(deemph_serial_kernel, dim3(static_cast<unsigned>((rows + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, a.x, a.pitch_x,
                           a.y, a.pitch_y, a.pcm, a.ac, a.wrap, rows, n, a.p, a.b0, a.state);
        FMRX_LAUNCH_CHECK("deemph_serial_kernel");
        return FMRX_OK;
    }
    const DeemphShape sh = deemph_shape(o, a.n);
    if (!a.seg || !a.missed) return fail(FMRX_EINVAL, "deemph: null scratch");
    const long total = rows * sh.nseg;
    if (sh.nseg > (1L << 30) || (total + kLanes - 1) / kLanes > 0x7fffffffL) return fail(FMRX_EINVAL, "deemph: too many segments");
    hipLaunchKernelGGL(deemph_segments_kernel, dim3(static_cast<unsigned>((total + kLanes - 1) / kLanes)), dim3(kLanes), 0, s, a.x, a.pitch_x,
                       a.y, a.pitch_y, a.pcm, a.ac, a.wrap, rows, n, static_cast<int>(sh.nseg), sh.L, sh.W, a.p, a.b0, a.state, a.seg);
    FMRX_LAUNCH_CHECK("deemph_segments_kernel");
    // lanes per row: enough to check a row's segments in few passes, whole waves
    const long vt = (sh.nseg + kLanes - 1) / kLanes * kLanes;
    hipLaunchKernelGGL(deemph_verify_kernel, dim3(static_cast<unsigned>(rows)), dim3(static_cast<unsigned>(vt < kVerifyMax ? vt : kVerifyMax)), 0, s, a.x, a.pitch_x, a.y, a.pitch_y, a.pcm,
                       a.ac, a.wrap, rows, n, static_cast<int>(sh.nseg), sh.L, a.p, a.b0, a.state, a.seg, a.missed);
    FMRX_LAUNCH_CHECK("deemph_verify_kernel");
    if (segments) *segments += static_cast<unsigned long long>(rows) * static_cast<unsigned long long>(sh.nseg - 1);
    return FMRX_OK;
}

// ---- a handle's de-emphasis: coefficients, carried state, scratch, counters ----
int Deemph::set(double fs, double tau_us_, size_t rows_, size_t n_max_, const Options &o)
{
    if (!(tau_us_ >= 0.0)) return fail(FMRX_EINVAL, "set_deemphasis: tau must be positive, or 0 for off");
    if (on && tau_us_ == tau_us) return FMRX_OK;
    FMRX_HIP(hipDeviceSynchronize());   // nothing in flight sees the change under it
    if (tau_us_ == 0.0) {
        on = false;
        tau_us = 0.0;
        return FMRX_OK;
    }
    float p_, b0_;
    FMRX_TRY(fmrx_deemph_design(fs, tau_us_, &p_, &b0_));
    rows = rows_;
    n_max = n_max_;
    FMRX_TRY(in.ensure(rows * n_max));
    FMRX_TRY(state.ensure(2 * rows));
    FMRX_TRY(seg.ensure(deemph_scratch_floats(rows, n_max, o)));
    FMRX_TRY(counter.ensure(1));
    if (!counted) FMRX_HIP(hipMemset(counter.p, 0, sizeof(unsigned long long)));
    counted = true;
    FMRX_HIP(hipMemset(state.p, 0, 2 * rows * sizeof(float)));
    FMRX_HIP(hipDeviceSynchronize());
    p = p_;
    b0 = b0_;
    tau_us = tau_us_;
    on = true;
    return FMRX_OK;
}

int Deemph::reset(long first_row, long n_rows, hipStream_t s)
{
    if (!state.p) return FMRX_OK;
    FMRX_HIP(hipMemsetAsync(state.p + 2 * first_row, 0, 2 * n_rows * sizeof(float), s));
    return FMRX_OK;
}

int Deemph::run(size_t n, float *d_f32, int16_t *d_pcm, int ac, int wrap, const Options &o, bool serial, hipStream_t s)
{
    if (n > n_max) return fail(FMRX_EINVAL, "deemph: %zu samples per row exceed the %zu the handle was sized for", n, n_max);
    FMRX_TRY(seg.ensure(deemph_scratch_floats(rows, n, o)));   // (grows only when the options' shape changes: a wait, not per call)
    if (!d_f32) FMRX_TRY(out.ensure(rows * n_max));            // (the first call that takes PCM only)
    DeemphArgs a;
    a.x = in.p;
    a.pitch_x = a.pitch_y = static_cast<long>(n);
    a.y = d_f32 ? d_f32 : out.p;
    a.pcm = d_pcm;
    a.ac = ac;
    a.wrap = wrap;
    a.rows = rows;
    a.n = n;
    a.p = p;
    a.b0 = b0;
    a.state = state.p;
    a.seg = seg.p;
    a.missed = counter.p;
    return deemph_launch(a, o, serial, s, &segments);
}

int Deemph::diagnostics(unsigned long long *segments_, unsigned long long *missed_)
{
    FMRX_HIP(hipDeviceSynchronize());
    if (segments_) *segments_ = segments;
    if (missed_) {
        *missed_ = 0;
        if (counter.p) FMRX_HIP(hipMemcpy(missed_, counter.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
    }
    return FMRX_OK;
}

}  // namespace fmrx
