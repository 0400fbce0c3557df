// onepole_walk.hpp -- a one-pole recurrence over rows [rows][n], parallel in time and bit-identical to the serial walk: the
// bodies of the de-emphasis' and the high-cut's kernels (kernels_deemph.hip, kernels_highcut.hip).
//
// What a filter brings (DeemphFilter, HighcutFilter):
//     State                               what a walk carries from sample to sample: .y, the last output, and whatever the step
//                                         needs of the input behind it (the de-emphasis: x_prev)
//     load(state, row) -> State, store(state, row, State)     the row's carried state in memory
//     at(row) -> K                        the row's parameters, fetched once per lane
//     K::enter(y, x) -> State             a walk that enters at the sample x points to with y behind it: the input is known, so
//                                         the rest of the state is read from in front of x
//     K::step(x, k, State) -> State       sample k of the call's n
// With |pole| < 1 the recurrence is a contraction, which is what the segments rely on.
//
//   walk_segments  A lane owns one (row, segment of L samples): it starts W samples early with y = +0 and the true x_prev, or
//                  at sample 0 from the carried state where its warm-up would begin in front of the call; it remembers the y it
//                  has reached at its segment's start, writes its L outputs (f32 and PCM) and leaves its end y.  After W steps
//                  the lane's y has the true one's bits, unless the input stepped by many orders of magnitude.
//   walk_verify    one workgroup per row (64 .. 1024 lanes, by the row's segments).  Segment c is right iff the bits of its
//                  start y equal segment c-1's true end y (two NaNs count as equal: payloads are not part of a definition).
//                  With every segment's start equal to its predecessor's speculative end, all of them are true by induction
//                  from the exact segment 0: the lanes check that in parallel.  A miss is walked again by one lane from the
//                  true state, outputs and PCM rewritten, until a recomputed y has the stored one's bits -- everything behind
//                  is identical.  The row's carried state is the last segment's true end.  Misses are counted.
//   walk_serial    one lane per row walks the whole row: what the segment kernels are measured against.
// The walk is out of place: warm-up and repair read x again.
//
// Staging (walk_segments): 64 lanes per workgroup, in batches of 32 steps.  Lanes are L samples apart, so a batch is staged
// through LDS: 32 consecutive lanes of the wave read one lane's 32 consecutive floats (128 contiguous bytes per half wave; which
// row, and where that lane starts, comes from its own registers by v_readlane: an LDS lookup there cost two round trips per
// element), each lane then walks its own LDS row -- row stride 33 words, so the 64 lanes of a step hit 32 different banks twice
// (the minimum for a 64-lane ds_read_b32) -- and leaves y in place; the same mapping stores the batch, packing PCM on the way.
// Whatever of a step does not depend on y stays off the dependent chain.
#pragma once
#include "device_math.hpp"
#include "fmrx_internal.hpp"

namespace fmrx {
namespace walk {

constexpr int kLanes = 64, kBatch = 32, kStride = kBatch + 1;
constexpr int kScan = 8;           // segments every lane checks per pass
constexpr int kVerifyMax = 1024;   // lanes per row at most

__device__ __forceinline__ bool same(float a, float b) { return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b); }

// PCM of row r, sample k: [row / ac][k][row % ac] -- mono rows (ac = 1), the pipeline's interleaved stereo (2 rows, ac = 2) and
// a bank's [N][n][ac] are all this one layout: sample k of a row sits k * ac behind the row's first
__device__ __forceinline__ long pcm_row_at(long row, int n, int ac) { return (row / ac) * n * ac + row % ac; }

// the one writer: sample k of a row, f32 and PCM (pcm_row: pcm_row_at() of the row; the test is on the kernel's argument, the
// same for every lane)
__device__ __forceinline__ void write(float *y_row, int16_t *pcm, long pcm_row, int k, int ac, float v, int wrap)
{
    y_row[k] = v;
    if (pcm) pcm[pcm_row + static_cast<long>(k) * ac] = pcm_pack(v, wrap);
}

// lane (2 it + half)'s value of v: both halves of the wave ask for one lane each, so two scalar reads and a select -- no LDS
// lookup (and its latency) in the staging loops
__device__ __forceinline__ int pick(int v, int it, int half)
{
    const int a = __builtin_amdgcn_readlane(v, 2 * it), b = __builtin_amdgcn_readlane(v, 2 * it + 1);
    return half ? b : a;
}

// The three bodies: always inlined into a __global__ wrapper, whose arguments say what is __restrict__.
// seg: [2][rows][nseg], the segments' start and end y
template <class F>
__device__ __forceinline__ void walk_segments(const F &f, const float *x, long pitch_x, float *y, long pitch_y,
                                              int16_t *pcm, int ac, int wrap, long rows, int n, int nseg, int L, int W,
                                              const float *state, float *seg)
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
    const long pcm_row = pcm_row_at(row, n, ac);
    const int pcm_lo = static_cast<int>(pcm_row), pcm_hi = static_cast<int>(pcm_row >> 32);
    const int steps = W + L;
    const auto k = f.at(row);
    typename F::State st{};
    float ystart = 0.0f;
    if (ok) st = g0 <= 0 ? f.load(state, row) : k.enter(0.0f, x + row * pitch_x + g0);
    const int e = tid & (kBatch - 1), half = tid >> 5;
    for (int j0 = 0; j0 < steps; j0 += kBatch) {
        float in[kLanes / 2];   // all of the batch's loads in flight at once, then LDS
#pragma unroll
        for (int it = 0; it < kLanes / 2; it++) {
            const long r = pick(lane_row, it, half);
            const int j = j0 + e, g = pick(lane_g0, it, half) + j;
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
            ystart = j == W ? st.y : ystart;
            const typename F::State next = k.step(xs[i], g, st);
            st = act ? next : st;
            xs[i] = st.y;
        }
#pragma unroll
        for (int i = 0; i < kBatch; i++) buf[tid * kStride + i] = xs[i];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kLanes / 2; it++) {
            const long r = pick(lane_row, it, half);
            const int j = j0 + e, g = pick(lane_g0, it, half) + j;
            const long po = (static_cast<long>(pick(pcm_hi, it, half)) << 32) | static_cast<unsigned>(pick(pcm_lo, it, half));
            const float v = buf[(2 * it + half) * kStride + e];
            if (j >= W && j < steps && g >= 0 && g < n) write(y + r * pitch_y, pcm, po, g, ac, v, wrap);
        }
        __syncthreads();
    }
    if (ok) {
        seg[t] = ystart;
        seg[total + t] = st.y;
    }
}

// (y, pcm and seg are read and written here: no __restrict__ or const on the wrapper's either)
template <class F>
__device__ __forceinline__ void walk_verify(const F &f, const float *x, long pitch_x, float *y, long pitch_y, int16_t *pcm, int ac,
                                            int wrap, long rows, int n, int nseg, int L, float *state, float *seg,
                                            unsigned long long *missed)
{
    __shared__ int first, resume;
    const int tid = threadIdx.x;
    const long row = blockIdx.x;
    const float *xr = x + row * pitch_x;
    float *yr = y + row * pitch_y;
    float *start = seg + row * nseg, *end = seg + rows * nseg + row * nseg;
    const long pcm_row = pcm ? pcm_row_at(row, n, ac) : 0;   // (a division: not without PCM)
    const auto k = f.at(row);
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
            if (c < hi && !same(start[c], end[c - 1])) found = c;
        }
        if (found < nseg) atomicMin(&first, found);
        __syncthreads();
        const int fm = first;
        __syncthreads();   // (everybody has read it before lane 0 writes it again)
        if (fm >= nseg) {
            from = hi;
            continue;
        }
        if (tid == 0) {
            // everything in front of segment fm is true: walk it again from its predecessor's end, and on through the segments
            // behind it for as long as the walk does not meet the stored values
            int c = fm;
            float yv = end[c - 1];
            for (;;) {
                miss++;
                const int g_lo = c * L, g_hi = g_lo + L < n ? g_lo + L : n;
                typename F::State st = k.enter(yv, xr + g_lo);
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
                        st = k.step(xs[i], g + i, st);
                        if (same(st.y, ys[i])) met = true;
                        else write(yr, pcm, pcm_row, g + i, ac, st.y, wrap);
                    }
                }
                yv = st.y;
                c++;
                if (met || c >= nseg) {
                    if (!met) end[c - 1] = yv;
                    break;
                }
                end[c - 1] = yv;
                if (same(start[c], yv)) {   // the next segment started from exactly this: it and its end are true
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
        f.store(state, row, k.enter(end[nseg - 1], xr + n));
        if (miss) atomicAdd(missed, static_cast<unsigned long long>(miss));
    }
}

template <class F>
__device__ __forceinline__ void walk_serial(const F &f, const float *x, long pitch_x, float *y, long pitch_y,
                                            int16_t *pcm, int ac, int wrap, long rows, int n, float *state)
{
    const long row = static_cast<long>(blockIdx.x) * kLanes + threadIdx.x;
    if (row >= rows) return;
    const float *xr = x + row * pitch_x;
    float *yr = y + row * pitch_y;
    typename F::State st = f.load(state, row);
    const long pcm_row = pcm ? pcm_row_at(row, n, ac) : 0;   // (a division: not without PCM)
    const auto k = f.at(row);
    for (int g = 0; g < n; g += 8) {
        float xs[8];
#pragma unroll
        for (int i = 0; i < 8; i++) xs[i] = g + i < n ? xr[g + i] : 0.0f;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (g + i >= n) break;
            st = k.step(xs[i], g + i, st);
            write(yr, pcm, pcm_row, g + i, ac, st.y, wrap);
        }
    }
    f.store(state, row, st);
}

// ---- launch geometry: segments kernel <<<blocks, kLanes>>>, verify kernel <<<rows, verify_lanes>>>, serial kernel <<<serial_blocks(rows), kLanes>>>
struct Grid {
    long nseg = 0;
    unsigned blocks = 0, verify_lanes = 0;
    unsigned long long checked = 0;   // the segment boundaries the verify step checks
};

inline long segments(size_t n, int L) { return static_cast<long>((n + static_cast<size_t>(L) - 1) / static_cast<size_t>(L)); }
inline unsigned serial_blocks(long rows) { return static_cast<unsigned>((rows + kLanes - 1) / kLanes); }

// rows <= 2^30, n <= 2^30 (the callers' checks)
inline int grid(const char *who, long rows, size_t n, int L, Grid *g)
{
    g->nseg = segments(n, L);
    const long blocks = (rows * g->nseg + kLanes - 1) / kLanes;
    if (blocks > 0x7fffffffL) return fail(FMRX_EINVAL, "%s: too many segments", who);
    g->blocks = static_cast<unsigned>(blocks);
    const long vt = (g->nseg + kLanes - 1) / kLanes * kLanes;   // lanes per row: whole waves, enough to check a row's segments in few passes
    g->verify_lanes = static_cast<unsigned>(vt < kVerifyMax ? vt : kVerifyMax);
    g->checked = static_cast<unsigned long long>(rows) * static_cast<unsigned long long>(g->nseg - 1);
    return FMRX_OK;
}

}  // namespace walk
}  // namespace fmrx
