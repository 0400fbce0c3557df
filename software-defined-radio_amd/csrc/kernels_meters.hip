// kernels_meters.hip -- the signal meters' two passes (include/fmrx.h: fmrx_meters_*; defined by
// tests/_meters_model.py).
//
// RF pass (meters_rf_kernel): a channel's u8 I,Q bytes -> sum i, sum q, sum p, sum p^2 (p = i^2 + q^2) and the count of bytes
// 0 / 255, all integers.  The channel rides in the grid's x (banks have more than 65 535 receivers), a piece of the row in
// its y.  A lane reads 16 bytes = 8 complex samples per step; p fits 16 bits, a piece's sums fit 32 bits except sum p^2,
// which is added in 64 bits two samples at a time (rf_dword).  The five sums are reduced across the wave with shuffles, across the workgroup's four
// waves through LDS, and leave as ONE 64-bit integer atomic per field and workgroup: integer adds are exact in any order, so
// the results are the model's integers whatever the schedule.  A row of any alignment: the bytes in front of the first
// 16-byte boundary and behind the last whole piece are walked sample by sample by the row's first workgroup; a row at an odd
// address (an I,Q pair would straddle every piece) is walked that way as a whole.
//
// MPX pass (meters_mpx_kernel): a channel's float32 discriminator row -> sum x, sum x^2, max |x| and the five Hann-windowed
// tone powers, in float64 in a FIXED order (no floating-point atomics: the same row gives the same bytes).  One workgroup of
// 256 threads walks whole channels (blockIdx.x, blockIdx.x + gridDim.x, ...; the grid is capped at a few workgroups per CU),
// so the table is read once per workgroup, not once per channel.  Thread t owns samples 4 t .. 4 t + 3 of every 1024-sample
// segment: one 16-byte load per segment where the row is 16-byte aligned, four 4-byte loads otherwise -- the same samples and
// the same order of additions either way -- and keeps its 4 x 5 complex table entries in registers (40 doubles).  Per
// segment: 5 complex partial sums of 4 fused multiply-adds each, reduced across the wave with shuffles (wave_sum10: all ten
// sums in 13 exchanges) into LDS; after every 16 segments one barrier, and threads 0 .. 4 add wave 0 + 1 + 2 + 3 and then
// |c_p|^2 to their probe's running sum in segment order.  (A barrier waits for every load in flight, so one per segment
// would undo the loads issued two segments ahead.)  sum x, sum x^2 and max |x| ride along in the same loads, take the samples
// past the last whole segment at the end, and are reduced once per channel, lane by lane and then wave by wave.
#include "fmrx_internal.hpp"

namespace fmrx {
namespace {

using u4 = unsigned __attribute__((ext_vector_type(4)));
using f4 = float __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256, kWaves = kThreads / 64;

struct RfSums {
    long long si = 0, sq = 0;
    unsigned long long m2 = 0, m4 = 0, cl = 0;
};

__device__ __forceinline__ void rf_sample(unsigned I, unsigned Q, int &si, int &sq, unsigned &m2, unsigned long long &m4, unsigned &cl)
{
    const int i = static_cast<int>(I) - 128, q = static_cast<int>(Q) - 128;
    const unsigned p = static_cast<unsigned>(i * i + q * q);   // <= 2^15
    si += i;
    sq += q;
    m2 += p;
    m4 += static_cast<unsigned long long>(p) * p;
    cl += (I == 0u) + (I == 255u) + (Q == 0u) + (Q == 255u);
}

// The same for one dword = two samples (I0, Q0, I1, Q1), in full-rate instructions: XOR 0x80 turns the bytes into the int8 i, q;
// 4 x int8 dot products give p0 + p1, p0 alone (the other half masked), sum i and sum q; p^2 <= 2^30 is a 24-bit multiply; a
// byte is 0 or 255 where (byte + 1) mod 256 has no bit above bit 0, counted for the four bytes at once.
__device__ __forceinline__ void rf_dword(unsigned w, int &si, int &sq, unsigned &m2, unsigned long long &m4, unsigned &cl)
{
    const int s = static_cast<int>(w ^ 0x80808080u);
    const unsigned pp = static_cast<unsigned>(__builtin_amdgcn_sdot4(s, s, 0, false));
    const unsigned p0 = static_cast<unsigned>(__builtin_amdgcn_sdot4(s, s & 0x0000ffff, 0, false)), p1 = pp - p0;
    si = __builtin_amdgcn_sdot4(s, 0x00010001, si, false);
    sq = __builtin_amdgcn_sdot4(s, 0x01000100, sq, false);
    m2 += pp;
    m4 += __umul24(p0, p0) + __umul24(p1, p1);   // <= 2^31
    const unsigned c = (((w & 0x7f7f7f7fu) + 0x01010101u) ^ (w & 0x80808080u)) & 0xfefefefeu;   // per byte: (byte + 1) & 0xfe
    const unsigned z = ~(((c & 0x7f7f7f7fu) + 0x7f7f7f7fu) | c) & 0x80808080u;                  // 0x80 in every byte of c that is 0
    cl += static_cast<unsigned>(__builtin_popcount(z));
}

__global__ __launch_bounds__(kThreads) void meters_rf_kernel(const uint8_t *__restrict__ iq, size_t pitch, size_t n_bytes,
                                                             unsigned pieces_per_thread, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long part[kWaves][kMetersRfFields];
    const size_t c = blockIdx.x;
    const uint8_t *row = iq + c * pitch;
    const uintptr_t a = reinterpret_cast<uintptr_t>(row);
    const size_t to_16 = static_cast<size_t>((0 - a) & 15);
    const size_t head = (a & 1) ? n_bytes : (to_16 < n_bytes ? to_16 : n_bytes);   // even: a and n_bytes are
    const size_t nvec = (n_bytes - head) / 16;
    const size_t tail = head + 16 * nvec;
    const size_t first = static_cast<size_t>(blockIdx.y) * pieces_per_thread * kThreads;
    if (blockIdx.y > 0 && first >= nvec) return;   // the whole workgroup: the grid is sized for a row without a head
    RfSums t;
    const u4 *v = reinterpret_cast<const u4 *>(row + head);
    for (unsigned j = 0; j < pieces_per_thread; j++) {
        const size_t k = first + static_cast<size_t>(j) * kThreads + threadIdx.x;
        if (k >= nvec) break;
        const u4 w = v[k];
        int si = 0, sq = 0;
        unsigned m2 = 0, cl = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) rf_dword(w[d], si, sq, m2, t.m4, cl);
        t.si += si;
        t.sq += sq;
        t.m2 += m2;
        t.cl += cl;
    }
    if (blockIdx.y == 0) {
        const size_t nh = head / 2, nt = (n_bytes - tail) / 2;
        for (size_t s = threadIdx.x; s < nh + nt; s += kThreads) {
            const size_t off = s < nh ? 2 * s : tail + 2 * (s - nh);
            int si = 0, sq = 0;
            unsigned m2 = 0, cl = 0;
            rf_sample(row[off], row[off + 1], si, sq, m2, t.m4, cl);
            t.si += si;
            t.sq += sq;
            t.m2 += m2;
            t.cl += cl;
        }
    }
    unsigned long long f[kMetersRfFields] = {static_cast<unsigned long long>(t.si), static_cast<unsigned long long>(t.sq), t.m2, t.m4, t.cl};
#pragma unroll
    for (int i = 0; i < kMetersRfFields; i++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) f[i] += __shfl_down(f[i], o, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kMetersRfFields; i++) part[wave][i] = f[i];
    }
    __syncthreads();
    if (threadIdx.x < kMetersRfFields) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) s += part[w][threadIdx.x];
        atomicAdd(acc + c * kMetersRfFields + threadIdx.x, s);   // two's complement: the signed sums add the same way
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;   // lane 0 holds the sum
}

// The ten per-lane partial sums a[0 .. 10) of a segment -> their ten wave totals in 13 exchanges instead of 60: at every step a
// lane keeps half of the values it holds, adds its partner's partial sums of those and hands over the other half (xor 32: values
// 0-4 stay in lanes 0-31, 5-9 in 32-63; xor 16: three stay, two go; xor 8: two and one; xor 4: one and one; xor 2 and 1: plain).
// Lane 32 b5 + {0, 4, 8, 16, 20} ends with the total of value 5 b5 + {0, 1, 2, 3, 4}; the order of the additions is fixed.
__device__ __forceinline__ double wave_sum10(const double (&a)[10], int lane, int &index, bool &holds)
{
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8, h2 = lane & 4;
    double b[5], c[3], d[2];
#pragma unroll
    for (int j = 0; j < 5; j++) b[j] = (h5 ? a[5 + j] : a[j]) + __shfl_xor(h5 ? a[j] : a[5 + j], 32, 64);
    c[0] = (h4 ? b[3] : b[0]) + __shfl_xor(h4 ? b[0] : b[3], 16, 64);
    c[1] = (h4 ? b[4] : b[1]) + __shfl_xor(h4 ? b[1] : b[4], 16, 64);
    c[2] = b[2] + __shfl_xor(h4 ? b[2] : 0.0, 16, 64);                  // lanes with h4: not a value
    d[0] = (h3 ? c[2] : c[0]) + __shfl_xor(h3 ? c[0] : c[2], 8, 64);
    d[1] = c[1] + __shfl_xor(h3 ? c[1] : 0.0, 8, 64);                   // lanes with h3: not a value
    double e = (h2 ? d[1] : d[0]) + __shfl_xor(h2 ? d[0] : d[1], 4, 64);
    e += __shfl_xor(e, 2, 64);
    e += __shfl_xor(e, 1, 64);
    const int m = h2 ? 1 : 0, k = h3 ? 2 : m, j = h4 ? 3 + k : k;
    holds = (lane & 3) == 0 && !(h3 && h2) && !(h4 && h3);
    index = (h5 ? 5 : 0) + j;
    return e;
}

__device__ __forceinline__ f4 load_row4(const float *p, bool vec)
{
    if (vec) return *reinterpret_cast<const f4 *>(p);
    return f4{p[0], p[1], p[2], p[3]};
}

__global__ __launch_bounds__(kThreads) void meters_mpx_kernel(const float *__restrict__ x, size_t pitch, size_t n_if, unsigned n_channels,
                                                              const double *__restrict__ table, double *__restrict__ out)
{
    constexpr int P = kMetersProbes, L = kMetersSegment;
    constexpr int B = 16;   // segments per barrier
    __shared__ double seg_part[2][B][kWaves][2 * P];
    __shared__ double row_part[kWaves][3];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double tr[P][4], ti[P][4];
#pragma unroll
    for (int p = 0; p < P; p++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            tr[p][j] = table[p * L + 4 * t + j];
            ti[p][j] = table[(P + p) * L + 4 * t + j];
        }
    const size_t M = n_if / L;
    for (size_t c = blockIdx.x; c < n_channels; c += gridDim.x) {
        const float *row = x + c * pitch;
        const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;   // the same for the whole workgroup
        double sx = 0.0, sx2 = 0.0, mx = 0.0, probe = 0.0;
        f4 v0 = load_row4(row + 4 * t, vec), v1 = v0;   // M >= 1
        if (M > 1) v1 = load_row4(row + L + 4 * t, vec);
        for (size_t s0 = 0; s0 < M; s0 += B) {
            const int nb = static_cast<int>(M - s0 < B ? M - s0 : B);
            // two buffers by batch parity: a thread that writes batch n + 2 has passed the barrier of batch n + 1, which threads
            // 0 .. 4 reach only after they have read batch n
            double(*buf)[kWaves][2 * P] = seg_part[(s0 / B) & 1];
            for (int b = 0; b < nb; b++) {
                f4 v2 = v1;
                if (s0 + b + 2 < M) v2 = load_row4(row + (s0 + b + 2) * L + 4 * t, vec);   // two segments ahead of the arithmetic
                double a[2 * P];
#pragma unroll
                for (int p = 0; p < 2 * P; p++) a[p] = 0.0;
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double d = static_cast<double>(v0[j]);
                    sx += d;
                    sx2 = fma(d, d, sx2);
                    mx = fmax(mx, fabs(d));
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        a[p] = fma(d, tr[p][j], a[p]);
                        a[P + p] = fma(d, ti[p][j], a[P + p]);
                    }
                }
                int index;
                bool holds;
                const double total = wave_sum10(a, lane, index, holds);
                if (holds) buf[b][wave][index] = total;
                v0 = v1;
                v1 = v2;
            }
            __syncthreads();
            if (t < P)
                for (int b = 0; b < nb; b++) {
                    const double re = ((buf[b][0][t] + buf[b][1][t]) + buf[b][2][t]) + buf[b][3][t];
                    const double im = ((buf[b][0][P + t] + buf[b][1][P + t]) + buf[b][2][P + t]) + buf[b][3][P + t];
                    probe += re * re + im * im;
                }
        }
        for (size_t k = M * L + t; k < n_if; k += kThreads) {
            const double d = static_cast<double>(row[k]);
            sx += d;
            sx2 = fma(d, d, sx2);
            mx = fmax(mx, fabs(d));
        }
        sx = wave_sum(sx);
        sx2 = wave_sum(sx2);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_down(mx, o, 64));
        if (lane == 0) {
            row_part[wave][0] = sx;
            row_part[wave][1] = sx2;
            row_part[wave][2] = mx;
        }
        __syncthreads();
        double *o = out + c * kMetersMpxFields;
        if (t < 2) o[t] = ((row_part[0][t] + row_part[1][t]) + row_part[2][t]) + row_part[3][t];
        if (t == 2) o[2] = fmax(fmax(row_part[0][2], row_part[1][2]), fmax(row_part[2][2], row_part[3][2]));
        if (t < P) o[3 + t] = probe;
        __syncthreads();   // row_part and seg_part are free for the next channel
    }
}

}  // namespace

int meters_rf_launch(const uint8_t *d_iq, size_t pitch, size_t n_bytes, int n_channels, unsigned long long *d_acc, hipStream_t s)
{
    // 4 pieces of 16 bytes per thread = 16 KiB of a row per workgroup; longer where the grid's y would pass 65 535
    size_t per_thread = 4;
    const size_t pieces = n_bytes / 16;
    auto blocks = [&] { return (pieces + per_thread * kThreads - 1) / (per_thread * kThreads); };
    while (blocks() > 65535) per_thread *= 2;
    const dim3 grid(static_cast<unsigned>(n_channels), static_cast<unsigned>(blocks() ? blocks() : 1));
    meters_rf_kernel<<<grid, kThreads, 0, s>>>(d_iq, pitch, n_bytes, static_cast<unsigned>(per_thread), d_acc);
    FMRX_LAUNCH_CHECK("meters_rf_kernel");
    return FMRX_OK;
}

int meters_mpx_launch(const float *d_x, size_t pitch, size_t n_if, int n_channels, const double *d_table, double *d_out, int max_blocks,
                      hipStream_t s)
{
    const int grid = n_channels < max_blocks ? n_channels : max_blocks;
    meters_mpx_kernel<<<grid, kThreads, 0, s>>>(d_x, pitch, n_if, static_cast<unsigned>(n_channels), d_table, d_out);
    FMRX_LAUNCH_CHECK("meters_mpx_kernel");
    return FMRX_OK;
}

}  // namespace fmrx
