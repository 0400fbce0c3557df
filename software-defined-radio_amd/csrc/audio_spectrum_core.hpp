// audio_spectrum_core.hpp -- the tables and the frame arithmetic of the audio spectrum meter (include/fmrx.h:
// fmrx_audio_spectrum_*; defined by tests/_audio_spectrum_model.py).  The host function
// fmrx_audio_spectrum_walk (audio_spectrum.hip) and the kernel (kernels_audio_spectrum.hip) share the tables, the window multiply,
// the bin power and the band sum; the 2 x 128 chains of a frame are fmaf on the host and v_mfma_f32_16x16x4_f32 on the device,
// which is the same chain (tests/_fir_model.py from MFMA_K_ORDER on).
//
// A frame is 256 samples.  xw[j] = x[j] w[j]; for bins k = 0 .. 127, re_k = the fmaf chain over j ascending from +0 of
// C[(k j) mod 256] xw[j], im_k the same with C[(k j - 64) mod 256]; p_k = fmaf(im_k, im_k, fl(re_k re_k)); a band is the float32
// sum of its bins ascending from +0.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FMRX_AS_HD __host__ __device__ __forceinline__
#else
#define FMRX_AS_HD inline
#endif

namespace fmrx {
namespace audio_spectrum {

constexpr int kFrame = 256;      // samples of a frame
constexpr int kBins = 128;       // bins 0 .. 127; bin 0 belongs to no band
constexpr int kTile = 16;        // frames whose float64 sum is formed first: the columns of one matrix instruction
constexpr int kMaxBands = 32;
constexpr int kDefaultBands = 23;
constexpr int kDefaultEdges[kDefaultBands + 1] = {1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 128};

// float32 of cos(2 pi m / 256), m = 0 .. 64, made in float64 and rounded once, C[64] = +0: these literals are the definition
#define FMRX_AS_COS_QUARTER                                                                                                          \
    1.0f, 0.999698818f, 0.99879545f, 0.997290432f, 0.99518472f, 0.992479563f, 0.989176512f, 0.985277653f, 0.980785251f, 0.975702107f, \
        0.970031261f, 0.963776052f, 0.956940353f, 0.949528158f, 0.941544056f, 0.932992816f, 0.923879504f, 0.914209783f, 0.903989315f, \
        0.893224299f, 0.881921291f, 0.870086968f, 0.857728601f, 0.84485358f, 0.831469595f, 0.817584813f, 0.803207517f, 0.78834641f,   \
        0.773010433f, 0.757208824f, 0.740951121f, 0.724247098f, 0.707106769f, 0.689540565f, 0.671558976f, 0.653172851f, 0.634393275f, \
        0.615231574f, 0.59569931f, 0.575808167f, 0.555570245f, 0.534997642f, 0.514102757f, 0.492898196f, 0.471396744f, 0.449611336f,  \
        0.427555084f, 0.405241311f, 0.382683426f, 0.359895051f, 0.336889863f, 0.313681751f, 0.290284663f, 0.266712755f, 0.242980182f, \
        0.219101235f, 0.195090324f, 0.170961887f, 0.146730468f, 0.122410677f, 0.0980171412f, 0.0735645667f, 0.0490676761f,            \
        0.024541229f, 0.0f
// float32 of 0.5 - 0.5 cos(2 pi j / 256), j = 0 .. 128, the periodic Hann window's first half and its middle
#define FMRX_AS_WINDOW_HALF                                                                                                          \
    0.0f, 0.000150590655f, 0.000602271874f, 0.00135477167f, 0.00240763673f, 0.00376023259f, 0.00541174505f, 0.00736117875f,          \
        0.00960735977f, 0.0121489353f, 0.014984373f, 0.0181119666f, 0.0215298329f, 0.02523591f, 0.0292279683f, 0.0335035995f,         \
        0.038060233f, 0.0428951234f, 0.0480053537f, 0.0533878505f, 0.0590393692f, 0.0649565011f, 0.0711356923f, 0.0775732175f,        \
        0.0842651948f, 0.0912075937f, 0.0983962342f, 0.105826788f, 0.113494776f, 0.12139558f, 0.12952444f, 0.137876466f,              \
        0.146446615f, 0.155229732f, 0.164220527f, 0.173413575f, 0.182803363f, 0.192384198f, 0.202150345f, 0.212095901f,               \
        0.222214878f, 0.232501194f, 0.242948622f, 0.253550917f, 0.264301628f, 0.275194347f, 0.286222458f, 0.297379345f,               \
        0.308658272f, 0.320052475f, 0.331555068f, 0.343159139f, 0.354857653f, 0.366643608f, 0.378509909f, 0.390449375f,               \
        0.402454853f, 0.414519042f, 0.426634759f, 0.438794672f, 0.450991422f, 0.463217705f, 0.475466162f, 0.4877294f, 0.5f,           \
        0.512270629f, 0.524533808f, 0.536782265f, 0.549008548f, 0.561205328f, 0.573365211f, 0.585480928f, 0.597545147f,               \
        0.609550595f, 0.621490061f, 0.633356392f, 0.645142317f, 0.656840861f, 0.668444932f, 0.679947495f, 0.691341698f,               \
        0.702620685f, 0.713777542f, 0.724805653f, 0.735698342f, 0.746449113f, 0.757051349f, 0.767498791f, 0.777785122f,               \
        0.787904084f, 0.797849655f, 0.807615817f, 0.817196667f, 0.826586425f, 0.835779488f, 0.844770253f, 0.853553414f,               \
        0.862123549f, 0.87047559f, 0.878604412f, 0.886505246f, 0.894173205f, 0.901603758f, 0.908792436f, 0.915734828f,                \
        0.92242676f, 0.9288643f, 0.935043514f, 0.940960646f, 0.946612179f, 0.951994658f, 0.957104862f, 0.961939752f, 0.966496408f,    \
        0.970772028f, 0.974764109f, 0.978470147f, 0.981888056f, 0.985015631f, 0.987851083f, 0.990392625f, 0.992638826f,               \
        0.994588256f, 0.996239781f, 0.99759239f, 0.998645246f, 0.999397755f, 0.999849439f, 1.0f

// w[256] and C[256], unfolded by symmetry: C[128 - m] = -C[m], C[256 - m] = C[m], C[64] = C[192] = +0; w[256 - j] = w[j]
struct Tables {
    float w[kFrame], c[kFrame];
};

constexpr Tables make_tables()
{
    constexpr float q[65] = {FMRX_AS_COS_QUARTER}, h[129] = {FMRX_AS_WINDOW_HALF};
    Tables t{};
    for (int m = 0; m <= 64; m++) {
        t.c[m] = q[m];
        t.c[128 - m] = -q[m];
    }
    t.c[64] = 0.0f;
    for (int m = 1; m < 128; m++) t.c[256 - m] = t.c[m];
    for (int j = 0; j <= 128; j++) t.w[j] = h[j];
    for (int j = 1; j < 128; j++) t.w[256 - j] = h[j];
    return t;
}

// p_k of one bin: the product re re is rounded on its own
FMRX_AS_HD float bin_power(float re, float im)
{
    const float rr = re * re;
    return fmaf(im, im, rr);
}

// a band of one frame: p[lo .. hi - 1] summed ascending from +0
FMRX_AS_HD float band_sum(const float *p, int lo, int hi)
{
    float acc = 0.0f;
    for (int k = lo; k < hi; k++) acc = acc + p[k];
    return acc;
}

// edges[0 .. n_bands]: strictly ascending within 1 .. 128, 1 <= n_bands <= 32
inline bool good_edges(const int *edges, int n_bands)
{
    if (!edges || n_bands < 1 || n_bands > kMaxBands) return false;
    if (edges[0] < 1 || edges[n_bands] > kBins) return false;
    for (int b = 0; b < n_bands; b++)
        if (edges[b] >= edges[b + 1]) return false;
    return true;
}

}  // namespace audio_spectrum
}  // namespace fmrx
