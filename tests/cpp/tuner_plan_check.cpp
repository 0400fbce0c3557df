// tuner_plan_check.cpp -- walks the whole domain of the wideband tuner's matrix kernels through the product's own host
// arithmetic (csrc/tuner_host.hpp: tuner_shape, tuner_lds_bytes, tuner_plan_info) on the CPU.  Test infrastructure
// (tests/test_tuner_plan_host.py builds and runs it; tests/_tuner_plan_shapes.py holds the shapes the GPU tests run).
//
//   tuner_plan_check walk                             every integer R 2..32 x T 2..256, every coprime U <= 24, 2 U <= D <= 125,
//                                                     T <= 4096 with ceil(T / U) <= 256 (U = 1: D >= 33), in the three formats
//   tuner_plan_check plan (U D T fmt N n_wide)...     the plan of each shape and call, one line each
//
// walk checks for every shape: the matrix kernels take it (tiles > 0); the LDS is at most 65 536 bytes where two workgroups are
// planned per CU and at most 163 840 otherwise; front, ks and ksp against a restatement of what the kernels compute from them
// (every tap of every image inside its K-step range, the range inside the window, ksp the largest range and at most ks and 9);
// the grid covers the steps.  It prints one line per plan class (count, the smallest shape by T, U, D, the shape with the
// largest LDS; shapes as U D T), for the direct-store class the first T of every ratio that flips to it, and the first integer and rational
// shape of every ksp.  A shape depends on T only through Tp = ceil(T / U), so the walk computes one per Tp and counts its T's.
// Exit status 1 if any check failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>

#include "tuner_host.hpp"

using namespace fmrx;

static long n_bad = 0;
static void bad(const char *what, int U, int D, int T, int fmt)
{
    if (n_bad++ < 20) std::printf("FAILED %s: U %d D %d T %d format %d\n", what, U, D, T, fmt);
}

static const char *kFmt[3] = {"u8", "s8", "s16"};

struct Extreme {
    int U = 0, D = 0, T = 0;
    size_t lds = 0;
};
struct Class {
    long count = 0;
    Extreme first, largest;   // the smallest shape (by T, then U, then D) and the first in walk order with the largest LDS; as U D T
};

static std::string class_name(int U, int D, int fmt, const TunerPlanInfo &p)
{
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s %s tiles=%d %s per_cu=%d", tuner_integer_rate(U, D) ? "int" : "rat", kFmt[fmt], p.tiles,
                  p.via_lds ? "buffered" : "direct", p.lds_bytes <= kTwoPerCu ? 2 : 1);
    return buf;
}

// front, ks, ksp, j0, j1 against what the kernels do with them (kernels_tuner.hip: tuner_phase_ranges; kernels_tuner_rational.hip:
// rat_block; tuner_mfma.hpp: tuner_mac; tuner_host.hpp: tuner_fill_image)
static void check_shape(const TunerShape &s, int U, int D, int T)
{
    const int Tp = (T + U - 1) / U, reach = 2 * (Tp - 1);
    if (s.Tp != Tp || s.front % 16 || s.front < 16 || s.front < reach || (s.front > 16 && s.front >= reach + 16)) bad("front", U, D, T, -1);
    int ksp = 0, ks = 0;
    for (int q = 0; q < kTunerPhases * U; q++) {
        const int nq = static_cast<int>(static_cast<long>(q) * D / U);   // the image's newest sample, samples into the column
        const int lo = s.front + 2 * nq - reach, hi = s.front + 2 * nq + 1;   // first and last window byte its taps meet
        if (lo < 0 || s.j0[q] != lo / 64 || s.j1[q] != hi / 64 + 1) bad("K-step range of an image", U, D, T, -1);
        if (s.j0[q] < 0 || s.j1[q] > s.ks) bad("j1 <= ks", U, D, T, -1);
        ksp = std::max(ksp, s.j1[q] - s.j0[q]);
        ks = std::max(ks, s.j1[q]);
    }
    if (s.ksp != ksp || s.ks != ks || s.ksp > s.ks || s.ksp < 1 || s.ksp > 9) bad("ks / ksp", U, D, T, -1);
}

static void check_plan(const TunerPlanInfo &p, const TunerShape &s, int U, int D, int T, int fmt, int N, long n_wide)
{
    if (!p.matrix || p.tiles <= 0) {
        bad("tiles > 0", U, D, T, fmt);
        return;
    }
    const bool integer = tuner_integer_rate(U, D);
    if (integer ? (p.tiles != (fmt == kTunerS16 ? 2 : 4) || p.via_lds) : (p.tiles > (fmt == kTunerS16 ? 2 : 4) || (p.tiles & (p.tiles - 1))))
        bad("tiles of the compiled kernels", U, D, T, fmt);
    if (p.tiles > 1 && p.lds_bytes > kTwoPerCu) bad("more than one tile only with two workgroups per CU", U, D, T, fmt);
    if (p.lds_bytes > (p.tiles > 1 ? 65536u : 163840u)) bad("LDS limit", U, D, T, fmt);
    if (p.lds_bytes != tuner_lds_bytes(U, D, s.ks, fmt, p.tiles, p.via_lds)) bad("lds_bytes", U, D, T, fmt);
    const long n_out = n_wide / D * U, per_step = 128L * U * p.tiles;
    if (static_cast<long>(p.n_steps) * per_step < n_out || static_cast<long>(p.n_steps - 1) * per_step >= n_out) bad("n_steps", U, D, T, fmt);
    if (p.grid_y != (N + 15) / 16 || p.steps_per_wg < 1 || static_cast<long>(p.grid_x) * p.steps_per_wg < p.n_steps ||
        static_cast<long>(p.grid_x - 1) * p.steps_per_wg >= p.n_steps || static_cast<long>(p.grid_x) * p.grid_y > kTunerWorkgroups + p.grid_y)
        bad("grid", U, D, T, fmt);
}

static int walk()
{
    std::map<std::string, Class> classes;
    std::map<int, Extreme> ksp_int, ksp_rat;
    long n_shapes = 0;
    for (int U = 1; U <= kTunerRatMfmaMaxU; U++)
        for (int D = 2 * U; D <= kTunerRatMfmaMaxD; D++) {
            if (tuner_gcd(U, D) != 1) continue;
            int direct_first[3] = {0, 0, 0};
            for (int Tp = 1; Tp <= kTunerMfmaMaxTaps; Tp++) {
                const int t_lo = std::max(2, U * (Tp - 1) + 1), t_hi = std::min(U * Tp, kTunerMaxTaps);   // the T's of this Tp
                if (t_lo > t_hi) continue;
                const TunerShape s = tuner_shape(t_lo, U, D);
                check_shape(s, U, D, t_lo);
                const TunerShape s_hi = tuner_shape(t_hi, U, D);
                if (s_hi.front != s.front || s_hi.ks != s.ks || s_hi.ksp != s.ksp || s_hi.j0 != s.j0 || s_hi.j1 != s.j1) bad("shape depends on Tp only", U, D, t_hi, -1);
                auto &by_ksp = tuner_integer_rate(U, D) ? ksp_int : ksp_rat;
                if (!by_ksp.count(s.ksp) && (U > 1 || D <= kTunerMaxR)) by_ksp[s.ksp] = Extreme{U, D, t_lo, 0};   // rational: a U > 1
                for (int fmt = 0; fmt < 3; fmt++) {
                    // a call of 8 steps' worth of outputs and a few more on 70 channels: the grid arithmetic with more than one row
                    const int N = 70;
                    const TunerPlanInfo p0 = tuner_plan_info(U, D, t_lo, fmt, N, 0);
                    const long n_wide = static_cast<long>(D) * (8L * 128 * std::max(p0.tiles, 1) + 3);
                    const TunerPlanInfo p = tuner_plan_info(U, D, t_lo, fmt, N, n_wide);
                    check_plan(p, s, U, D, t_lo, fmt, N, n_wide);
                    if (!p.matrix) continue;
                    Class &c = classes[class_name(U, D, fmt, p)];
                    if (!c.count || std::make_tuple(t_lo, U, D) < std::make_tuple(c.first.T, c.first.U, c.first.D)) c.first = Extreme{U, D, t_lo, p.lds_bytes};
                    if (p.lds_bytes > c.largest.lds) c.largest = Extreme{U, D, t_lo, p.lds_bytes};
                    c.count += t_hi - t_lo + 1;
                    n_shapes += t_hi - t_lo + 1;
                    if (!p.via_lds && !tuner_integer_rate(U, D) && !direct_first[fmt]) direct_first[fmt] = t_lo;
                }
            }
            for (int fmt = 0; fmt < 3; fmt++)
                if (direct_first[fmt]) std::printf("direct_first %s U %d D %d T %d\n", kFmt[fmt], U, D, direct_first[fmt]);
        }
    for (const auto &kv : classes) {
        const Class &c = kv.second;
        std::printf("class %s shapes %ld smallest %d %d %d lds %zu largest %d %d %d lds %zu\n", kv.first.c_str(), c.count, c.first.U, c.first.D,
                    c.first.T, c.first.lds, c.largest.U, c.largest.D, c.largest.T, c.largest.lds);
    }
    for (const auto &kv : ksp_int) std::printf("ksp int %d U %d D %d T %d\n", kv.first, kv.second.U, kv.second.D, kv.second.T);
    for (const auto &kv : ksp_rat) std::printf("ksp rat %d U %d D %d T %d\n", kv.first, kv.second.U, kv.second.D, kv.second.T);
    std::printf("walked %ld shapes, %ld failed checks\n", n_shapes, n_bad);
    return n_bad ? 1 : 0;
}

static int plans(int argc, char **argv)
{
    if ((argc - 2) % 6) {
        std::fprintf(stderr, "plan: groups of U D T fmt N n_wide\n");
        return 2;
    }
    for (int i = 2; i + 5 < argc; i += 6) {
        const int U = std::atoi(argv[i]), D = std::atoi(argv[i + 1]), T = std::atoi(argv[i + 2]), fmt = std::atoi(argv[i + 3]),
                  N = std::atoi(argv[i + 4]);
        const long n_wide = std::atol(argv[i + 5]);
        if (tuner_ratio_check(U, D) || T < 2 || T > kTunerMaxTaps || !tuner_format_ok(fmt) || N < 1 || n_wide < 0 || n_wide % D) {
            std::fprintf(stderr, "plan: bad shape %d %d %d %d %d %ld\n", U, D, T, fmt, N, n_wide);
            return 2;
        }
        const TunerShape s = tuner_shape(T, U, D);
        const TunerPlanInfo p = tuner_plan_info(U, D, T, fmt, N, n_wide);
        std::printf("plan %d %d %d %d %d %ld matrix %d tiles %d via_lds %d lds_bytes %zu n_steps %d steps_per_wg %d grid_x %d grid_y %d ksp %d\n", U, D, T,
                    fmt, N, n_wide, p.matrix ? 1 : 0, p.tiles, p.via_lds ? 1 : 0, p.lds_bytes, p.n_steps, p.steps_per_wg, p.grid_x, p.grid_y, s.ksp);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "walk")) return walk();
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return plans(argc, argv);
    std::fprintf(stderr, "usage: tuner_plan_check walk | plan (U D T fmt N n_wide)...\n");
    return 2;
}
