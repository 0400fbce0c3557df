// Dumps the host-built operands of the f32 matrix-core FIRs, so that tests/test_mfma_model_host.py can compare them with
// the numpy model of the kernels (tests/_fir_model.py).  No GPU involved.
//   mfma_tables_dump audio <taps.f32> <taps> <decim> <out.f32>
//       audio_mfma_build_table (fe_mfma_host.hpp): [AK][64] floats
//   mfma_tables_dump resample <taps.f32> <taps> <upsamp> <decim> <front> <back> <out.f32> <out.txt>
//       resample_mfma_geometry (resample_mfma_host.hpp): the tap image [tile][64][4 KS4] floats; the text file holds
//       "ks4 K max_pieces nl nl_elem reach_ok" (reach within <front> / <back> samples: kResampleFront / kResampleBack),
//       then the tops, then the groups (4 numbers each), one line each
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fe_mfma_host.hpp"
#include "resample_mfma_host.hpp"

static std::vector<float> read_f32(const char *path, int n)
{
    std::vector<float> v(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(float), n, f) != static_cast<size_t>(n)) {
        std::fprintf(stderr, "cannot read %d floats from %s\n", n, path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

static void write_f32(const char *path, const std::vector<float> &v)
{
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) {
        std::fprintf(stderr, "cannot write %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
}

int main(int argc, char **argv)
{
    if (argc == 6 && !std::strcmp(argv[1], "audio")) {
        const int taps = std::atoi(argv[3]), decim = std::atoi(argv[4]);
        const std::vector<float> h = read_f32(argv[2], taps);
        std::vector<float> tab;
        fmrx::audio_mfma_build_table(h.data(), taps, decim, tab);
        write_f32(argv[5], tab);
        return 0;
    }
    if (argc == 10 && !std::strcmp(argv[1], "resample")) {
        const int taps = std::atoi(argv[3]), U = std::atoi(argv[4]), D = std::atoi(argv[5]);
        const int front = std::atoi(argv[6]), back = std::atoi(argv[7]);
        const std::vector<float> h = read_f32(argv[2], taps);
        fmrx::RsMfmaGeometry g;
        if (!fmrx::resample_mfma_geometry(h.data(), taps, U, D, g)) {
            std::fprintf(stderr, "no matrix-core plan\n");
            return 3;
        }
        write_f32(argv[8], g.img);
        FILE *f = std::fopen(argv[9], "w");
        if (!f) return 2;
        std::fprintf(f, "%d %d %d %d %d %d\n", g.ks4, g.k, g.max_pieces, fmrx::resample_mfma_nl(g.max_pieces),
                     fmrx::resample_mfma_nl_elem(g.max_pieces),
                     fmrx::resample_mfma_reach_ok(g, D, front, back) ? 1 : 0);
        for (int t : g.top) std::fprintf(f, "%d ", t);
        std::fprintf(f, "\n");
        for (int t : g.groups) std::fprintf(f, "%d ", t);
        std::fprintf(f, "\n");
        std::fclose(f);
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of this file\n");
    return 1;
}
