// fmrx_project -- drop-in streaming receiver: raw u8 I/Q on stdin -> s16 PCM
// on stdout, processing on the MI355X through libfmrx.so.
//
// Process contract of the reference (src/project.cpp:385-500 and
// src/threadMonoOnly.cpp:206-267):
//   fmrx_project                    mode 0, mono          (project.cpp:390-392)
//   fmrx_project <mode> <channels>  mode 0..3, 1|2 chans  (project.cpp:393-412)
//   fmrx_project <mode>             mono, like threadMonoOnly (:210-224)
//   stdin : interleaved unsigned 8-bit I,Q            (src/iofunc.cpp:128-135)
//   stdout: native-endian s16, sample*16384, mono, or L,R interleaved for
//           2 channels (threadMonoOnly.cpp:185-191; project.cpp:292-302)
//   a trailing partial block is dropped                (project.cpp:78-79, 83)
//   diagnostics go to stderr; stdout carries PCM only.
// Same structure as the reference: a producer thread reads blocks into a
// bounded queue of QUEUE_ELEMS = 6 (include/dy4.h:30) while the consumer runs
// the device pipeline and writes PCM -- so stdin I/O overlaps GPU work -- but
// unlike the reference the queue is drained at EOF (its exit(1) in the producer
// drops up to 7 blocks nondeterministically) and the exit status is
// 0 unless --compat-exit asks for the reference's 1.
// Extra options (all --flags, never positional):
//   --rf-taps N --audio-taps N --stereo-taps N   (defaults 101 101 101: the report's final choice,
//                         doc/3DY4 Report.pdf p.7; neither shipped binary uses it)
//   --like project        the tap counts of src/project.cpp as shipped:        13 / 13 / 13
//   --like threadMonoOnly the tap counts of src/threadMonoOnly.cpp as shipped: 151 / 101
//   --blocks-per-call K   process K reference-size blocks per device call (the stream is still cut into
//                         reference-size blocks: at EOF every whole one is processed, only the trailing
//                         partial reference block is dropped, exactly as with K = 1)
//   --exact               the bit-exact mode (fmrx_pipeline_set_force_generic): every stage in the
//                         reference's float32 evaluation order, serial PLL with glibc's functions --
//                         stereo output equal to the reference's bit for bit for any stream length
//   --saturate            clamp PCM instead of the reference's wrap-around
//   --deemph US           de-emphasis of the audio with the time constant US microseconds (50: Europe, Asia; 75: the
//                         Americas, Korea; any positive value): fmrx_pipeline_set_deemphasis.  The reference has no such
//                         stage; without the flag the output is what it always was
//   --device N            HIP device ordinal
//   --compat-exit         exit status 1 at EOF, like the reference
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <vector>

#include "fmrx.h"

namespace {
constexpr size_t kQueueElems = 6;

// blocks travel as indices into a fixed pool of page-locked buffers (no per-block
// allocation, DMA-able by the GPU): `full` carries read blocks to the consumer,
// `free_` returns them
struct BlockQueue {
    std::queue<std::pair<int, size_t>> full;   // (pool index, bytes in it: whole reference blocks)
    std::queue<int> free_;
    std::mutex m;
    std::condition_variable cv;
    bool done = false;
};

[[noreturn]] void usage(const char *argv0)
{
    std::fprintf(stderr,
                 "Usage: %s [<mode 0-3> [<channels 1-2>]] [--rf-taps N] [--audio-taps N] [--stereo-taps N]\n"
                 "          [--like project|threadMonoOnly] [--blocks-per-call K] [--exact] [--saturate] [--deemph US] [--device N]\n"
                 "          [--compat-exit]\n"
                 "  --deemph US  de-emphasis time constant in microseconds (50: Europe, Asia; 75: the Americas, Korea); default: none\n",
                 argv0);
    std::exit(1);
}
}  // namespace

int main(int argc, char *argv[])
{
    int mode = 0, channels = 1, rf_taps = 101, audio_taps = 101, stereo_taps = 101, device = 0, per_call = 1;
    bool saturate = false, compat_exit = false, exact = false;
    double deemph_us = 0.0;
    std::vector<std::string> pos;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto next = [&](int &dst) {
            if (i + 1 >= argc) usage(argv[0]);
            dst = std::atoi(argv[++i]);
        };
        if (a == "--rf-taps") next(rf_taps);
        else if (a == "--audio-taps") next(audio_taps);
        else if (a == "--stereo-taps") next(stereo_taps);
        else if (a == "--blocks-per-call") next(per_call);
        else if (a == "--device") next(device);
        else if (a == "--like") {
            if (i + 1 >= argc) usage(argv[0]);
            const std::string w = argv[++i];
            if (w == "project") rf_taps = audio_taps = stereo_taps = 13;            // src/project.cpp:46, 424-429
            else if (w == "threadMonoOnly") { rf_taps = 151; audio_taps = 101; }    // src/threadMonoOnly.cpp:66, 229-232
            else usage(argv[0]);
        }
        else if (a == "--deemph") {
            if (i + 1 >= argc) usage(argv[0]);
            char *end = nullptr;
            deemph_us = std::strtod(argv[++i], &end);
            if (end == argv[i] || *end != '\0' || !(deemph_us > 0.0)) usage(argv[0]);
        }
        else if (a == "--exact") exact = true;
        else if (a == "--saturate") saturate = true;
        else if (a == "--compat-exit") compat_exit = true;
        else if (a.rfind("--", 0) == 0) usage(argv[0]);
        else pos.push_back(a);
    }
    if (pos.size() > 2) usage(argv[0]);
    if (!pos.empty()) mode = std::atoi(pos[0].c_str());
    if (pos.size() == 2) channels = std::atoi(pos[1].c_str());
    if (mode < 0 || mode > 3) {
        std::fprintf(stderr, "Wrong mode %d\n", mode);
        return 1;
    }
    if (channels < 1 || channels > 2) {
        std::fprintf(stderr, "Wrong number of channels %d\n", channels);
        return 1;
    }
    if (per_call < 1) per_call = 1;

    fmrx_params p;
    if (fmrx_mode_params(mode, rf_taps, audio_taps, stereo_taps, &p) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
        return 1;
    }
    const size_t block_bytes = static_cast<size_t>(p.block_bytes) * per_call;
    std::fprintf(stderr, "Operating in mode:%d  Number of channels set to: %d  block_size = %zu  (%s)\n", mode, channels,
                 block_bytes, fmrx_version());

    fmrx_pipeline *pl = nullptr;
    if (fmrx_pipeline_create(&pl, &p, channels, block_bytes, device) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
        return 2;
    }
    if (exact && fmrx_pipeline_set_force_generic(pl, 1) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
        return 2;
    }

    if (deemph_us > 0.0 && fmrx_pipeline_set_deemphasis(pl, deemph_us) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
        return 2;
    }

    constexpr int kPool = static_cast<int>(kQueueElems) + 2;   // 6 queued + 1 being read + 1 being processed
    std::vector<uint8_t *> pool(kPool, nullptr);
    for (int i = 0; i < kPool; i++) {
        void *ptr = nullptr;
        if (fmrx_host_alloc(&ptr, block_bytes) != FMRX_OK) {
            std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
            return 2;
        }
        pool[i] = static_cast<uint8_t *>(ptr);
    }
    BlockQueue bq;
    for (int i = 0; i < kPool; i++) bq.free_.push(i);
    std::thread producer([&] {
        for (;;) {
            int idx;
            {
                std::unique_lock<std::mutex> lk(bq.m);
                bq.cv.wait(lk, [&] { return (!bq.free_.empty() && bq.full.size() < kQueueElems) || bq.done; });
                if (bq.done) return;
                idx = bq.free_.front();
                bq.free_.pop();
            }
            const size_t got = std::fread(pool[idx], 1, block_bytes, stdin);
            // EOF inside a K-block chunk: its whole reference-size blocks still count; only the trailing
            // partial reference block is ignored, as in the reference (src/project.cpp:78-83)
            const size_t whole = got - got % static_cast<size_t>(p.block_bytes);
            std::lock_guard<std::mutex> lk(bq.m);
            if (whole) bq.full.push({idx, whole});
            if (got != block_bytes) bq.done = true;
            bq.cv.notify_all();
            if (got != block_bytes) return;
        }
    });

    const size_t n_out = fmrx_pipeline_n_audio(pl, block_bytes) * channels;
    int16_t *pcm[2] = {nullptr, nullptr};
    for (auto &q : pcm) {
        void *ptr = nullptr;
        if (fmrx_host_alloc(&ptr, n_out * sizeof(int16_t)) != FMRX_OK) {
            std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
            return 2;
        }
        q = static_cast<int16_t *>(ptr);
    }
    // Two blocks in flight (fmrx_pipeline_submit / _wait): block i+1's copy to the device and its kernels run while block i's
    // PCM is copied back and written to stdout.  Output order = input order.
    size_t blocks = 0;
    int rc = 0;
    struct InFlight { int idx; size_t bytes; bool valid; } fl[2] = {{0, 0, false}, {0, 0, false}};
    auto retire = [&](int slot) {   // the block submitted into `slot`: wait, write its PCM, give its input buffer back
        if (!fl[slot].valid) return;
        fl[slot].valid = false;
        const size_t n_pcm = fmrx_pipeline_n_audio(pl, fl[slot].bytes) * channels;
        if (fmrx_pipeline_wait(pl) != FMRX_OK) {
            std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
            rc = 3;
        } else if (std::fwrite(pcm[slot], sizeof(int16_t), n_pcm, stdout) != n_pcm) {
            std::fprintf(stderr, "fmrx: short write on stdout\n");
            rc = 4;
        }
        {
            std::lock_guard<std::mutex> lk(bq.m);
            bq.free_.push(fl[slot].idx);
            bq.cv.notify_all();
        }
        if (!rc) blocks += fl[slot].bytes / static_cast<size_t>(p.block_bytes);
    };
    int slot = 0;                                           // the slot the next submission uses; it alternates
    for (;; slot ^= 1) {
        int idx;
        size_t bytes;
        {
            std::unique_lock<std::mutex> lk(bq.m);
            bq.cv.wait(lk, [&] { return !bq.full.empty() || bq.done; });
            if (bq.full.empty()) break;
            idx = bq.full.front().first;
            bytes = bq.full.front().second;
            bq.full.pop();
        }
        retire(slot);                                       // the block that used this slot two submissions ago
        if (rc) break;
        if (fmrx_pipeline_submit(pl, pool[idx], bytes, nullptr, pcm[slot], saturate ? FMRX_PCM_SATURATE : FMRX_PCM_WRAP) != FMRX_OK) {
            std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
            rc = 3;
            break;
        }
        fl[slot] = {idx, bytes, true};
    }
    // drain in submission order (fmrx_pipeline_wait retires the oldest block first): `slot` is the one that would be
    // reused next, i.e. it holds the older of the two
    if (!rc) retire(slot);
    if (!rc) retire(slot ^ 1);
    if (rc != 0) {  // retire the producer
        std::lock_guard<std::mutex> lk(bq.m);
        bq.done = true;
        bq.cv.notify_all();
    }
    producer.join();
    std::fflush(stdout);
    std::fprintf(stderr, "End of input stream reached after %zu reference-size blocks\n", blocks);
    fmrx_pipeline_destroy(pl);
    for (auto *b : pool) fmrx_host_free(b);
    for (auto *q : pcm) fmrx_host_free(q);
    if (rc) return rc;
    return compat_exit ? 1 : 0;
}
