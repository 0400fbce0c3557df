// rds_station.hpp -- RDS station decoder: continuous bit recovery from the in-phase matched-filter row, block synchronisation,
// group assembly and the station record (PI, PTY, TP, TA, MS, PS name, RadioText), one definition for the host decoder
// (fmrx_rds_station_*, capi.hip) and the RDS bank's lane-per-channel kernel (rdsb_station_kernel, rds_bank.hip).
//
// This sits NEXT TO the model-faithful bit recovery (rds_common.cpp: cdr / frame_sync), which re-makes its clock recovery
// every block and therefore cannot carry an RDS group (104 bits, 87.6 ms) across a 40 ms call.  Every filter, the PLL and the
// resampler in front of the matched filter carry their history, so the matched-filter row is one continuous signal; this
// decoder keeps everything it needs across calls in `Dec` (plus the per-phase energies, held by the caller).
//
// Stages, per sample y of the row (sps samples per chip):
//   chip timing   E[p] <- E[p] + (|y| - E[p]) * kTimingAlpha for the sample's phase p (mod sps); a chip is sampled every
//                 sps + step samples, where step in {-1, 0, +1} moves the sampling phase one sample towards argmax E when
//                 E[argmax] > E[phase] * kTimingHyst (nearer way round the circle; a tie in distance moves later).  Stepping
//                 across the wrap is the inserted or skipped chip: the chip count never jumps.  A ±200 ppm chip-rate error
//                 drifts one sample every 192 chips (mode 0) or 116 chips (mode 2).
//   Manchester    M[q] <- M[q] + (|c[j-1] - c[j]| - M[q]) * kPairBeta with q = the parity of chip j-1; bits start at the chips
//                 of parity `pair`, which switches when M[other] > M[pair] * kPairHyst.  bit = (c[2k] - c[2k+1] > 0) (the
//                 biphase convention of tests/rds_signal.py), then differential decoding against the previous bit.
//   block sync    syndrome of the last 26 bits with frame_sync's parity matrix (offsets A 0x3D8, B 0x3D4, C 0x25C, C' 0x3CC,
//                 D 0x258).  Not synced: two offset matches 26 bits apart in sequence (A->B, B->C/C', C/C'->D, D->A) acquire
//                 sync.  Synced: one block every 26 bits against the expected offset (C and C' both pass in slot 2); sync is
//                 lost after kSyncLossBad bad blocks in a row.
//   correction    option max_burst 0..5 (0 = off, the default), only while sync is held (acquisition always wants two CLEAN
//                 matches).  A block whose syndrome is not a pass gets s = syndrome ^ syndrome-of-the-expected-offset looked up
//                 in a 1024-entry table (build_burst_table) that holds, for every syndrome that exactly one burst of length
//                 <= 5 inside the 26 bits produces, that burst's pattern and length.  The (26,16) code tells all bursts up to
//                 length 5 apart: bursts of length <= 1, 2, 3, 4, 5 have 26, 51, 99, 191, 367 distinct non-zero syndromes
//                 (length 6 collides), so the table is well defined up to 5 and no further.  Length <= max_burst: the pattern
//                 is XORed in and the block counts as CORRECTED: used exactly like a clean one (good_blocks, ok_mask, station
//                 data), and marked in the group's corrected mask (fmrx_rds_group.reserved[0], bit s = slot s).  Expected
//                 offset: slots 0, 1, 3: A, B, D.  Slot 2: a clean C or C' passes as ever; correction aims at C or C' by the
//                 version bit of block B when slot 1 passed (clean or corrected), and is not tried when slot 1 failed.
//                 Flywheel: a clean block clears the bad-block count, a failed one adds to it, a corrected one leaves it alone
//                 (evidence neither way).  The price: 26 random bits are taken for a block with probability
//                 (correctable syndromes + 1) / 1024 -- 0.1 % at max_burst 0, 2.6 % at 1, 5.1 % at 2, 9.8 % at 3, 18.8 % at 4
//                 and 35.9 % at 5, which is what a decoder that has lost the block grid but not yet its sync flag is fed.
//                 The offset words' syndromes themselves differ by burst syndromes (A/B 2 bits, C/D 1, A/D 2, B/C' 2, A/C' 3,
//                 C'/D 3, B/C 4, B/D 4, C/C' 5; A/C none): a block of one offset with that burst IS a clean block of the other,
//                 which is why correction aims at the expected offset only -- and why, from max_burst 4 on, a lock on the right
//                 block grid with the slots one off (A for B, B for C, C for D, D for A: 2, 4, 1, 2 bits) corrects every block
//                 and holds; corrected_blocks == good_blocks gives it away.  Up to 3 such a lock fails slots 1 and 2 of every
//                 group and is dropped after three groups.
//                 One wrong chip pair is a 2-bit burst after differential decoding: 2 is the recommended setting.
//   groups        one record per four block slots (emitted at slot 3): {block[4], ok_mask, bit_index}; ok_mask bit s = slot s
//                 passed, bit 4 = slot 2 carried C'.  bit_index = index of the group's first bit in the decoded bit stream.
//   station       updated at each group from the blocks that passed: PI (A, or C' of version-B groups), PTY / TP (B);
//                 groups 0A/0B: TA, MS, two PS characters from D at segment B & 3 (+ ps_mask); groups 2A/2B: RadioText, 2A four
//                 characters from C and D (both must pass), 2B two from D; rt_mask per segment; a change of the A/B flag clears
//                 the text (to spaces) and the mask.
//   extension     fmrx_rds_station_ext, where the caller keeps one (Out::ext), from groups whose block B passed:
//                 group_types bit 2*type + version.  0A/0B: decoder identification, bit (B>>2)&1 at position 3 - (B&3) of di,
//                 the same position set in di_mask.  0A with C passed: two alternative-frequency codes, high byte first: 1..204
//                 set that bit of the 256-bit set af_bits (87.5 + 0.1 code MHz); 224 + n sets af_announced = n (n <= 25); 250
//                 in the high byte (an LF/MF frequency follows) makes the low byte ignored; everything else (205 the filler,
//                 250 in the low byte, unassigned codes) is ignored.  1A with C passed: variant (C>>12)&7 = 0: ecc = C & 0xFF,
//                 3: lang = C & 0xFFF; 1A with D passed (C or not): pin = D; ext_seen bits 0, 1, 2 say which are valid.  4A
//                 with C and D passed: ct_mjd = ((B&3)<<15) | (C>>1), ct_hour = ((C&1)<<4) | (D>>12), ct_minute = (D>>6)&63,
//                 ct_offset = D&63, ct_bit_index = the group's bit_index, ct_count + 1 -- all only if hour < 24 and minute < 60.
//                 10A: a change of the A/B flag (B>>4)&1 clears ptyn (to spaces) and ptyn_mask; with C and D passed, four
//                 characters at segment B&1.  The counters (corrected_blocks, burst_hist, sync_losses) are carried in Dec
//                 and written by finish_ext.
// Not decoded: EON (14A), TMC (8A), open data applications (3A and their groups), 2A/2B beyond the text, 1A's other variants.
//
// Floating point: fabs, add, multiply and compare only, in a fixed order, FP contraction off -- host and device compute the
// same bits.  tests/_rds_station_model.py restates this file in Python, tests/_rds_station_ext_model.py its correction and
// extension record.
#pragma once
#include <stdint.h>

#include "fmrx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FMRX_SHD __host__ __device__ __forceinline__
#else
#include <cmath>
#define FMRX_SHD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace fmrx {
namespace rdsst {

// ---- the decoder's constants (tests/_rds_station_model.py repeats them) ----------------------------------------------------
constexpr int kMaxSps = 64;                 // samples per chip the decoder accepts (mode 0: 26, mode 2: 43)
constexpr double kTimingAlpha = 1.0 / 64;   // forgetting factor of the per-phase energies (per chip: ~64 chips = 27 ms)
constexpr double kTimingHyst = 1.03125;     // the energy maximum must exceed the current phase's by 1/32 to move it
constexpr double kPairBeta = 1.0 / 16;      // forgetting factor of the two pairings' |c[2k] - c[2k+1]|
constexpr double kPairHyst = 1.25;          // the other pairing must beat the current one by a quarter to take over
constexpr int kSyncLossBad = 6;             // bad blocks in a row that lose block sync
constexpr uint32_t kSynA = 0x3D8, kSynB = 0x3D4, kSynC = 0x25C, kSynCp = 0x3CC, kSynD = 0x258;
constexpr uint32_t kMask26 = (1u << 26) - 1, kMask27 = (1u << 27) - 1;
constexpr int kMaxBurst = 5;                // the longest burst the (26,16) code locates uniquely
constexpr int kBurstTableSize = 1024;       // one entry per syndrome: pattern in bits 0..25, burst length in bits 26..28 (0: none)

// offset codes: 0 A, 1 B, 2 C, 3 C', 4 D, -1 none
FMRX_SHD int offset_of(uint32_t syn)
{
    return syn == kSynA ? 0 : syn == kSynB ? 1 : syn == kSynC ? 2 : syn == kSynCp ? 3 : syn == kSynD ? 4 : -1;
}
FMRX_SHD uint32_t syndrome_of_offset(int off)
{
    return off == 0 ? kSynA : off == 1 ? kSynB : off == 2 ? kSynC : off == 3 ? kSynCp : kSynD;
}

// the parity matrix of frame_sync (rds_common.cpp), row k for the k-th bit of the block (first received first)
FMRX_SHD uint32_t syndrome(uint32_t w)
{
    const uint32_t P[26] = {0x200, 0x100, 0x080, 0x040, 0x020, 0x010, 0x008, 0x004, 0x002, 0x001, 0x2DC, 0x16E, 0x0B7,
                            0x287, 0x39F, 0x313, 0x355, 0x376, 0x1BB, 0x201, 0x3DC, 0x1EE, 0x0F7, 0x2A7, 0x38F, 0x31B};
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 26; k++) s ^= ((w >> (25 - k)) & 1u) ? P[k] : 0u;
    return s;
}

// The correction table, by enumeration: every burst of length 1..5 that lies inside the 26 bits (first and last bit of the
// burst wrong, the ones between either way), shortest first.  Host only, once; the kernel reads it from global memory.
// Returns the number of entries filled (367), or -1 if two bursts met in one syndrome (they do not).
inline int build_burst_table(uint32_t *t)
{
    for (int i = 0; i < kBurstTableSize; i++) t[i] = 0u;
    int n = 0;
    for (int len = 1; len <= kMaxBurst; len++)
        for (int lo = 0; lo + len <= 26; lo++)                     // lo: the burst's last received bit, counted from bit 0
            for (uint32_t mid = 0; mid < (len > 2 ? 1u << (len - 2) : 1u); mid++) {
                const uint32_t ends = len == 1 ? 1u : (1u | (1u << (len - 1)));
                const uint32_t pat = (ends | (mid << 1)) << lo;
                const uint32_t s = syndrome(pat);
                if (s == 0u || t[s] != 0u) return -1;
                t[s] = pat | (static_cast<uint32_t>(len) << 26);
                n++;
            }
    return n;
}

// A block that did not pass: sx = its syndrome ^ the expected offset's.  Repairs w and returns the burst's length where
// exactly one burst of at most max_burst bits explains sx; 0 otherwise.
FMRX_SHD int correct_block(uint32_t &w, uint32_t sx, int max_burst, const uint32_t *__restrict__ tab)
{
    const uint32_t e = tab[sx & 1023u];
    const int len = static_cast<int>(e >> 26);
    if (len == 0 || len > max_burst) return 0;
    w ^= e & kMask26;
    return len;
}

// Everything carried across calls except the per-phase energies E[sps] (the host decoder keeps them next to this struct, the
// bank's kernel in LDS) and the PS / RT text (kept in the caller's fmrx_rds_station).  Plain scalars only: the device kernel
// holds it in registers.
struct Dec {
    int32_t sps, ph, countdown, cpar;      // samples per chip; phase of the next sample; samples to the next chip; its parity
    int32_t pair, dprev, synced, slot;     // pairing; previous Manchester bit; block sync; slot of the next block (0..3)
    double cprev, m0, m1;                  // previous chip; pairing energies of parity 0 and 1
    uint64_t sr;                           // the last 64 decoded bits, newest in bit 0
    uint64_t blk;                          // the group being assembled, slot s in bits 16s..16s+15
    uint32_t nbits, bpos, bad, ok;         // bits decoded; bits since the last block; bad blocks in a row; ok_mask so far
    uint32_t gbit;                         // bit_index of the group being assembled
    uint32_t hA, hB, hC, hCp, hD;          // per offset: matches over the last 27 bits (bit 26 = 26 bits ago)
    uint32_t blocks, good, groups;         // counters of the station record
    uint32_t pi, pty, tp, ta, ms, seen, ps_mask, rt_mask, rt_ab;
    uint32_t max_burst;                    // the correction option, 0..5
    uint32_t corr, bh1, bh2, bh3, bh4, bh5, losses;   // corrected blocks, by burst length; sync losses
};

struct Out {
    fmrx_rds_station *st;                  // PS / RT are written here as groups arrive; the rest by finish()
    fmrx_rds_group *g;                     // room for max_g records of this call
    uint32_t max_g, n_g;
    const uint32_t *tab = nullptr;         // the correction table (build_burst_table); needed where max_burst > 0
    fmrx_rds_station_ext *ext = nullptr;   // the extension record, written as groups arrive; may be null (nothing kept)
};

FMRX_SHD void init(Dec &d, int sps, int max_burst = 0)
{
    d.sps = sps; d.ph = 0; d.countdown = 0; d.cpar = 0;
    d.pair = 0; d.dprev = 0; d.synced = 0; d.slot = 0;
    d.cprev = 0.0; d.m0 = 0.0; d.m1 = 0.0;
    d.sr = 0; d.blk = 0;
    d.nbits = 0; d.bpos = 0; d.bad = 0; d.ok = 0; d.gbit = 0;
    d.hA = 0; d.hB = 0; d.hC = 0; d.hCp = 0; d.hD = 0;
    d.blocks = 0; d.good = 0; d.groups = 0;
    d.pi = 0; d.pty = 0; d.tp = 0; d.ta = 0; d.ms = 0; d.seen = 0; d.ps_mask = 0; d.rt_mask = 0; d.rt_ab = 2;
    d.max_burst = static_cast<uint32_t>(max_burst);
    d.corr = 0; d.bh1 = 0; d.bh2 = 0; d.bh3 = 0; d.bh4 = 0; d.bh5 = 0; d.losses = 0;
}

// the station record of a fresh decoder: zeros, PS and RT all spaces, rt_ab = 2 (no group 2 seen)
FMRX_SHD void clear_record(fmrx_rds_station *st)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(st);
    for (int i = 0; i < 6; i++) w[i] = 0u;
    for (int i = 6; i < 24; i++) w[i] = 0x20202020u;
    st->rt_ab = 2;
}

// the extension record of a fresh decoder: zeros, ptyn all spaces, ptyn_ab = 2 (no group 10A seen), the option echoed
FMRX_SHD void clear_ext(fmrx_rds_station_ext *x, int max_burst)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(x);
    for (int i = 0; i < 32; i++) w[i] = 0u;
    w[19] = 0x20202020u;
    w[20] = 0x20202020u;
    x->ptyn_ab = 2;
    x->max_burst = static_cast<uint8_t>(max_burst);
}

// the counters of the extension record from the state (everything else is written as it arrives)
FMRX_SHD void finish_ext(const Dec &d, fmrx_rds_station_ext *x)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(x);
    w[0] = d.corr;
    w[1] = d.bh1;
    w[2] = d.bh2;
    w[3] = d.bh3;
    w[4] = d.bh4;
    w[5] = d.bh5;
    w[6] = d.losses;
    x->max_burst = static_cast<uint8_t>(d.max_burst);
}

// the scalar fields of the record from the state (the text is written as it arrives)
FMRX_SHD void finish(const Dec &d, fmrx_rds_station *st)
{
    uint32_t *w = reinterpret_cast<uint32_t *>(st);
    w[0] = d.pi | (d.pty << 16) | (d.tp << 24);
    w[1] = d.ta | (d.ms << 8) | (static_cast<uint32_t>(d.synced) << 16) | (d.seen << 24);
    w[2] = d.ps_mask | (d.rt_ab << 8) | (d.rt_mask << 16);
    w[3] = d.blocks;
    w[4] = d.good;
    w[5] = d.groups;
}

FMRX_SHD void put_block(Dec &d, int slot, uint32_t word, int off)
{
    const uint32_t info = word >> 10;
    d.blk = (d.blk & ~(0xFFFFull << (16 * slot))) | (static_cast<uint64_t>(info) << (16 * slot));
    d.ok |= 1u << slot;
    if (off == 3) d.ok |= 0x10u;
    d.good++;
}

// one alternative-frequency code of a group 0A
FMRX_SHD void ext_af_code(fmrx_rds_station_ext *x, uint32_t code)
{
    if (code >= 1u && code <= 204u) x->af_bits[code >> 5] |= 1u << (code & 31u);
    else if (code >= 224u && code <= 249u) x->af_announced = static_cast<uint8_t>(code - 224u);
}

// a group whose block B passed into the extension record (at most once per group: everything lives in memory)
FMRX_SHD void ext_group(fmrx_rds_station_ext *x, uint32_t B, uint32_t Cw, uint32_t D, uint32_t ok, uint32_t gbit)
{
    const uint32_t gt = B >> 12, ver = (B >> 11) & 1u;
    x->group_types |= 1u << (2u * gt + ver);
    if (gt == 0) {
        const uint32_t pos = 3u - (B & 3u);
        x->di = static_cast<uint8_t>((x->di & ~(1u << pos)) | (((B >> 2) & 1u) << pos));
        x->di_mask = static_cast<uint8_t>(x->di_mask | (1u << pos));
        if (ver == 0 && (ok & 4u)) {
            const uint32_t hi = Cw >> 8, lo = Cw & 0xFFu;
            ext_af_code(x, hi);
            if (hi != 250u) ext_af_code(x, lo);
        }
    } else if (ver != 0) {
        return;                                                  // the rest are version-A groups
    } else if (gt == 1) {
        if (ok & 4u) {
            const uint32_t var = (Cw >> 12) & 7u;
            if (var == 0) {
                x->ecc = static_cast<uint8_t>(Cw & 0xFFu);
                x->ext_seen |= 1u;
            } else if (var == 3) {
                x->lang = static_cast<uint16_t>(Cw & 0xFFFu);
                x->ext_seen |= 2u;
            }
        }
        if (ok & 8u) {
            x->pin = static_cast<uint16_t>(D);
            x->ext_seen |= 4u;
        }
    } else if (gt == 4) {
        const uint32_t hour = ((Cw & 1u) << 4) | (D >> 12), minute = (D >> 6) & 63u;
        if ((ok & 0xCu) == 0xCu && hour < 24u && minute < 60u) {
            x->ct_mjd = ((B & 3u) << 15) | (Cw >> 1);
            x->ct_hour = static_cast<uint8_t>(hour);
            x->ct_minute = static_cast<uint8_t>(minute);
            x->ct_offset = static_cast<uint8_t>(D & 63u);
            x->ct_bit_index = gbit;
            x->ct_count++;
        }
    } else if (gt == 10) {
        const uint32_t ab = (B >> 4) & 1u, seg = B & 1u;
        if (ab != x->ptyn_ab) {
            for (int i = 0; i < 8; i++) x->ptyn[i] = ' ';
            x->ptyn_mask = 0;
            x->ptyn_ab = static_cast<uint8_t>(ab);
        }
        if ((ok & 0xCu) == 0xCu) {
            x->ptyn[4 * seg] = static_cast<char>(Cw >> 8);
            x->ptyn[4 * seg + 1] = static_cast<char>(Cw & 0xFF);
            x->ptyn[4 * seg + 2] = static_cast<char>(D >> 8);
            x->ptyn[4 * seg + 3] = static_cast<char>(D & 0xFF);
            x->ptyn_mask = static_cast<uint8_t>(x->ptyn_mask | (1u << seg));
        }
    }
}

FMRX_SHD void end_group(Dec &d, Out &o)
{
    const uint32_t A = static_cast<uint32_t>(d.blk & 0xFFFF), B = static_cast<uint32_t>((d.blk >> 16) & 0xFFFF),
                   Cw = static_cast<uint32_t>((d.blk >> 32) & 0xFFFF), D = static_cast<uint32_t>((d.blk >> 48) & 0xFFFF);
    if (o.n_g < o.max_g) {
        uint32_t *w = reinterpret_cast<uint32_t *>(o.g + o.n_g);
        w[0] = A | (B << 16);
        w[1] = Cw | (D << 16);
        w[2] = d.ok;
        w[3] = d.gbit;
        o.n_g++;
    }
    d.groups++;
    const uint32_t ok = d.ok;
    if (ok & 1u) {
        d.pi = A;
        d.seen |= 1u;
    }
    if (!(ok & 2u)) return;
    d.pty = (B >> 5) & 31u;
    d.tp = (B >> 10) & 1u;
    d.seen |= 2u;
    const uint32_t gt = B >> 12, ver = (B >> 11) & 1u;
    if (ver && (ok & 0x14u) == 0x14u) d.pi = Cw;
    char *ps = o.st->ps, *rt = o.st->rt;
    if (gt == 0) {
        d.ta = (B >> 4) & 1u;
        d.ms = (B >> 3) & 1u;
        if (ok & 8u) {
            const uint32_t seg = B & 3u;
            ps[2 * seg] = static_cast<char>(D >> 8);
            ps[2 * seg + 1] = static_cast<char>(D & 0xFF);
            d.ps_mask |= 1u << seg;
        }
    } else if (gt == 2) {
        const uint32_t ab = (B >> 4) & 1u, seg = B & 15u;
        if (ab != d.rt_ab) {
            uint32_t *t = reinterpret_cast<uint32_t *>(rt);
            for (int i = 0; i < 16; i++) t[i] = 0x20202020u;
            d.rt_mask = 0;
            d.rt_ab = ab;
        }
        if (ver == 0) {
            if ((ok & 0xCu) == 0xCu) {
                rt[4 * seg] = static_cast<char>(Cw >> 8);
                rt[4 * seg + 1] = static_cast<char>(Cw & 0xFF);
                rt[4 * seg + 2] = static_cast<char>(D >> 8);
                rt[4 * seg + 3] = static_cast<char>(D & 0xFF);
                d.rt_mask |= 1u << seg;
            }
        } else if (ok & 8u) {
            rt[2 * seg] = static_cast<char>(D >> 8);
            rt[2 * seg + 1] = static_cast<char>(D & 0xFF);
            d.rt_mask |= 1u << seg;
        }
    }
    if (o.ext) ext_group(o.ext, B, Cw, D, ok, d.gbit);
}

// one differentially decoded bit into block sync and group assembly
FMRX_SHD void feed_bit(Dec &d, int bit, Out &o)
{
    d.sr = (d.sr << 1) | static_cast<uint64_t>(bit & 1);
    d.nbits++;
    const uint32_t w = static_cast<uint32_t>(d.sr) & kMask26;
    const uint32_t syn = syndrome(w);
    const int off = offset_of(syn);
    d.hA = ((d.hA << 1) | (off == 0 ? 1u : 0u)) & kMask27;
    d.hB = ((d.hB << 1) | (off == 1 ? 1u : 0u)) & kMask27;
    d.hC = ((d.hC << 1) | (off == 2 ? 1u : 0u)) & kMask27;
    d.hCp = ((d.hCp << 1) | (off == 3 ? 1u : 0u)) & kMask27;
    d.hD = ((d.hD << 1) | (off == 4 ? 1u : 0u)) & kMask27;
    if (!d.synced) {
        if (off < 0 || d.nbits < 52) return;
        // the offset that must have matched 26 bits ago, at bit 26 of its history
        const uint32_t before = off == 0 ? d.hD : off == 1 ? d.hA : (off == 2 || off == 3) ? d.hB : (d.hC | d.hCp);
        if (!((before >> 26) & 1u)) return;
        const int slot = off == 0 ? 0 : off == 1 ? 1 : off == 4 ? 3 : 2;
        d.synced = 1;
        d.bad = 0;
        d.bpos = 0;
        d.blk = 0;
        d.ok = 0;
        d.gbit = d.nbits - 26u * static_cast<uint32_t>(slot + 1);
        if (slot > 0) {
            const uint32_t pw = static_cast<uint32_t>(d.sr >> 26) & kMask26;
            put_block(d, slot - 1, pw, offset_of(syndrome(pw)));
            d.blocks++;
        }
        put_block(d, slot, w, off);
        d.blocks++;
        if (slot == 3) end_group(d, o);
        d.slot = (slot + 1) & 3;
        return;
    }
    if (++d.bpos < 26u) return;
    d.bpos = 0;
    const int slot = d.slot;
    if (slot == 0) {
        d.blk = 0;
        d.ok = 0;
        d.gbit = d.nbits - 26u;
    }
    const bool pass = slot == 2 ? (off == 2 || off == 3) : slot == 3 ? off == 4 : off == slot;
    d.blocks++;
    if (pass) {
        put_block(d, slot, w, off);
        d.bad = 0;
    } else {
        int len = 0, want = slot == 3 ? 4 : slot;
        if (d.max_burst != 0u && (slot != 2 || (d.ok & 2u))) {
            if (slot == 2) want = ((d.blk >> 27) & 1u) ? 3 : 2;     // the version bit of block B
            uint32_t fixed = w;
            len = correct_block(fixed, syn ^ syndrome_of_offset(want), static_cast<int>(d.max_burst), o.tab);
            if (len) {
                put_block(d, slot, fixed, want);
                d.ok |= 0x100u << slot;                             // the corrected mask, fmrx_rds_group.reserved[0]
                d.corr++;
                d.bh1 += len == 1;
                d.bh2 += len == 2;
                d.bh3 += len == 3;
                d.bh4 += len == 4;
                d.bh5 += len == 5;
            }
        }
        if (!len) d.bad++;
    }
    if (slot == 3) end_group(d, o);
    d.slot = (slot + 1) & 3;
    if (d.bad >= static_cast<uint32_t>(kSyncLossBad)) {
        d.synced = 0;
        d.losses++;
    }
}

// one chip: pairing energies, pairing decision, and a bit when the chip completes a pair
FMRX_SHD void feed_chip(Dec &d, double c, Out &o)
{
    const double diff = fabs(d.cprev - c);
    if (d.cpar) d.m0 = d.m0 + (diff - d.m0) * kPairBeta;   // the pair (j-1, j) starts at parity cpar ^ 1
    else d.m1 = d.m1 + (diff - d.m1) * kPairBeta;
    if (d.pair == 0 ? d.m1 > d.m0 * kPairHyst : d.m0 > d.m1 * kPairHyst) d.pair ^= 1;
    if ((d.cpar ^ 1) == d.pair) {
        const int manch = (d.cprev - c > 0) ? 1 : 0;
        feed_bit(d, manch ^ d.dprev, o);
        d.dprev = manch;
    }
    d.cprev = c;
    d.cpar ^= 1;
}

// one sample of the in-phase matched-filter row; E[p * es], p < sps: the per-phase energies
FMRX_SHD void feed_sample(Dec &d, double *E, int es, double y, Out &o)
{
    const int ph = d.ph;
    const double e = E[ph * es];
    E[ph * es] = e + (fabs(y) - e) * kTimingAlpha;
    if (d.countdown == 0) {
        int am = 0;
        double best = E[0];
        for (int p = 1; p < d.sps; p++) {
            const double v = E[p * es];
            if (v > best) {
                best = v;
                am = p;
            }
        }
        int step = 0;
        if (am != ph && best > E[ph * es] * kTimingHyst) {
            const int dist = am > ph ? am - ph : am - ph + d.sps;   // samples ahead, 1 .. sps-1
            step = 2 * dist <= d.sps ? 1 : -1;
        }
        d.countdown = d.sps - 1 + step;
        feed_chip(d, y, o);
    } else {
        d.countdown--;
    }
    d.ph = ph + 1 == d.sps ? 0 : ph + 1;
}

// groups one call of n samples (n_bits bits) can emit: a group at most every 26 bits, twice where sync is lost and re-acquired
// on consecutive bits
FMRX_SHD uint32_t max_groups_for_bits(uint64_t n_bits) { return static_cast<uint32_t>(2 * (n_bits / 26 + 1)); }
FMRX_SHD uint32_t max_groups_for_samples(uint64_t n, int sps)
{
    // chips are at least sps - 1 samples apart: n / (sps - 1) + 1 chips, half as many bits plus one
    const uint64_t chips = n / static_cast<uint64_t>(sps - 1) + 1;
    return max_groups_for_bits(chips / 2 + 1);
}

}  // namespace rdsst
}  // namespace fmrx
