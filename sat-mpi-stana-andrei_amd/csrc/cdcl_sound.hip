// cdcl_sound.hip -- Kernel 11: a sound clause-learning search (CDCL) on gfx950,
// one wavefront per formula, batched over a persistent grid, whose learned
// clauses are its refutation.  The rule is stated in full in include/satmi.h
// (satmi_cdcl_sound_batch_device) and restated in tests/cdcl_sound_rows.py.
//
//   * Wave w of W takes instances w, w + W, ... (no work counter: the device
//     form owns no device memory and a launch is one kernel on the caller's
//     stream).
//   * Per-variable state in the wave's LDS region, indexed by the variable id:
//       reason  int32   CS_NONE while unassigned, -1 for a decision, else the
//                       code of the clause that implied it: c < m for formula
//                       clause c, m + (word offset of its record) for a learned
//                       clause.  Offsets ascend with the learning order, so
//                       codes order clauses as their indices do, and a code
//                       finds its record without an index array.
//       seen    1 bit   the analysis' marks (atomicOr: one lane marks a variable)
//       level   uint16  decision level
//       trail   uint16  the assigned literals in order: variable | 0x8000 if negative
//       act     uint16  activity (below 512: +1 per learned clause, halved every 256 conflicts)
//       flags   uint8   bits 0-1 the value (0 unassigned, 1 true, 2 false), bit 2
//                       the saved phase, bit 3 "occurs in the formula"
//   * The learned clauses live in the instance's region of `lemmas`, one record
//     `len, lit_1 .. lit_len` each: the clause database and the proof log at once.
//   * A propagation round evaluates every clause under the assignment of the
//     round's start: nothing is assigned while it scans.  A unit clause offers
//     its literal: reason[v] takes the lowest offering code (formula clauses of
//     the short form by an LDS atomicMin within a 64-clause step, whose winners
//     are pushed in lane order; otherwise clause after clause, first come).  The
//     offered literals wait behind the trail's end, in ascending order of their
//     clause, and become assignments when the round found no falsified clause;
//     else they are retracted.  The formula is scanned in one of refute.hip's
//     two forms (lane-per-clause up to CS_SHORT_MAX literals, else
//     wave-per-clause), the learned records wave-per-clause along their chain.
//   * Every loop carries its bound in its condition; a record that does not fit
//     the region is counted and never written, in part or whole.
//   * Under assumptions (satmi_cdcl_assume_batch_device, restated in
//     tests/cdcl_assume_rows.py) level i <= k belongs to assumption i, read from
//     the caller's array at each fixpoint below level k; a false one ends the
//     search with the final analysis, a walk down the trail along the reasons
//     that collects the failed assumptions.  The search kernel and the pack's
//     scan are compiled twice from cdcl_sound_search.inc, without and with it.
//   * With carried lemmas (satmi_cdcl_carry_batch_device, restated in
//     tests/cdcl_carry_rows.py) an instance starts with records in its region:
//     the wave walks their chain once, refusing a malformed one before it
//     touches anything, marks their variables as occurring and starts with
//     `used` behind them; from then on they are learned clauses.  A third
//     inclusion of the same text gives that search kernel.
//   * Minimal cores (satmi_cdcl_shrink_batch_device, restated in
//     tests/cdcl_shrink_rows.py): a fourth inclusion wraps the instance's body
//     in the loop of a chain of queries.  After a query that ended ASSUMED the
//     wave keeps the core in the caller's scratch, rebuilds the per-variable
//     arrays as every query does, walks the region again as the next query's
//     carry, and searches under the core less one literal; no wave waits for
//     another, and nothing of the chain lives in LDS.
//
// Plain C++ and vector memory operations only.  The translation unit shares no
// device code with any other kernel, whose machine code stays what it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "batch_host.h"
#include "carry_records.h"
#include "common.h"

namespace satmi {

constexpr int CS_SHORT_MAX = 8;            // longest clause of the lane-per-clause form
constexpr int32_t CS_NONE = INT32_MAX;     // reason of an unassigned variable
constexpr int CS_RUNNING = -1;

// LDS words of one wave's arrays for variables 0 .. max_vars (each a multiple of 4 bytes)
constexpr uint32_t cs_reason_words(uint32_t v) { return v + 1u; }
constexpr uint32_t cs_seen_words(uint32_t v) { return (v + 32u) >> 5; }
constexpr uint32_t cs_half_words(uint32_t v) { return (v + 2u) >> 1; }
constexpr uint32_t cs_byte_words(uint32_t v) { return (v + 4u) >> 2; }
constexpr uint32_t cs_region_words(uint32_t v) {
    return (cs_reason_words(v) + cs_seen_words(v) + 3u * cs_half_words(v) + cs_byte_words(v) + 3u) & ~3u;
}
static_assert(SATMI_CDCL_SOUND_MAX_VARS < 0x8000, "a trail entry is 15 bits of variable and a sign");
static_assert(SATMI_CDCL_SOUND_MAX_VARS <= SATMI_TRIM_MAX_VARS, "every proof can be checked and trimmed");
static_assert(4u * cs_region_words(SATMI_CDCL_SOUND_MAX_VARS) <= LDS_PER_CU, "a region fits a CU at the limit");

struct CsArgs {
    const int32_t *icb, *clb, *lits, *nvars;   // the formulas (CSR)
    int32_t *lemmas;
    const int64_t *lemma_begin;
    int32_t *status;
    int64_t *counters;                         // [B x SATMI_CDCL_SOUND_NCOUNTERS]
    int32_t *row_len, *row_lits;
    int64_t *info;                             // [B x SATMI_CDCL_SOUND_NWORDS]
    int num_instances, stride;
    uint32_t max_vars, region_words;
    int64_t conflict_limit;
    uint64_t time_limit_ticks;
};

// The same under assumptions: instance b assumes assume_lits[assume_begin[b] ..
// assume_begin[b + 1]), in that order, and answers with its failed ones.
struct CsAssumeArgs : CsArgs {
    const int32_t *assume_begin, *assume_lits;
    int32_t *core_len, *core_lits;             // [B], [B x core_stride]
    int core_stride;
};

// The same with carried lemmas: instance b starts with carry_in[b] = (records,
// words) in its region (nullptr: none anywhere) and ends with carry_out[b], the
// non-empty records there.  Only wave b touches entry b: the two may be one array.
struct CsCarryArgs : CsAssumeArgs {
    const int64_t *carry_in;
    int64_t *carry_out;                        // [B x 2]
};

// The same as a chain of queries that shrinks the core: instance b's scratch is
// work_lits[2 * assume_begin[b] .. 2 * assume_begin[b + 1]), touched by its wave only.
struct CsShrinkArgs : CsCarryArgs {
    int32_t *work_lits;
    int64_t *shrink_info;                      // [B x SATMI_CDCL_SHRINK_NWORDS]
};

struct CsWave {
    int32_t *reason;
    uint32_t *seen;
    uint16_t *level, *trail, *act;
    uint8_t *flags;
    const int32_t *fclb, *lits;   // the formula: clause c is lits[fclb[c] .. fclb[c + 1])
    int32_t *rec;                 // the instance's lemma region
    int64_t used, room;           // words written, words there
    int m, nv;
    int trail_len, ncand, cur;    // wave-uniform
};

__device__ __forceinline__ uint32_t cs_var(int32_t l) { return l < 0 ? 0u - (uint32_t)l : (uint32_t)l; }
__device__ __forceinline__ uint16_t cs_enc(int32_t l) { return (uint16_t)(cs_var(l) | (l < 0 ? 0x8000u : 0u)); }
__device__ __forceinline__ int32_t cs_dec(uint16_t e) { return (e & 0x8000u) ? -(int32_t)(e & 0x7FFFu) : (int32_t)e; }
// 0 unassigned, 1 true, 2 false
__device__ __forceinline__ uint32_t cs_val(const CsWave &w, int32_t l) {
    const uint32_t x = w.flags[cs_var(l)] & 3u;
    return x == 0u ? 0u : ((l > 0) == (x == 1u)) ? 1u : 2u;
}
__device__ __forceinline__ bool cs_seen(const CsWave &w, uint32_t v) { return (w.seen[v >> 5] >> (v & 31u)) & 1u; }

// The whole wave evaluates one clause of `len` literals at `p`: 0 = satisfied or
// open, 1 = unit with *u its literal, 2 = falsified.  Wave-uniform.
__device__ __forceinline__ int cs_eval_wave(const CsWave &w, const int32_t *p, int len, int32_t *u_out) {
    const int ln = lane_id();
    bool sat = false, many = false, have = false;
    int32_t u = 0;
    for (int j0 = 0; j0 < len && !sat; j0 += 64) {
        const int j = j0 + ln;
        uint32_t st = 2u;   // a lane past the clause's end decides nothing
        int32_t l = 0;
        if (j < len) {
            l = p[j];
            st = cs_val(w, l);
        }
        sat = __ballot(st == 1u) != 0ull;
        const uint64_t om = __ballot(st == 0u);
        if (om) {
            if (!have) u = __builtin_amdgcn_readlane(l, (int)__builtin_ctzll(om));
            have = true;
            many |= __ballot(st == 0u && l != u) != 0ull;
        }
    }
    *u_out = u;
    return sat ? 0 : !have ? 2 : many ? 0 : 1;
}

// A unit clause of code `code` (ascending from call to call within a round)
// offers its literal; the first offer for a variable stands.
__device__ __forceinline__ void cs_offer_wave(CsWave &w, int32_t code, int32_t u) {
    const uint32_t v = cs_var(u);
    const bool first = uniform_i32(w.reason[v]) == CS_NONE;
    if (first) {
        if (lane_id() == 0) {
            w.reason[v] = code;
            w.trail[w.trail_len + w.ncand] = cs_enc(u);   // < nv: one entry per unassigned variable
        }
        ++w.ncand;
        wave_sync();
    }
}

// One round over the formula, a lane per clause.  Returns the lowest falsified clause or -1.
__device__ __forceinline__ int cs_scan_short(CsWave &w) {
    const int ln = lane_id();
    for (int cb = 0; cb < w.m; cb += 64) {
        const int c = cb + ln;
        bool unit = false, fals = false;
        int32_t u = 0;
        if (c < w.m) {
            const int s = w.fclb[c], e = w.fclb[c + 1];
            bool sat = false, many = false, have = false;
            for (int j = s; j < e; ++j) {
                const int32_t l = w.lits[j];
                const uint32_t st = cs_val(w, l);
                sat |= st == 1u;
                if (st == 0u) {
                    many |= have && l != u;
                    if (!have) u = l;
                    have = true;
                }
            }
            fals = !sat && !have;
            unit = !sat && have && !many;
        }
        const uint64_t fm = __ballot(fals);
        if (fm) return cb + (int)__builtin_ctzll(fm);
        if (__ballot(unit) == 0ull) continue;
        const uint32_t v = cs_var(u);
        if (unit) atomicMin(&w.reason[v], c);
        wave_sync();
        const bool win = unit && w.reason[v] == c;   // (a variable offered by an earlier step keeps its lower clause)
        const uint64_t wm = __ballot(win);
        if (win) w.trail[w.trail_len + w.ncand + __popcll(wm & lanemask_lt())] = cs_enc(u);
        w.ncand += __popcll(wm);
        wave_sync();
    }
    return -1;
}

// The same, the whole wave on one clause at a time.
__device__ __forceinline__ int cs_scan_long(CsWave &w) {
    for (int c = 0; c < w.m; ++c) {
        const int s = uniform_i32(w.fclb[c]), e = uniform_i32(w.fclb[c + 1]);
        int32_t u;
        const int k = cs_eval_wave(w, w.lits + s, e - s, &u);
        if (k == 2) return c;
        if (k == 1) cs_offer_wave(w, c, u);
    }
    return -1;
}

// The learned clauses, along the chain of their records.  Returns a code or -1.
__device__ __forceinline__ int cs_scan_learned(CsWave &w) {
    for (int64_t p = 0; p < w.used;) {
        const int len = uniform_i32(w.rec[p]);
        int32_t u;
        const int k = cs_eval_wave(w, w.rec + p + 1, len, &u);
        if (k == 2) return w.m + (int)p;
        if (k == 1) cs_offer_wave(w, w.m + (int)p, u);
        p += 1 + (int64_t)max(len, 0);
    }
    return -1;
}

// The clause of a code: its literals and their number.
__device__ __forceinline__ const int32_t *cs_clause(const CsWave &w, int code, int *len) {
    if (code < w.m) {
        const int s = uniform_i32(w.fclb[code]);
        *len = uniform_i32(w.fclb[code + 1]) - s;
        return w.lits + s;
    }
    const int32_t *p = w.rec + (code - w.m);
    *len = uniform_i32(p[0]);
    return p + 1;
}

// ------------------------------------------------------------------ the pack
// The lemma regions of a solve as the proof triple of the refutation check.
// An instance contributes its records when it ended UNSAT (its region then holds
// all of them), else none.
struct CsPack {
    const int32_t *status, *lemmas;
    const int64_t *lemma_begin;
    int64_t *info;
    int32_t *pib, *pcb, *plits;
    int64_t clause_cap, lit_cap;
    int64_t *totals;
    int num_instances;
};

// (ASSUMED: the pack of the assumption-carrying solve, where an instance that
// ended ASSUMED contributes too: its region is closed like an UNSAT one's.)
template <bool ASSUMED>
__device__ __forceinline__ void cs_contribution(const CsPack &P, int b, int64_t *n, int64_t *l) {
    const int64_t *w = P.info + (int64_t)b * SATMI_CDCL_SOUND_NWORDS;
    const int32_t st = P.status[b];
    const bool whole = (st == SATMI_CDCL_SOUND_UNSAT || (ASSUMED && st == SATMI_CDCL_SOUND_ASSUMED)) &&
                       !(w[2] & SATMI_CDCL_SOUND_TRUNCATED);
    *n = whole ? w[0] : 0;
    *l = whole ? w[1] - w[0] : 0;
}

__device__ __forceinline__ int64_t cs_incl_scan64(int64_t x) {
    const int ln = lane_id();
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d, 64);
        if (ln >= d) x += y;
    }
    return x;
}

// ------------------------------------------------------------------ the kernels
// The search and the pack's scan, in both forms: cdcl_sound_search.inc is their
// text.  The first inclusion gives the kernels of satmi_cdcl_sound_* as they
// always were; the second the assumption-carrying ones of satmi_cdcl_assume_*;
// the third the search of satmi_cdcl_carry_*, which starts from carried lemmas;
// the fourth the search of satmi_cdcl_shrink_*, a chain of such searches.
#define CS_ASSUME 0
#define CS_CARRY 0
#define CS_SHRINK 0
#define CS_SEARCH_KERNEL cdcl_sound_kernel
#define CS_SEARCH_ARGS CsArgs
#define CS_PACK_SCAN_KERNEL cdcl_sound_pack_scan_kernel
#include "cdcl_sound_search.inc"
#undef CS_ASSUME
#undef CS_SEARCH_KERNEL
#undef CS_SEARCH_ARGS
#undef CS_PACK_SCAN_KERNEL
#define CS_ASSUME 1
#define CS_SEARCH_KERNEL cdcl_assume_kernel
#define CS_SEARCH_ARGS CsAssumeArgs
#define CS_PACK_SCAN_KERNEL cdcl_assume_pack_scan_kernel
#include "cdcl_sound_search.inc"
#undef CS_ASSUME
#undef CS_CARRY
#undef CS_SEARCH_KERNEL
#undef CS_SEARCH_ARGS
#undef CS_PACK_SCAN_KERNEL
#define CS_ASSUME 1
#define CS_CARRY 1
#define CS_SEARCH_KERNEL cdcl_carry_kernel
#define CS_SEARCH_ARGS CsCarryArgs
#include "cdcl_sound_search.inc"
#undef CS_SHRINK
#undef CS_SEARCH_KERNEL
#undef CS_SEARCH_ARGS
#define CS_SHRINK 1
#define CS_SEARCH_KERNEL cdcl_shrink_kernel
#define CS_SEARCH_ARGS CsShrinkArgs
#include "cdcl_sound_search.inc"
#undef CS_ASSUME
#undef CS_CARRY
#undef CS_SHRINK
#undef CS_SEARCH_KERNEL
#undef CS_SEARCH_ARGS

// One wavefront per instance, record after record.
__global__ void __launch_bounds__(256) cdcl_sound_pack_copy_kernel(CsPack P) {
    const int ln = lane_id();
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int b = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); b < P.num_instances; b += waves) {
        const int cb = P.pib[b];
        const int n = P.pib[b + 1] - cb;
        if (n <= 0) continue;   // no contribution, or totals that do not fit
        const int64_t *w = P.info + (int64_t)b * SATMI_CDCL_SOUND_NWORDS;
        const int64_t words = w[1], lbase = w[3];
        const int32_t *rec = P.lemmas + P.lemma_begin[b];
        int64_t p = 0;
        for (int k = 0; k < n && p < words; ++k) {
            const int len = max(uniform_i32(rec[p]), 0);
            const int64_t at = lbase + p - k;   // the words before it, less their headers
            if (ln == 0 && cb + (int64_t)k < P.clause_cap) P.pcb[cb + k] = (int32_t)at;
            for (int j = ln; j < len && p + 1 + j < words; j += 64)
                if (at + j < P.lit_cap) P.plits[at + j] = rec[p + 1 + j];
            p += 1 + (int64_t)len;
        }
    }
}

// ------------------------------------------------------------------ the carry pack
// The kept lemmas of a carrying solve as a clause triple: instance b's are the
// first carry[2b] records, carry[2b + 1] words, of its region, whatever its
// status.  Counts that no region holds (negative, fewer words than records,
// more words than the region) contribute nothing.
struct CsCarryPack {
    const int32_t *lemmas;
    const int64_t *lemma_begin, *carry;
    int32_t *kib, *kcb, *klits;
    int64_t clause_cap, lit_cap;
    int64_t *totals;
    int num_instances;
};

__device__ __forceinline__ void cs_carry_contribution(const CsCarryPack &P, int b, int64_t *n, int64_t *l) {
    const int64_t r = P.carry[2 * (int64_t)b], wd = P.carry[2 * (int64_t)b + 1];
    const bool ok = r > 0 && wd >= 2 * r && wd <= P.lemma_begin[b + 1] - P.lemma_begin[b];
    *n = ok ? r : 0;
    *l = ok ? wd - r : 0;
}

// One wavefront, as the packs' scan above.  There is no info word to keep an
// instance's literal offset in: it goes where its first clause's offset belongs,
// which the copy kernel reads before it writes the same value there.
__global__ void __launch_bounds__(64) cdcl_carry_pack_scan_kernel(CsCarryPack P) {
    const int ln = lane_id(), B = P.num_instances;
    int64_t sn = 0, sl = 0;
    for (int b = ln; b < B; b += 64) {
        int64_t n, l;
        cs_carry_contribution(P, b, &n, &l);
        sn += n;
        sl += l;
    }
    const int64_t tn = __shfl(cs_incl_scan64(sn), 63, 64), tl = __shfl(cs_incl_scan64(sl), 63, 64);
    const bool fits = tn <= P.clause_cap && tl <= P.lit_cap && tn <= INT32_MAX - 1 && tl <= INT32_MAX;
    if (ln == 0) {
        P.totals[0] = tn;
        P.totals[1] = tl;
        P.kib[B] = fits ? (int32_t)tn : 0;
    }
    int64_t cn = 0, cl = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + ln;
        int64_t n = 0, l = 0;
        if (b < B) cs_carry_contribution(P, b, &n, &l);
        const int64_t in = cs_incl_scan64(n), il = cs_incl_scan64(l);
        if (b < B) {
            P.kib[b] = fits ? (int32_t)(cn + in - n) : 0;
            if (fits && n > 0) P.kcb[cn + in - n] = (int32_t)(cl + il - l);   // (< tn <= clause_cap)
        }
        cn += __shfl(in, 63, 64);
        cl += __shfl(il, 63, 64);
    }
    if (ln == 0) P.kcb[fits ? tn : 0] = fits ? (int32_t)tl : 0;   // (after the offsets: with no lemma it is word 0)
}

// One wavefront per instance, record after record.
__global__ void __launch_bounds__(256) cdcl_carry_pack_copy_kernel(CsCarryPack P) {
    const int ln = lane_id();
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int b = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); b < P.num_instances; b += waves) {
        const int cb = P.kib[b];
        const int n = P.kib[b + 1] - cb;
        if (n <= 0) continue;   // no lemma kept, or totals that do not fit
        const int64_t words = P.carry[2 * (int64_t)b + 1];   // (within the region: the scan counted it)
        const int64_t lbase = uniform_i32(P.kcb[cb]);
        wave_sync();
        const int32_t *rec = P.lemmas + P.lemma_begin[b];
        int64_t p = 0;
        for (int k = 0; k < n && p < words; ++k) {
            const int len = max(uniform_i32(rec[p]), 0);
            const int64_t at = lbase + p - k;   // the words before it, less their headers
            if (ln == 0 && cb + (int64_t)k < P.clause_cap) P.kcb[cb + k] = (int32_t)at;
            for (int j = ln; j < len && p + 1 + j < words; j += 64)
                if (at + j < P.lit_cap) P.klits[at + j] = rec[p + 1 + j];
            p += 1 + (int64_t)len;
        }
    }
}

// The host form's carried records, from their image to the head of each region
// (one wavefront per instance).  A chain larger than its region stays where it
// is: the search refuses that instance before it reads a word.
__global__ void __launch_bounds__(256) cdcl_carry_place_kernel(const int32_t *image, const int64_t *image_begin,
                                                               int32_t *lemmas, const int64_t *lemma_begin,
                                                               int num_instances) {
    const int ln = lane_id();
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int b = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); b < num_instances; b += waves) {
        const int64_t from = image_begin[b], n = image_begin[b + 1] - from, to = lemma_begin[b];
        if (n > lemma_begin[b + 1] - to) continue;
        for (int64_t j = ln; j < n; j += 64) lemmas[to + j] = image[from + j];
    }
}

// ------------------------------------------------------------------ host side
namespace {

constexpr OomText CS_OOM{"satmi_cdcl_sound_batch_host", "split the batch"};
constexpr OomText CS_ASSUME_OOM{"satmi_cdcl_assume_batch_host", "split the batch"};
constexpr OomText CS_CARRY_OOM{"satmi_cdcl_carry_batch_host", "split the batch"};
constexpr OomText CS_SHRINK_OOM{"satmi_cdcl_shrink_batch_host", "split the batch"};

std::atomic<int> g_cs_grid{0}, g_cs_wpg{0};      // satmi_cdcl_sound_debug_grid
std::atomic<int64_t> g_cs_room{0};               // satmi_cdcl_sound_debug_room

// The workspace a satmi_cdcl_sound_batch_host call leases: one carved block for
// the batch, the proof and the outputs, and the lemma regions.
struct CdclSoundWork : WorkStream {
    DevBuf block, lemmas;
    PinBuf carry_h;   // satmi_cdcl_carry_batch_host: the carried records, their ranges and counts
};

int cs_too_large(const char *who, int64_t max_vars) {
    set_error(std::string(who) + ": variable " + std::to_string(max_vars) + " is beyond the layout's " +
              std::to_string(SATMI_CDCL_SOUND_MAX_VARS));
    return SATMI_ERR_TOO_LARGE;
}

}  // namespace

}  // namespace satmi

using namespace satmi;

extern "C" uint64_t satmi_cdcl_sound_lds_bytes(int max_vars) {
    return max_vars < 0 || max_vars > SATMI_CDCL_SOUND_MAX_VARS ? 0 : 4ull * cs_region_words((uint32_t)max_vars);
}

extern "C" int satmi_cdcl_sound_debug_grid(int workgroups, int waves_per_wg) {
    if (workgroups < 0 || !(waves_per_wg == 0 || waves_per_wg == 1 || waves_per_wg == 2 || waves_per_wg == 4))
        return fail_arg("satmi_cdcl_sound_debug_grid", "workgroups >= 0 and waves_per_wg one of 0, 1, 2, 4");
    g_cs_grid = workgroups;
    g_cs_wpg = waves_per_wg;
    return SATMI_OK;
}

extern "C" int satmi_cdcl_sound_debug_room(int64_t words) {
    if (words < 0) return fail_arg("satmi_cdcl_sound_debug_room", "words >= 0");
    g_cs_room.store(words);
    return SATMI_OK;
}

namespace {

// The assumption arrays and core outputs of the satmi_cdcl_assume_* forms.
struct CsAssumeIo {
    const int32_t *begin, *lits;
    int32_t *core_len, *core_lits;
    int core_stride;
};

// The carried-lemma counts of satmi_cdcl_carry_batch_device.
struct CsCarryDev {
    const int64_t *in;
    int64_t *out;
};

// The scratch and the chain's words of satmi_cdcl_shrink_batch_device.
struct CsShrinkDev {
    int32_t *work;
    int64_t *info;
};

// The device forms: `as` = nullptr is satmi_cdcl_sound_batch_device, its kernels and all;
// `cy` (with `as`) is satmi_cdcl_carry_batch_device; `sk` (with both) satmi_cdcl_shrink_batch_device.
int cs_solve_device(const char *who, const CsAssumeIo *as, const CsCarryDev *cy, const CsShrinkDev *sk, int num_instances, const int32_t *d_inst_clause_begin,
                    const int32_t *d_clause_lit_begin, const int32_t *d_lits, const int32_t *d_inst_nvars,
                    int max_vars, int max_clause_len, int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                    const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters, int32_t *d_row_len,
                    int32_t *d_row_lits, int stride, int64_t *d_info, void *stream) {
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (max_vars < 0 || max_clause_len < 0) return fail_arg(who, "negative max_vars / max_clause_len");
    if (stride < 1) return fail_arg(who, "row stride < 1");
    if (as && as->core_stride < 0) return fail_arg(who, "negative core_stride");
    if (num_instances == 0) return SATMI_OK;
    if (!d_inst_clause_begin || !d_clause_lit_begin || !d_lits || !d_inst_nvars || !d_lemmas || !d_lemma_begin ||
        !d_status || !d_counters || !d_row_len || !d_row_lits || !d_info)
        return fail_arg(who, "null pointer");
    if (as && (!as->begin || !as->lits || !as->core_len || (as->core_stride > 0 && !as->core_lits)))
        return fail_arg(who, "null pointer");
    if (cy && !cy->out) return fail_arg(who, "null pointer");
    if (sk && (!sk->work || !sk->info)) return fail_arg(who, "null pointer");
    if (max_vars > SATMI_CDCL_SOUND_MAX_VARS) return cs_too_large(who, max_vars);
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts));
    CsArgs A{};
    A.icb = d_inst_clause_begin;
    A.clb = d_clause_lit_begin;
    A.lits = d_lits;
    A.nvars = d_inst_nvars;
    A.lemmas = d_lemmas;
    A.lemma_begin = d_lemma_begin;
    A.status = d_status;
    A.counters = d_counters;
    A.row_len = d_row_len;
    A.row_lits = d_row_lits;
    A.info = d_info;
    A.num_instances = num_instances;
    A.stride = stride;
    A.max_vars = (uint32_t)max_vars;
    A.region_words = cs_region_words(A.max_vars);
    A.conflict_limit = conflict_limit;
    A.time_limit_ticks = time_limit_s > 0 ? (uint64_t)(time_limit_s * facts.ticks_per_s) : 0;
    const size_t region = 4 * (size_t)A.region_words;
    // waves per workgroup: the most waves resident on a CU by LDS, the wider on a tie
    int wpg = g_cs_wpg;
    if (wpg == 0) {
        size_t best = 0;
        for (int w : {4, 2, 1}) {
            const size_t resident = (size_t)w * std::min<size_t>(LDS_PER_CU / (region * (size_t)w), (size_t)(32 / w));
            if (resident > best) best = resident, wpg = w;
        }
    }
    const size_t lds_bytes = region * (size_t)wpg;
    if (lds_bytes > LDS_PER_CU) {
        set_error(std::string(who) + ": workgroups of " + std::to_string(wpg) + " waves do not fit the LDS at " +
                  std::to_string(max_vars) + " variables");
        return SATMI_ERR_TOO_LARGE;
    }
    const int wgs = (int)(((int64_t)num_instances + wpg - 1) / wpg);
    const int grid = batch_grid(facts, lds_bytes, 0, 64 * wpg, wgs, g_cs_grid);
    const bool long_form = max_clause_len <= 0 || max_clause_len > CS_SHORT_MAX;
    hipStream_t s = (hipStream_t)stream;
    if (sk) {
        CsShrinkArgs SA{};
        static_cast<CsArgs &>(SA) = A;
        SA.assume_begin = as->begin;
        SA.assume_lits = as->lits;
        SA.core_len = as->core_len;
        SA.core_lits = as->core_lits;
        SA.core_stride = as->core_stride;
        SA.carry_in = cy->in;
        SA.carry_out = cy->out;
        SA.work_lits = sk->work;
        SA.shrink_info = sk->info;
        const void *fn = long_form ? (const void *)cdcl_shrink_kernel<true> : (const void *)cdcl_shrink_kernel<false>;
        SATMI_TRY(batch_allow_lds(fn, lds_bytes));
        if (long_form)
            hipLaunchKernelGGL(cdcl_shrink_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, SA);
        else
            hipLaunchKernelGGL(cdcl_shrink_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, SA);
        SATMI_HIP(hipGetLastError());
        return SATMI_OK;
    }
    if (cy) {
        CsCarryArgs CA{};
        static_cast<CsArgs &>(CA) = A;
        CA.assume_begin = as->begin;
        CA.assume_lits = as->lits;
        CA.core_len = as->core_len;
        CA.core_lits = as->core_lits;
        CA.core_stride = as->core_stride;
        CA.carry_in = cy->in;
        CA.carry_out = cy->out;
        const void *fn = long_form ? (const void *)cdcl_carry_kernel<true> : (const void *)cdcl_carry_kernel<false>;
        SATMI_TRY(batch_allow_lds(fn, lds_bytes));
        if (long_form)
            hipLaunchKernelGGL(cdcl_carry_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, CA);
        else
            hipLaunchKernelGGL(cdcl_carry_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, CA);
        SATMI_HIP(hipGetLastError());
        return SATMI_OK;
    }
    if (as) {
        CsAssumeArgs AA{};
        static_cast<CsArgs &>(AA) = A;
        AA.assume_begin = as->begin;
        AA.assume_lits = as->lits;
        AA.core_len = as->core_len;
        AA.core_lits = as->core_lits;
        AA.core_stride = as->core_stride;
        const void *fn = long_form ? (const void *)cdcl_assume_kernel<true> : (const void *)cdcl_assume_kernel<false>;
        SATMI_TRY(batch_allow_lds(fn, lds_bytes));
        if (long_form)
            hipLaunchKernelGGL(cdcl_assume_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, AA);
        else
            hipLaunchKernelGGL(cdcl_assume_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, AA);
        SATMI_HIP(hipGetLastError());
        return SATMI_OK;
    }
    const void *fn = long_form ? (const void *)cdcl_sound_kernel<true> : (const void *)cdcl_sound_kernel<false>;
    SATMI_TRY(batch_allow_lds(fn, lds_bytes));
    if (long_form)
        hipLaunchKernelGGL(cdcl_sound_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    else
        hipLaunchKernelGGL(cdcl_sound_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

// Both packs: `assumed` = an instance that ended ASSUMED has its lemmas in the proof too.
int cs_pack_device(const char *who, bool assumed, int num_instances, const int32_t *d_status, const int32_t *d_lemmas,
                   const int64_t *d_lemma_begin, int64_t *d_info, int32_t *d_proof_inst_begin,
                   int32_t *d_proof_clause_begin, int64_t proof_clause_cap, int32_t *d_proof_lits,
                   int64_t proof_lit_cap, int64_t *d_totals, void *stream) {
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (proof_clause_cap < 1 || proof_lit_cap < 1) return fail_arg(who, "non-positive proof capacity");
    if (num_instances == 0) return SATMI_OK;
    if (!d_status || !d_lemmas || !d_lemma_begin || !d_info || !d_proof_inst_begin || !d_proof_clause_begin ||
        !d_proof_lits || !d_totals)
        return fail_arg(who, "null pointer");
    CsPack P{};
    P.status = d_status;
    P.lemmas = d_lemmas;
    P.lemma_begin = d_lemma_begin;
    P.info = d_info;
    P.pib = d_proof_inst_begin;
    P.pcb = d_proof_clause_begin;
    P.plits = d_proof_lits;
    P.clause_cap = proof_clause_cap;
    P.lit_cap = proof_lit_cap;
    P.totals = d_totals;
    P.num_instances = num_instances;
    hipStream_t s = (hipStream_t)stream;
    if (assumed)
        hipLaunchKernelGGL(cdcl_assume_pack_scan_kernel, dim3(1), dim3(64), 0, s, P);
    else
        hipLaunchKernelGGL(cdcl_sound_pack_scan_kernel, dim3(1), dim3(64), 0, s, P);
    SATMI_HIP(hipGetLastError());
    const int wgs = std::min((num_instances + 3) / 4, 8192);
    hipLaunchKernelGGL(cdcl_sound_pack_copy_kernel, dim3(wgs), dim3(256), 0, s, P);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

}  // namespace

extern "C" int satmi_cdcl_sound_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                             const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                             const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                             int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                             const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                             int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                             void *stream) {
    return cs_solve_device("satmi_cdcl_sound_batch_device", nullptr, nullptr, nullptr, num_instances, d_inst_clause_begin,
                           d_clause_lit_begin, d_lits, d_inst_nvars, max_vars, max_clause_len, conflict_limit,
                           time_limit_s, d_lemmas, d_lemma_begin, d_status, d_counters, d_row_len, d_row_lits, stride,
                           d_info, stream);
}

extern "C" int satmi_cdcl_assume_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                              const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                              const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                              int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                              const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                              int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                              const int32_t *d_assume_begin, const int32_t *d_assume_lits,
                                              int32_t *d_core_len, int32_t *d_core_lits, int core_stride,
                                              void *stream) {
    const CsAssumeIo as{d_assume_begin, d_assume_lits, d_core_len, d_core_lits, core_stride};
    return cs_solve_device("satmi_cdcl_assume_batch_device", &as, nullptr, nullptr, num_instances, d_inst_clause_begin,
                           d_clause_lit_begin, d_lits, d_inst_nvars, max_vars, max_clause_len, conflict_limit,
                           time_limit_s, d_lemmas, d_lemma_begin, d_status, d_counters, d_row_len, d_row_lits, stride,
                           d_info, stream);
}

extern "C" int satmi_cdcl_carry_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                             const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                             const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                             int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                             const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                             int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                             const int32_t *d_assume_begin, const int32_t *d_assume_lits,
                                             int32_t *d_core_len, int32_t *d_core_lits, int core_stride,
                                             const int64_t *d_carry_in, int64_t *d_carry_out, void *stream) {
    const CsAssumeIo as{d_assume_begin, d_assume_lits, d_core_len, d_core_lits, core_stride};
    const CsCarryDev cy{d_carry_in, d_carry_out};
    return cs_solve_device("satmi_cdcl_carry_batch_device", &as, &cy, nullptr, num_instances, d_inst_clause_begin,
                           d_clause_lit_begin, d_lits, d_inst_nvars, max_vars, max_clause_len, conflict_limit,
                           time_limit_s, d_lemmas, d_lemma_begin, d_status, d_counters, d_row_len, d_row_lits, stride,
                           d_info, stream);
}

extern "C" int satmi_cdcl_shrink_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                              const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                              const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                              int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                              const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                              int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                              const int32_t *d_assume_begin, const int32_t *d_assume_lits,
                                              int32_t *d_core_len, int32_t *d_core_lits, int core_stride,
                                              const int64_t *d_carry_in, int64_t *d_carry_out, int32_t *d_work_lits,
                                              int64_t *d_shrink_info, void *stream) {
    const CsAssumeIo as{d_assume_begin, d_assume_lits, d_core_len, d_core_lits, core_stride};
    const CsCarryDev cy{d_carry_in, d_carry_out};
    const CsShrinkDev sk{d_work_lits, d_shrink_info};
    return cs_solve_device("satmi_cdcl_shrink_batch_device", &as, &cy, &sk, num_instances, d_inst_clause_begin,
                           d_clause_lit_begin, d_lits, d_inst_nvars, max_vars, max_clause_len, conflict_limit,
                           time_limit_s, d_lemmas, d_lemma_begin, d_status, d_counters, d_row_len, d_row_lits, stride,
                           d_info, stream);
}

extern "C" int satmi_cdcl_carry_pack_device(int num_instances, const int32_t *d_lemmas, const int64_t *d_lemma_begin,
                                            const int64_t *d_carry, int32_t *d_kept_inst_begin,
                                            int32_t *d_kept_clause_begin, int64_t kept_clause_cap,
                                            int32_t *d_kept_lits, int64_t kept_lit_cap, int64_t *d_totals,
                                            void *stream) {
    const char *who = "satmi_cdcl_carry_pack_device";
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (kept_clause_cap < 0 || kept_lit_cap < 0) return fail_arg(who, "negative kept capacity");
    if (num_instances == 0) return SATMI_OK;
    if (!d_lemmas || !d_lemma_begin || !d_carry || !d_kept_inst_begin || !d_kept_clause_begin || !d_kept_lits ||
        !d_totals)
        return fail_arg(who, "null pointer");
    CsCarryPack P{};
    P.lemmas = d_lemmas;
    P.lemma_begin = d_lemma_begin;
    P.carry = d_carry;
    P.kib = d_kept_inst_begin;
    P.kcb = d_kept_clause_begin;
    P.klits = d_kept_lits;
    P.clause_cap = kept_clause_cap;
    P.lit_cap = kept_lit_cap;
    P.totals = d_totals;
    P.num_instances = num_instances;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cdcl_carry_pack_scan_kernel, dim3(1), dim3(64), 0, s, P);
    SATMI_HIP(hipGetLastError());
    const int wgs = std::min((num_instances + 3) / 4, 8192);
    hipLaunchKernelGGL(cdcl_carry_pack_copy_kernel, dim3(wgs), dim3(256), 0, s, P);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

extern "C" int satmi_cdcl_sound_pack_device(int num_instances, const int32_t *d_status, const int32_t *d_lemmas,
                                            const int64_t *d_lemma_begin, int64_t *d_info,
                                            int32_t *d_proof_inst_begin, int32_t *d_proof_clause_begin,
                                            int64_t proof_clause_cap, int32_t *d_proof_lits, int64_t proof_lit_cap,
                                            int64_t *d_totals, void *stream) {
    return cs_pack_device("satmi_cdcl_sound_pack_device", false, num_instances, d_status, d_lemmas, d_lemma_begin,
                          d_info, d_proof_inst_begin, d_proof_clause_begin, proof_clause_cap, d_proof_lits,
                          proof_lit_cap, d_totals, stream);
}

extern "C" int satmi_cdcl_assume_pack_device(int num_instances, const int32_t *d_status, const int32_t *d_lemmas,
                                             const int64_t *d_lemma_begin, int64_t *d_info,
                                             int32_t *d_proof_inst_begin, int32_t *d_proof_clause_begin,
                                             int64_t proof_clause_cap, int32_t *d_proof_lits, int64_t proof_lit_cap,
                                             int64_t *d_totals, void *stream) {
    return cs_pack_device("satmi_cdcl_assume_pack_device", true, num_instances, d_status, d_lemmas, d_lemma_begin,
                          d_info, d_proof_inst_begin, d_proof_clause_begin, proof_clause_cap, d_proof_lits,
                          proof_lit_cap, d_totals, stream);
}

namespace {

// The carried lemmas and the kept output of satmi_cdcl_carry_batch_host, both clause triples.
struct CsCarryIo {
    const int32_t *cib, *ccb, *clits;
    int32_t *kib, *kcb;
    int64_t kclause_cap;
    int32_t *klits;
    int64_t klit_cap;
};

// The host forms: `as` = nullptr is satmi_cdcl_sound_batch_host, else its host arrays;
// `cy` (with `as`) is satmi_cdcl_carry_batch_host, whose h_totals has four words;
// `shrink` (with both) is satmi_cdcl_shrink_batch_host, which fills h_shrink_info.
int cs_batch_host(const char *who, const OomText *oom, const CsAssumeIo *as, const CsCarryIo *cy, bool shrink,
                  int64_t *h_shrink_info, int num_instances,
                  const int32_t *h_inst_clause_begin, const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                  const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s, int64_t room_cap,
                  int32_t *h_status, int64_t *h_counters, int32_t *h_row_len, int32_t *h_row_lits, int stride,
                  int32_t *h_proof_inst_begin, int32_t *h_proof_clause_begin, int64_t proof_clause_cap,
                  int32_t *h_proof_lits, int64_t proof_lit_cap, int64_t *h_info, int64_t *h_totals) {
    // ---- check: all of it before any HIP call
    CsrShape sh;
    std::vector<int32_t> nv((size_t)std::max(num_instances, 0));
    const char *own = proof_clause_cap < 1 || proof_lit_cap < 1 ? "non-positive proof capacity"
                      : room_cap < 0                            ? "negative room_cap"
                      : stride < 1                              ? "row stride < 1"
                      : as && as->core_stride < 0               ? "negative core_stride"
                      : cy && (cy->kclause_cap < 0 || cy->klit_cap < 0) ? "negative kept capacity"
                                                                : nullptr;
    // (the kept arrays: all three, or none of them and no capacity)
    const bool kept = cy && (cy->kib || cy->kcb || cy->klits || cy->kclause_cap > 0 || cy->klit_cap > 0);
    const bool outs = h_inst_nvars && h_status && h_counters && h_row_len && h_row_lits && h_proof_inst_begin &&
                      h_proof_clause_begin && h_proof_lits && h_totals &&
                      (!as || (as->begin && as->core_len && (as->core_stride == 0 || as->core_lits))) &&
                      (!kept || (cy->kib && cy->kcb && cy->klits)) && (!shrink || h_shrink_info);
    if (const char *bad = batch_csr_check(num_instances, h_inst_clause_begin, h_clause_lit_begin, h_lits, own, outs,
                                          &sh, nv.data()))
        return fail_arg(who, bad);
    if (num_instances == 0) return SATMI_OK;
    const int C = sh.C, Ltot = (int)sh.Ltot;
    int max_vars = 0;
    for (int b = 0; b < num_instances; ++b) {
        if (h_inst_nvars[b] < 0) return fail_arg(who, "negative inst_nvars");
        if (nv[(size_t)b] > h_inst_nvars[b]) return fail_arg(who, "literal beyond inst_nvars");
        max_vars = std::max(max_vars, h_inst_nvars[b]);
    }
    if (stride < max_vars) return fail_arg(who, "row stride < number of variables");
    if (proof_clause_cap > INT32_MAX - 1 || proof_lit_cap > INT32_MAX)
        return fail_arg(who, "proof capacity beyond the 32-bit offsets of the proof arrays");
    int Atot = 0;
    if (as) {   // the assumption ranges, as satmi_dpll_batch_host checks its init ranges
        if (as->begin[0] < 0) return fail_arg(who, "assumption ranges are not ascending");
        for (int b = 0; b < num_instances; ++b)
            if (as->begin[b + 1] < as->begin[b]) return fail_arg(who, "assumption ranges are not ascending");
        Atot = as->begin[num_instances];
        if (Atot > 0 && !as->lits) return fail_arg(who, "null pointer");
        for (int b = 0; b < num_instances; ++b)
            for (int i = as->begin[b]; i < as->begin[b + 1]; ++i) {
                const int32_t x = as->lits[i];
                if (x == 0 || x == INT32_MIN) return fail_arg(who, "assumption literal 0 / INT32_MIN");
                if (std::abs(x) > h_inst_nvars[b]) return fail_arg(who, "assumption literal beyond inst_nvars");
            }
    }
    int64_t image_words = 0;
    if (cy) {
        if (cy->kclause_cap > INT32_MAX - 1 || cy->klit_cap > INT32_MAX)
            return fail_arg(who, "kept capacity beyond the 32-bit offsets of the kept arrays");
        if (const char *bad = carry_triple_check(num_instances, cy->cib, cy->ccb, cy->clits, h_inst_nvars, &image_words))
            return fail_arg(who, bad);
    }
    if (max_vars > SATMI_CDCL_SOUND_MAX_VARS) return cs_too_large(who, max_vars);

    // ---- lease the workspace
    int dev = 0;
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts, &dev));
    Lease<CdclSoundWork> lease{Pool<CdclSoundWork>::get().acquire(dev)};
    if (!lease.w) {
        set_error(std::string(who) + ": hipStreamCreate failed");
        return SATMI_ERR_HIP;
    }
    CdclSoundWork &wk = *lease.w;
    hipStream_t s = wk.stream;
    // ---- carve one block: the batch, the solve's outputs, the region ranges, the proof
    const size_t B = (size_t)num_instances;
    Carve cv;
    const size_t o_icb = cv.take(4 * (B + 1));
    const size_t o_clb = cv.take(4 * (size_t)(C + 1));
    const size_t o_lits = cv.take(4 * (size_t)std::max(Ltot, 1));
    const size_t o_nv = cv.take(4 * B);
    const size_t o_st = cv.take(4 * B);
    const size_t o_ctr = cv.take(8 * B * SATMI_CDCL_SOUND_NCOUNTERS);
    const size_t o_rl = cv.take(4 * B);
    const size_t o_row = cv.take(4 * B * (size_t)stride);
    const size_t o_lb = cv.take(8 * (B + 1));
    const size_t o_info = cv.take(8 * B * SATMI_CDCL_SOUND_NWORDS);
    const size_t o_tot = cv.take(16);
    const size_t o_pib = cv.take(4 * (B + 1));
    const size_t o_pcb = cv.take(4 * ((size_t)proof_clause_cap + 1));
    const size_t o_plits = cv.take(4 * (size_t)proof_lit_cap);
    const size_t cstride = as ? (size_t)as->core_stride : 0;
    const size_t o_ab = as ? cv.take(4 * (B + 1)) : 0;
    const size_t o_al = as ? cv.take(4 * (size_t)std::max(Atot, 1)) : 0;
    const size_t o_cl = as ? cv.take(4 * B) : 0;
    const size_t o_core = as ? cv.take(4 * std::max<size_t>(B * cstride, 1)) : 0;
    const size_t kccap = cy ? (size_t)cy->kclause_cap : 0, klcap = cy ? (size_t)cy->klit_cap : 0;
    const size_t o_cin = cy ? cv.take(16 * B) : 0;        // the carried counts, read by every run
    const size_t o_cout = cy ? cv.take(16 * B) : 0;       // the kept counts of the last run
    const size_t o_cbeg = cy ? cv.take(8 * (B + 1)) : 0;
    const size_t o_cimg = cy ? cv.take(4 * (size_t)std::max<int64_t>(image_words, 1)) : 0;
    const size_t o_ktot = cy ? cv.take(16) : 0;
    const size_t o_kib = cy ? cv.take(4 * (B + 1)) : 0;
    const size_t o_kcb = cy ? cv.take(4 * (kccap + 1)) : 0;
    const size_t o_klits = cy ? cv.take(4 * std::max<size_t>(klcap, 1)) : 0;
    const size_t o_work = shrink ? cv.take(8 * (size_t)std::max(Atot, 1)) : 0;   // two words per assumption
    const size_t o_sinfo = shrink ? cv.take(8 * B * SATMI_CDCL_SHRINK_NWORDS) : 0;
    SATMI_TRY(wk.block.reserve(cv.at, oom));
    const Staged d{wk.block.as<unsigned char>(), s};
    SATMI_TRY(d.up(o_icb, h_inst_clause_begin, 4 * (B + 1)));
    SATMI_TRY(d.up(o_clb, h_clause_lit_begin, 4 * (size_t)(C + 1)));
    SATMI_TRY(d.up(o_lits, h_lits, 4 * (size_t)Ltot));
    SATMI_TRY(d.up(o_nv, h_inst_nvars, 4 * B));
    SATMI_HIP(hipMemsetAsync(d.at<int32_t>(o_row), 0, 4 * B * (size_t)stride, s));   // the words behind a row's length read 0
    CsAssumeIo das{};
    if (as) {
        SATMI_TRY(d.up(o_ab, as->begin, 4 * (B + 1)));
        SATMI_TRY(d.up(o_al, as->lits, 4 * (size_t)Atot));
        if (cstride) SATMI_HIP(hipMemsetAsync(d.at<int32_t>(o_core), 0, 4 * B * cstride, s));   // likewise behind a core's length
        das = CsAssumeIo{d.at<const int32_t>(o_ab), d.at<const int32_t>(o_al), d.at<int32_t>(o_cl),
                         d.at<int32_t>(o_core), as->core_stride};
    }

    // ---- the carried records, laid out in pinned memory: one upload each of image, ranges and counts
    std::vector<int64_t> carried(B, 0);   // words per instance
    CsCarryDev dcy{};
    if (cy) {
        const size_t img = 4 * (size_t)image_words, beg = 8 * (B + 1), cnt = 16 * B;
        const size_t at_beg = (img + 7) & ~(size_t)7, at_cnt = at_beg + beg;
        SATMI_TRY(wk.carry_h.reserve(at_cnt + cnt));
        int64_t *hb = (int64_t *)(wk.carry_h.p + at_beg), *hc = (int64_t *)(wk.carry_h.p + at_cnt);
        carry_records_layout(num_instances, cy->cib, cy->ccb, cy->clits, hb, (int32_t *)wk.carry_h.p, hc);
        for (size_t b = 0; b < B; ++b) carried[b] = hc[2 * b + 1];
        SATMI_TRY(d.up(o_cimg, wk.carry_h.p, img));
        SATMI_TRY(d.up(o_cbeg, hb, beg));
        SATMI_TRY(d.up(o_cin, hc, cnt));
        dcy = CsCarryDev{d.at<const int64_t>(o_cin), d.at<int64_t>(o_cout)};
    }
    const CsShrinkDev dsk{shrink ? d.at<int32_t>(o_work) : nullptr, shrink ? d.at<int64_t>(o_sinfo) : nullptr};

    // ---- solve; again with four times the room for the instances that ended FULL, up to the caller's cap
    const int64_t dbg_room = g_cs_room.load();
    const int64_t cap = room_cap > 0 ? room_cap : (int64_t)INT32_MAX - sh.max_clauses - 1;
    const int64_t first = dbg_room > 0 ? dbg_room
                                       : std::min<int64_t>(65536, std::max<int64_t>(256, ((int64_t)16 << 20) / (int64_t)B));
    std::vector<int64_t> room(B, std::min(first, cap));
    for (size_t b = 0; b < B; ++b) room[b] = std::min(carried[b] + first, cap);   // (the carried words, then the usual room)
    std::vector<int64_t> lb(B + 1), info(B * SATMI_CDCL_SOUND_NWORDS);
    std::vector<int32_t> status(B);
    for (int round = 0; round < 32; ++round) {
        lb[0] = 0;
        for (size_t b = 0; b < B; ++b) lb[b + 1] = lb[b] + room[b];
        SATMI_TRY(wk.lemmas.reserve(4 * (size_t)std::max<int64_t>(lb[B], 1), oom));
        SATMI_TRY(d.up(o_lb, lb.data(), 8 * (B + 1)));
        if (cy && image_words > 0) {   // every run starts from the input carry
            hipLaunchKernelGGL(cdcl_carry_place_kernel, dim3(std::min((num_instances + 3) / 4, 8192)), dim3(256), 0, s,
                               d.at<const int32_t>(o_cimg), d.at<const int64_t>(o_cbeg), wk.lemmas.as<int32_t>(),
                               d.at<const int64_t>(o_lb), num_instances);
            SATMI_HIP(hipGetLastError());
        }
        SATMI_TRY(cs_solve_device(
            shrink ? "satmi_cdcl_shrink_batch_device"
            : cy   ? "satmi_cdcl_carry_batch_device"
            : as   ? "satmi_cdcl_assume_batch_device"
                   : "satmi_cdcl_sound_batch_device",
            as ? &das : nullptr, cy ? &dcy : nullptr, shrink ? &dsk : nullptr, num_instances, d.at<const int32_t>(o_icb), d.at<const int32_t>(o_clb), d.at<const int32_t>(o_lits),
            d.at<const int32_t>(o_nv), max_vars, C > 0 ? sh.max_len : 0, conflict_limit, time_limit_s,
            wk.lemmas.as<int32_t>(), d.at<const int64_t>(o_lb), d.at<int32_t>(o_st), d.at<int64_t>(o_ctr),
            d.at<int32_t>(o_rl), d.at<int32_t>(o_row), stride, d.at<int64_t>(o_info), s));
        SATMI_TRY(d.down(status.data(), o_st, 4 * B));
        SATMI_HIP(hipStreamSynchronize(s));
        bool again = false;
        for (size_t b = 0; b < B; ++b)
            if (status[b] == SATMI_CDCL_SOUND_FULL && room[b] < cap) {
                room[b] = std::min(cap, std::max<int64_t>(4 * room[b], 4));
                again = true;
            }
        if (!again) break;
    }
    SATMI_TRY(cs_pack_device(as ? "satmi_cdcl_assume_pack_device" : "satmi_cdcl_sound_pack_device", as != nullptr,
                             num_instances, d.at<const int32_t>(o_st), wk.lemmas.as<const int32_t>(),
                             d.at<const int64_t>(o_lb), d.at<int64_t>(o_info), d.at<int32_t>(o_pib),
                             d.at<int32_t>(o_pcb), proof_clause_cap, d.at<int32_t>(o_plits), proof_lit_cap,
                             d.at<int64_t>(o_tot), s));
    int64_t totals[4] = {0, 0, 0, 0};
    if (cy) {
        SATMI_TRY(satmi_cdcl_carry_pack_device(num_instances, wk.lemmas.as<const int32_t>(), d.at<const int64_t>(o_lb),
                                               d.at<const int64_t>(o_cout), d.at<int32_t>(o_kib), d.at<int32_t>(o_kcb),
                                               cy->kclause_cap, d.at<int32_t>(o_klits), cy->klit_cap,
                                               d.at<int64_t>(o_ktot), s));
        SATMI_TRY(d.down(totals + 2, o_ktot, 16));
        if (kept) SATMI_TRY(d.down(cy->kib, o_kib, 4 * (B + 1)));
    }
    // ---- copy back
    SATMI_TRY(d.down(totals, o_tot, 16));
    SATMI_TRY(d.down(info.data(), o_info, 8 * B * SATMI_CDCL_SOUND_NWORDS));
    SATMI_TRY(d.down(h_counters, o_ctr, 8 * B * SATMI_CDCL_SOUND_NCOUNTERS));
    SATMI_TRY(d.down(h_row_len, o_rl, 4 * B));
    SATMI_TRY(d.down(h_row_lits, o_row, 4 * B * (size_t)stride));
    SATMI_TRY(d.down(h_proof_inst_begin, o_pib, 4 * (B + 1)));
    if (as) {
        SATMI_TRY(d.down(as->core_len, o_cl, 4 * B));
        SATMI_TRY(d.down(as->core_lits, o_core, 4 * B * cstride));
    }
    if (shrink) SATMI_TRY(d.down(h_shrink_info, o_sinfo, 8 * B * SATMI_CDCL_SHRINK_NWORDS));
    SATMI_HIP(hipStreamSynchronize(s));
    lease.ok = true;   // the stream is drained; the next call trusts nothing of the workspace
    const bool fits = totals[0] <= proof_clause_cap && totals[1] <= proof_lit_cap;
    // (totals that do not fit: no instance has a lemma, and proof_clause_begin is its first word)
    SATMI_TRY(d.down(h_proof_clause_begin, o_pcb, 4 * (size_t)((fits ? totals[0] : 0) + 1)));
    SATMI_TRY(d.down(h_proof_lits, o_plits, fits ? 4 * (size_t)totals[1] : 0));
    if (kept) {
        const bool kfits = totals[2] <= cy->kclause_cap && totals[3] <= cy->klit_cap;
        SATMI_TRY(d.down(cy->kcb, o_kcb, 4 * (size_t)((kfits ? totals[2] : 0) + 1)));
        SATMI_TRY(d.down(cy->klits, o_klits, kfits ? 4 * (size_t)totals[3] : 0));
    }
    SATMI_HIP(hipStreamSynchronize(s));
    std::memcpy(h_status, status.data(), 4 * B);
    if (h_info) std::memcpy(h_info, info.data(), 8 * B * SATMI_CDCL_SOUND_NWORDS);
    h_totals[0] = totals[0];
    h_totals[1] = totals[1];
    if (cy) h_totals[2] = totals[2], h_totals[3] = totals[3];
    if (wk.lemmas.cap > ((size_t)256 << 20)) wk.lemmas.release();   // large regions are not kept in the pool
    return SATMI_OK;
}

}  // namespace

extern "C" int satmi_cdcl_sound_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                           const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                           const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                           int64_t room_cap, int32_t *h_status, int64_t *h_counters,
                                           int32_t *h_row_len, int32_t *h_row_lits, int stride,
                                           int32_t *h_proof_inst_begin, int32_t *h_proof_clause_begin,
                                           int64_t proof_clause_cap, int32_t *h_proof_lits, int64_t proof_lit_cap,
                                           int64_t *h_info, int64_t *h_totals) {
    return cs_batch_host("satmi_cdcl_sound_batch_host", &CS_OOM, nullptr, nullptr, false, nullptr, num_instances, h_inst_clause_begin,
                         h_clause_lit_begin, h_lits, h_inst_nvars, conflict_limit, time_limit_s, room_cap, h_status,
                         h_counters, h_row_len, h_row_lits, stride, h_proof_inst_begin, h_proof_clause_begin,
                         proof_clause_cap, h_proof_lits, proof_lit_cap, h_info, h_totals);
}

extern "C" int satmi_cdcl_assume_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                            const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                            const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                            int64_t room_cap, int32_t *h_status, int64_t *h_counters,
                                            int32_t *h_row_len, int32_t *h_row_lits, int stride,
                                            int32_t *h_proof_inst_begin, int32_t *h_proof_clause_begin,
                                            int64_t proof_clause_cap, int32_t *h_proof_lits, int64_t proof_lit_cap,
                                            int64_t *h_info, int64_t *h_totals, const int32_t *h_assume_begin,
                                            const int32_t *h_assume_lits, int32_t *h_core_len, int32_t *h_core_lits,
                                            int core_stride) {
    const CsAssumeIo as{h_assume_begin, h_assume_lits, h_core_len, h_core_lits, core_stride};
    return cs_batch_host("satmi_cdcl_assume_batch_host", &CS_ASSUME_OOM, &as, nullptr, false, nullptr, num_instances, h_inst_clause_begin,
                         h_clause_lit_begin, h_lits, h_inst_nvars, conflict_limit, time_limit_s, room_cap, h_status,
                         h_counters, h_row_len, h_row_lits, stride, h_proof_inst_begin, h_proof_clause_begin,
                         proof_clause_cap, h_proof_lits, proof_lit_cap, h_info, h_totals);
}

extern "C" int satmi_cdcl_carry_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                           const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                           const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                           int64_t room_cap, int32_t *h_status, int64_t *h_counters,
                                           int32_t *h_row_len, int32_t *h_row_lits, int stride,
                                           int32_t *h_proof_inst_begin, int32_t *h_proof_clause_begin,
                                           int64_t proof_clause_cap, int32_t *h_proof_lits, int64_t proof_lit_cap,
                                           int64_t *h_info, int64_t *h_totals, const int32_t *h_assume_begin,
                                           const int32_t *h_assume_lits, int32_t *h_core_len, int32_t *h_core_lits,
                                           int core_stride, const int32_t *h_carry_inst_begin,
                                           const int32_t *h_carry_clause_begin, const int32_t *h_carry_lits,
                                           int32_t *h_kept_inst_begin, int32_t *h_kept_clause_begin,
                                           int64_t kept_clause_cap, int32_t *h_kept_lits, int64_t kept_lit_cap) {
    const CsAssumeIo as{h_assume_begin, h_assume_lits, h_core_len, h_core_lits, core_stride};
    const CsCarryIo cy{h_carry_inst_begin, h_carry_clause_begin, h_carry_lits, h_kept_inst_begin,
                       h_kept_clause_begin, kept_clause_cap, h_kept_lits, kept_lit_cap};
    return cs_batch_host("satmi_cdcl_carry_batch_host", &CS_CARRY_OOM, &as, &cy, false, nullptr, num_instances, h_inst_clause_begin,
                         h_clause_lit_begin, h_lits, h_inst_nvars, conflict_limit, time_limit_s, room_cap, h_status,
                         h_counters, h_row_len, h_row_lits, stride, h_proof_inst_begin, h_proof_clause_begin,
                         proof_clause_cap, h_proof_lits, proof_lit_cap, h_info, h_totals);
}

extern "C" int satmi_cdcl_shrink_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                            const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                            const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                            int64_t room_cap, int32_t *h_status, int64_t *h_counters,
                                            int32_t *h_row_len, int32_t *h_row_lits, int stride,
                                            int32_t *h_proof_inst_begin, int32_t *h_proof_clause_begin,
                                            int64_t proof_clause_cap, int32_t *h_proof_lits, int64_t proof_lit_cap,
                                            int64_t *h_info, int64_t *h_totals, const int32_t *h_assume_begin,
                                            const int32_t *h_assume_lits, int32_t *h_core_len, int32_t *h_core_lits,
                                            int core_stride, const int32_t *h_carry_inst_begin,
                                            const int32_t *h_carry_clause_begin, const int32_t *h_carry_lits,
                                            int32_t *h_kept_inst_begin, int32_t *h_kept_clause_begin,
                                            int64_t kept_clause_cap, int32_t *h_kept_lits, int64_t kept_lit_cap,
                                            int64_t *h_shrink_info) {
    const CsAssumeIo as{h_assume_begin, h_assume_lits, h_core_len, h_core_lits, core_stride};
    const CsCarryIo cy{h_carry_inst_begin, h_carry_clause_begin, h_carry_lits, h_kept_inst_begin,
                       h_kept_clause_begin, kept_clause_cap, h_kept_lits, kept_lit_cap};
    return cs_batch_host("satmi_cdcl_shrink_batch_host", &CS_SHRINK_OOM, &as, &cy, true, h_shrink_info, num_instances,
                         h_inst_clause_begin, h_clause_lit_begin, h_lits, h_inst_nvars, conflict_limit, time_limit_s,
                         room_cap, h_status, h_counters, h_row_len, h_row_lits, stride, h_proof_inst_begin,
                         h_proof_clause_begin, proof_clause_cap, h_proof_lits, proof_lit_cap, h_info, h_totals);
}
