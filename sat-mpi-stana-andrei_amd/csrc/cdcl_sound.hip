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

template <bool LONG>
__global__ void __launch_bounds__(256) cdcl_sound_kernel(CsArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cs_lds[];
    const int ln = lane_id(), wv = (int)threadIdx.x >> 6, wpg = (int)blockDim.x >> 6;
    const uint64_t lt = lanemask_lt();
    CsWave w;
    {
        uint32_t *base = cs_lds + (size_t)wv * A.region_words;
        w.reason = (int32_t *)base;
        w.seen = base + cs_reason_words(A.max_vars);
        w.level = (uint16_t *)(w.seen + cs_seen_words(A.max_vars));
        w.trail = w.level + 2u * cs_half_words(A.max_vars);
        w.act = w.trail + 2u * cs_half_words(A.max_vars);
        w.flags = (uint8_t *)(w.act + 2u * cs_half_words(A.max_vars));
    }
    w.lits = A.lits;
    const int64_t W = (int64_t)gridDim.x * wpg;
    for (int64_t b = (int64_t)blockIdx.x * wpg + wv; b < A.num_instances; b += W) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        const int c0 = A.icb[b];
        w.m = A.icb[b + 1] - c0;
        w.fclb = A.clb + c0;
        w.nv = A.nvars[b];
        const int64_t lb = A.lemma_begin[b];
        w.rec = A.lemmas + lb;
        w.room = max((int64_t)0, A.lemma_begin[b + 1] - lb);
        w.used = 0;
        w.trail_len = w.ncand = w.cur = 0;
        int status = CS_RUNNING;
        int64_t conflicts = 0, decisions = 0, props = 0, rounds = 0, learned = 0, learned_lits = 0, top = 0;
        int64_t records = 0, words = 0;   // what the search needed of its region, exact
        int row = 0;
        const int ls = w.fclb[0], le = w.fclb[w.m];
        // ---- the instance must fit the layout: no LDS index beyond the region
        {
            bool bad = false;
            for (int j = ls + ln; j < le; j += 64) bad |= cs_var(A.lits[j]) - 1u >= (uint32_t)max(w.nv, 0);
            if (w.nv < 0 || (uint32_t)w.nv > A.max_vars || __ballot(bad) != 0ull) status = SATMI_CDCL_SOUND_TOO_LARGE;
        }
        if (status == CS_RUNNING) {
            for (int v = ln; v <= w.nv; v += 64) {
                w.reason[v] = CS_NONE;
                w.level[v] = 0;
                w.act[v] = 0;
                w.flags[v] = 0;
            }
            for (int t = ln; t < (int)cs_seen_words((uint32_t)w.nv); t += 64) w.seen[t] = 0u;
            wave_sync();
            for (int j = ls + ln; j < le; j += 64) w.flags[cs_var(A.lits[j])] = 8u;   // occurs (every lane the same byte value)
            wave_sync();
        }
        // Every pass of the loop ends the instance, learns a clause (two words of
        // the region at least) or decides (at most nv decisions between conflicts).
        const uint64_t pass_cap = ((uint64_t)w.room / 2u + 2u) * ((uint64_t)max(w.nv, 0) + 2u);
        for (uint64_t pass = 0; status == CS_RUNNING && pass < pass_cap; ++pass) {
            // ---- unit propagation in rounds, to a conflict or the fixpoint
            int confl = -1;
            for (int r = 0; r <= w.nv && confl < 0; ++r) {
                ++rounds;
                w.ncand = 0;
                confl = LONG ? cs_scan_long(w) : cs_scan_short(w);
                if (confl < 0) confl = cs_scan_learned(w);
                if (confl >= 0) {   // nothing is implied in this round
                    for (int i = ln; i < w.ncand; i += 64) w.reason[w.trail[w.trail_len + i] & 0x7FFFu] = CS_NONE;
                    w.ncand = 0;
                    wave_sync();
                    break;
                }
                if (w.ncand == 0) break;   // the fixpoint
                for (int i = ln; i < w.ncand; i += 64) {
                    const uint16_t e = w.trail[w.trail_len + i];
                    const uint32_t v = e & 0x7FFFu;
                    w.flags[v] = (uint8_t)((w.flags[v] & 12u) | ((e & 0x8000u) ? 2u : 1u));
                    w.level[v] = (uint16_t)w.cur;
                }
                w.trail_len += w.ncand;
                props += w.ncand;
                wave_sync();
            }
            const bool late = A.time_limit_ticks && __builtin_amdgcn_s_memrealtime() - t0 > A.time_limit_ticks;
            if (confl >= 0) {
                ++conflicts;
                if (w.cur == 0) {   // UNSAT: the empty clause closes the proof
                    ++records;
                    ++words;
                    if (w.used + 1 <= w.room) {
                        if (ln == 0) w.rec[w.used] = 0;
                        ++w.used;
                        status = SATMI_CDCL_SOUND_UNSAT;
                    } else {
                        status = SATMI_CDCL_SOUND_FULL;
                    }
                    break;
                }
                if ((A.conflict_limit > 0 && conflicts >= A.conflict_limit) || late) {
                    status = SATMI_CDCL_SOUND_LIMIT;
                    break;
                }
                // ---- first-UIP analysis, backwards over the trail
                int counter = 0, nlow = 0, idx = w.trail_len - 1;
                uint32_t pvar = 0;
                uint16_t pe = 0;
                int code = confl;
                bool broken = false;
                for (int step = 0; step <= w.trail_len; ++step) {
                    int len;
                    const int32_t *p = cs_clause(w, code, &len);
                    for (int j0 = 0; j0 < len; j0 += 64) {
                        const int j = j0 + ln;
                        bool at_cur = false, low = false;
                        if (j < len) {
                            const uint32_t v = cs_var(p[j]);
                            const int lv = w.level[v];
                            if (v != pvar && lv > 0) {
                                const uint32_t bit = 1u << (v & 31u);
                                if (!(atomicOr(&w.seen[v >> 5], bit) & bit)) {   // this lane marked it
                                    at_cur = lv == w.cur;
                                    low = !at_cur;
                                }
                            }
                        }
                        counter += __popcll(__ballot(at_cur));
                        nlow += __popcll(__ballot(low));
                    }
                    wave_sync();
                    // the next marked literal down the trail
                    bool found = false;
                    for (; idx >= 0 && !found;) {
                        const int i = idx - ln;
                        const uint64_t sm = __ballot(i >= 0 && cs_seen(w, w.trail[i] & 0x7FFFu));
                        if (sm) {
                            idx -= (int)__builtin_ctzll(sm);
                            found = true;
                        } else {
                            idx -= 64;
                        }
                    }
                    if (!found) {
                        broken = true;
                        break;
                    }
                    pe = (uint16_t)uniform_i32(w.trail[idx]);
                    pvar = pe & 0x7FFFu;
                    if (ln == 0) atomicAnd(&w.seen[pvar >> 5], ~(1u << (pvar & 31u)));
                    wave_sync();
                    --idx;
                    --counter;
                    if (counter <= 0) break;
                    code = uniform_i32(w.reason[pvar]);
                    if (code < 0 || code == CS_NONE) {   // a decision with marks above it: never by the rule
                        broken = true;
                        break;
                    }
                }
                if (broken || counter != 0) {
                    status = SATMI_CDCL_SOUND_LIMIT;
                    break;
                }
                // ---- the learned clause: the asserting literal, then the others down the trail
                const int len = 1 + nlow;
                const int64_t need = 1 + (int64_t)len;
                ++records;
                words += need;
                if (w.used + need > w.room || (int64_t)w.m + w.used + need > (int64_t)INT32_MAX) {
                    status = SATMI_CDCL_SOUND_FULL;   // nothing of the record is written
                    break;
                }
                int32_t *rp = w.rec + w.used;
                if (ln == 0) {
                    rp[0] = len;
                    rp[1] = -cs_dec(pe);
                    ++w.act[pvar];
                }
                int k = 0, bj = 0;
                for (; idx >= 0 && k < nlow; idx -= 64) {
                    const int i = idx - ln;
                    bool s = false;
                    uint16_t e = 0;
                    int lv = 0;
                    if (i >= 0) {
                        e = w.trail[i];
                        const uint32_t v = e & 0x7FFFu;
                        s = cs_seen(w, v);
                        lv = w.level[v];
                    }
                    const uint64_t sm = __ballot(s);
                    if (sm && k == 0) bj = __builtin_amdgcn_readlane(lv, (int)__builtin_ctzll(sm));
                    if (s) {
                        const uint32_t v = e & 0x7FFFu;
                        const int at = k + __popcll(sm & lt);
                        atomicAnd(&w.seen[v >> 5], ~(1u << (v & 31u)));
                        if (at < nlow) rp[2 + at] = -cs_dec(e);   // (every mark is on the trail once: always so)
                        ++w.act[v];
                    }
                    k += __popcll(sm);
                }
                w.used += need;
                ++learned;
                learned_lits += len;
                // ---- backjump: the trail's levels ascend, so what stays is a prefix
                int keep_n = 0;
                for (int i0 = 0; i0 < w.trail_len; i0 += 64) {
                    const int i = i0 + ln;
                    bool keep = false;
                    if (i < w.trail_len) {
                        const uint32_t v = w.trail[i] & 0x7FFFu;
                        keep = w.level[v] <= bj;
                        if (!keep) {
                            const uint32_t f = w.flags[v];
                            w.flags[v] = (uint8_t)((f & 8u) | ((f & 3u) == 1u ? 4u : 0u));   // unassigned, its phase saved
                            w.reason[v] = CS_NONE;
                        }
                    }
                    keep_n += __popcll(__ballot(keep));
                }
                w.trail_len = keep_n;
                w.cur = bj;
                if ((conflicts & 255) == 0)
                    for (int v = 1 + ln; v <= w.nv; v += 64) w.act[v] >>= 1;
                wave_sync();
                continue;
            }
            // ---- decide: the unassigned variable of the formula with the highest activity, the lowest id on a tie
            uint32_t best = 0;
            for (int v0 = 1; v0 <= w.nv; v0 += 64) {
                const int v = v0 + ln;
                if (v <= w.nv) {
                    const uint32_t f = w.flags[v];
                    if ((f & 8u) && !(f & 3u)) best = max(best, ((uint32_t)w.act[v] << 15) | (uint32_t)(32767 - v));
                }
            }
            best = wave_max_u32(best);
            if (best == 0u) {   // SAT: every variable of the formula is assigned
                int k = 0;
                for (int v0 = 1; v0 <= w.nv; v0 += 64) {
                    const int v = v0 + ln;
                    const uint32_t f = v <= w.nv ? w.flags[v] : 0u;
                    const bool occ = (f & 8u) != 0u;
                    const uint64_t om = __ballot(occ);
                    const int at = k + __popcll(om & lt);
                    if (occ && at < A.stride) A.row_lits[b * A.stride + at] = (f & 3u) == 1u ? v : -v;
                    k += __popcll(om);
                }
                row = k;
                status = SATMI_CDCL_SOUND_SAT;
                break;
            }
            if (late) {
                status = SATMI_CDCL_SOUND_LIMIT;
                break;
            }
            {
                const uint32_t v = 32767u - (best & 32767u);
                ++w.cur;
                ++decisions;
                top = max(top, (int64_t)w.cur);
                if (ln == 0) {
                    const uint32_t f = w.flags[v];
                    w.flags[v] = (uint8_t)(f | ((f & 4u) ? 1u : 2u));
                    w.level[v] = (uint16_t)w.cur;
                    w.reason[v] = -1;
                    w.trail[w.trail_len] = (uint16_t)(v | ((f & 4u) ? 0u : 0x8000u));
                }
                ++w.trail_len;
                wave_sync();
            }
        }
        if (status == CS_RUNNING) status = SATMI_CDCL_SOUND_LIMIT;   // the pass bound (never by the rule)
        const bool trunc = status == SATMI_CDCL_SOUND_FULL;
        if (ln == 0) {
            A.status[b] = status;
            A.row_len[b] = row;
        }
        if (ln < SATMI_CDCL_SOUND_NCOUNTERS)
            A.counters[b * SATMI_CDCL_SOUND_NCOUNTERS + ln] = ln == 0   ? conflicts
                                                              : ln == 1 ? decisions
                                                              : ln == 2 ? props
                                                              : ln == 3 ? rounds
                                                              : ln == 4 ? learned
                                                              : ln == 5 ? learned_lits
                                                              : ln == 6 ? top
                                                                        : 0;
        if (ln < SATMI_CDCL_SOUND_NWORDS)
            A.info[b * SATMI_CDCL_SOUND_NWORDS + ln] = ln == 0   ? records
                                                       : ln == 1 ? words
                                                       : ln == 2 ? (trunc ? SATMI_CDCL_SOUND_TRUNCATED : 0)
                                                                 : 0;
        wave_sync();
    }
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

__device__ __forceinline__ void cs_contribution(const CsPack &P, int b, int64_t *n, int64_t *l) {
    const int64_t *w = P.info + (int64_t)b * SATMI_CDCL_SOUND_NWORDS;
    const bool whole = P.status[b] == SATMI_CDCL_SOUND_UNSAT && !(w[2] & SATMI_CDCL_SOUND_TRUNCATED);
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

// One wavefront: the totals, whether they fit, and the offsets by an exclusive
// scan, 64 instances at a time.  Totals that do not fit leave every instance
// with no lemma, as dpll_proof.hip's pack does.
__global__ void __launch_bounds__(64) cdcl_sound_pack_scan_kernel(CsPack P) {
    const int ln = lane_id(), B = P.num_instances;
    int64_t sn = 0, sl = 0;
    for (int b = ln; b < B; b += 64) {
        int64_t n, l;
        cs_contribution(P, b, &n, &l);
        sn += n;
        sl += l;
    }
    const int64_t tn = __shfl(cs_incl_scan64(sn), 63, 64), tl = __shfl(cs_incl_scan64(sl), 63, 64);
    const bool fits = tn <= P.clause_cap && tl <= P.lit_cap && tn <= INT32_MAX - 1 && tl <= INT32_MAX;
    if (ln == 0) {
        P.totals[0] = tn;
        P.totals[1] = tl;
        P.pib[B] = fits ? (int32_t)tn : 0;
        P.pcb[fits ? tn : 0] = fits ? (int32_t)tl : 0;
    }
    int64_t cn = 0, cl = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + ln;
        int64_t n = 0, l = 0;
        if (b < B) cs_contribution(P, b, &n, &l);
        const int64_t in = cs_incl_scan64(n), il = cs_incl_scan64(l);
        if (b < B) {
            P.pib[b] = fits ? (int32_t)(cn + in - n) : 0;
            P.info[(int64_t)b * SATMI_CDCL_SOUND_NWORDS + 3] = fits ? cl + il - l : 0;
        }
        cn += __shfl(in, 63, 64);
        cl += __shfl(il, 63, 64);
    }
}

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

// ------------------------------------------------------------------ host side
namespace {

constexpr OomText CS_OOM{"satmi_cdcl_sound_batch_host", "split the batch"};

std::atomic<int> g_cs_grid{0}, g_cs_wpg{0};      // satmi_cdcl_sound_debug_grid
std::atomic<int64_t> g_cs_room{0};               // satmi_cdcl_sound_debug_room

// The workspace a satmi_cdcl_sound_batch_host call leases: one carved block for
// the batch, the proof and the outputs, and the lemma regions.
struct CdclSoundWork : WorkStream {
    DevBuf block, lemmas;
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

extern "C" int satmi_cdcl_sound_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                             const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                             const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                             int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                             const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                             int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                             void *stream) {
    const char *who = "satmi_cdcl_sound_batch_device";
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (max_vars < 0 || max_clause_len < 0) return fail_arg(who, "negative max_vars / max_clause_len");
    if (stride < 1) return fail_arg(who, "row stride < 1");
    if (num_instances == 0) return SATMI_OK;
    if (!d_inst_clause_begin || !d_clause_lit_begin || !d_lits || !d_inst_nvars || !d_lemmas || !d_lemma_begin ||
        !d_status || !d_counters || !d_row_len || !d_row_lits || !d_info)
        return fail_arg(who, "null pointer");
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
    const void *fn = long_form ? (const void *)cdcl_sound_kernel<true> : (const void *)cdcl_sound_kernel<false>;
    SATMI_TRY(batch_allow_lds(fn, lds_bytes));
    if (long_form)
        hipLaunchKernelGGL(cdcl_sound_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    else
        hipLaunchKernelGGL(cdcl_sound_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

extern "C" int satmi_cdcl_sound_pack_device(int num_instances, const int32_t *d_status, const int32_t *d_lemmas,
                                            const int64_t *d_lemma_begin, int64_t *d_info,
                                            int32_t *d_proof_inst_begin, int32_t *d_proof_clause_begin,
                                            int64_t proof_clause_cap, int32_t *d_proof_lits, int64_t proof_lit_cap,
                                            int64_t *d_totals, void *stream) {
    const char *who = "satmi_cdcl_sound_pack_device";
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
    hipLaunchKernelGGL(cdcl_sound_pack_scan_kernel, dim3(1), dim3(64), 0, s, P);
    SATMI_HIP(hipGetLastError());
    const int wgs = std::min((num_instances + 3) / 4, 8192);
    hipLaunchKernelGGL(cdcl_sound_pack_copy_kernel, dim3(wgs), dim3(256), 0, s, P);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

extern "C" int satmi_cdcl_sound_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                           const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                           const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                           int64_t room_cap, int32_t *h_status, int64_t *h_counters,
                                           int32_t *h_row_len, int32_t *h_row_lits, int stride,
                                           int32_t *h_proof_inst_begin, int32_t *h_proof_clause_begin,
                                           int64_t proof_clause_cap, int32_t *h_proof_lits, int64_t proof_lit_cap,
                                           int64_t *h_info, int64_t *h_totals) {
    const char *who = "satmi_cdcl_sound_batch_host";
    // ---- check: all of it before any HIP call
    CsrShape sh;
    std::vector<int32_t> nv((size_t)std::max(num_instances, 0));
    const char *own = proof_clause_cap < 1 || proof_lit_cap < 1 ? "non-positive proof capacity"
                      : room_cap < 0                            ? "negative room_cap"
                      : stride < 1                              ? "row stride < 1"
                                                                : nullptr;
    const bool outs = h_inst_nvars && h_status && h_counters && h_row_len && h_row_lits && h_proof_inst_begin &&
                      h_proof_clause_begin && h_proof_lits && h_totals;
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
    SATMI_TRY(wk.block.reserve(cv.at, &CS_OOM));
    const Staged d{wk.block.as<unsigned char>(), s};
    SATMI_TRY(d.up(o_icb, h_inst_clause_begin, 4 * (B + 1)));
    SATMI_TRY(d.up(o_clb, h_clause_lit_begin, 4 * (size_t)(C + 1)));
    SATMI_TRY(d.up(o_lits, h_lits, 4 * (size_t)Ltot));
    SATMI_TRY(d.up(o_nv, h_inst_nvars, 4 * B));
    SATMI_HIP(hipMemsetAsync(d.at<int32_t>(o_row), 0, 4 * B * (size_t)stride, s));   // the words behind a row's length read 0

    // ---- solve; again with four times the room for the instances that ended FULL, up to the caller's cap
    const int64_t dbg_room = g_cs_room.load();
    const int64_t cap = room_cap > 0 ? room_cap : (int64_t)INT32_MAX - sh.max_clauses - 1;
    const int64_t first = dbg_room > 0 ? dbg_room
                                       : std::min<int64_t>(65536, std::max<int64_t>(256, ((int64_t)16 << 20) / (int64_t)B));
    std::vector<int64_t> room(B, std::min(first, cap));
    std::vector<int64_t> lb(B + 1), info(B * SATMI_CDCL_SOUND_NWORDS);
    std::vector<int32_t> status(B);
    for (int round = 0; round < 32; ++round) {
        lb[0] = 0;
        for (size_t b = 0; b < B; ++b) lb[b + 1] = lb[b] + room[b];
        SATMI_TRY(wk.lemmas.reserve(4 * (size_t)std::max<int64_t>(lb[B], 1), &CS_OOM));
        SATMI_TRY(d.up(o_lb, lb.data(), 8 * (B + 1)));
        SATMI_TRY(satmi_cdcl_sound_batch_device(
            num_instances, d.at<const int32_t>(o_icb), d.at<const int32_t>(o_clb), d.at<const int32_t>(o_lits),
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
    SATMI_TRY(satmi_cdcl_sound_pack_device(num_instances, d.at<const int32_t>(o_st), wk.lemmas.as<const int32_t>(),
                                           d.at<const int64_t>(o_lb), d.at<int64_t>(o_info), d.at<int32_t>(o_pib),
                                           d.at<int32_t>(o_pcb), proof_clause_cap, d.at<int32_t>(o_plits),
                                           proof_lit_cap, d.at<int64_t>(o_tot), s));
    // ---- copy back
    int64_t totals[2] = {0, 0};
    SATMI_TRY(d.down(totals, o_tot, 16));
    SATMI_TRY(d.down(info.data(), o_info, 8 * B * SATMI_CDCL_SOUND_NWORDS));
    SATMI_TRY(d.down(h_counters, o_ctr, 8 * B * SATMI_CDCL_SOUND_NCOUNTERS));
    SATMI_TRY(d.down(h_row_len, o_rl, 4 * B));
    SATMI_TRY(d.down(h_row_lits, o_row, 4 * B * (size_t)stride));
    SATMI_TRY(d.down(h_proof_inst_begin, o_pib, 4 * (B + 1)));
    SATMI_HIP(hipStreamSynchronize(s));
    lease.ok = true;   // the stream is drained; the next call trusts nothing of the workspace
    const bool fits = totals[0] <= proof_clause_cap && totals[1] <= proof_lit_cap;
    // (totals that do not fit: no instance has a lemma, and proof_clause_begin is its first word)
    SATMI_TRY(d.down(h_proof_clause_begin, o_pcb, 4 * (size_t)((fits ? totals[0] : 0) + 1)));
    SATMI_TRY(d.down(h_proof_lits, o_plits, fits ? 4 * (size_t)totals[1] : 0));
    SATMI_HIP(hipStreamSynchronize(s));
    std::memcpy(h_status, status.data(), 4 * B);
    if (h_info) std::memcpy(h_info, info.data(), 8 * B * SATMI_CDCL_SOUND_NWORDS);
    h_totals[0] = totals[0];
    h_totals[1] = totals[1];
    if (wk.lemmas.cap > ((size_t)256 << 20)) wk.lemmas.release();   // large regions are not kept in the pool
    return SATMI_OK;
}
