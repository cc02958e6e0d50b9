// trim.hip -- batched refutation trimming on gfx950: the backward form of
// refute.hip's check.  For B clause sets, each with an ordered list of lemma
// clauses, one launch finds the first empty lemma of every instance, checks
// only the lemmas that the empty one needs (directly or through other needed
// lemmas), and writes which formula clauses (the UNSAT core) and which lemmas
// (the trimmed proof) the refutation uses.
//
//   * The walk.  Let e be the instance's first empty lemma (none: OPEN, nothing
//     marked).  Le is marked needed, and i runs e, e-1, ..., 0.  A lemma that
//     is not needed is skipped (64 marks are read at a time).  A needed lemma
//     is checked as refute.hip checks it -- its literals false, unit
//     propagation over the formula and the lemmas 0 .. i-1 to a conflict or a
//     fixpoint, bad literals and tautologies treated alike -- and every
//     propagated literal keeps its REASON, the clause that made it unit.  On a
//     conflict the analysis marks the conflict's clause (both reason clauses
//     when a variable is needed with both signs) and, transitively, the reason
//     of every false literal of a marked clause.  A marked formula clause is in
//     the core; a marked lemma is needed and will be checked when the walk
//     reaches it.  A needed lemma that reaches no conflict has failed and marks
//     nothing; a tautological one verifies and marks nothing.
//   * One wavefront per instance, persistent over the batch by fixed stride,
//     workgroups of 4, 2 or 1 waves by LDS residency, two clause forms chosen
//     from max_clause_len: all as in refute.hip.  The device form owns no
//     device memory.
//   * The wave's LDS region:
//       table    2 bits per variable, refute.hip's layout
//       side     1 bit per variable: "on the conflict side" -- a false literal
//                of a marked clause, whose reason the analysis still has to mark
//       trail    16 bits per assigned variable, in assignment order
//       reason   32 bits per trail entry: formula clause c as c, lemma j as
//                m + j, TR_NO_REASON for the lemma's own negated literals
//     At SATMI_TRIM_MAX_VARS = 16,383: 4 + 2 + 32 + 64 = 102 KiB, one to a CU.
//   * The analysis walks the trail from its end in chunks of 64 entries: a
//     ballot finds the entries whose variable is on the conflict side and that
//     have a reason; the highest one's reason clause is marked and read in
//     64-literal steps, its false literals join the side bitmap, and the ballot
//     is taken again over the entries below it.  Runs of unwanted entries cost
//     one ballot per 64.  A reason clause's false literals were assigned before
//     the literal it forced, so one pass from the end reaches them all.
//   * Determinism.  Which core is found depends on the propagation order, so
//     the marks are a function of the inputs and the clause form, and of
//     nothing else: not of the grid, the workgroup width, or which lane's LDS
//     atomic lands first.  In the lane-per-clause form everything a step
//     decides is settled in registers before any atomic: among the lanes that
//     hold the same unit literal the lowest (the lowest clause index) is the
//     leader and alone assigns it; two leaders with opposite literals are a
//     conflict of their two clauses; of several conflicts in one step the
//     lowest lane's is taken; and a step with a conflict assigns nothing.  The
//     leaders of a step without one hold distinct unassigned variables, so each
//     pushes exactly one trail entry, in lane order.  The wave-per-clause form
//     handles one clause at a time.  (The lemma's own literals are assigned
//     with the atomic's answer deciding which copy of a repeated literal
//     pushes; they carry no reason, so their order among themselves is never
//     read.)
//   * After a lemma the table words and the side words of the trail's
//     variables are stored 0: a side bit is only ever set for a false literal,
//     whose variable is on the trail.  Reasons are written with their entries.
//   * The mark arrays are global memory written by some lanes and read later by
//     other lanes of the same wave (tr_marks_visible below).  The kernel
//     initialises its instance's ranges itself: core 0, lemmas -1.
//   * Every loop states its bound in its condition.
//
// Plain C++ and vector memory operations only.  refute.hip's small helpers are
// restated here (tr_var, tr_bad, tr_lookup): the translation unit shares no
// device code with any other, whose machine code stays what it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>

#include "batch_host.h"
#include "common.h"

namespace satmi {

constexpr int TR_SHORT_MAX = 8;                 // longest clause of the lane-per-clause form (refute.hip's)
constexpr uint32_t TR_NO_REASON = 0xFFFFFFFFu;  // an assumption: the lemma's own negated literal
constexpr uint32_t TR_NO_CLAUSE = 0xFFFFFFFFu;
// LDS words of one wave's table, side bitmap, trail (16 bits per variable) and reasons, each a multiple of 4
constexpr uint32_t tr_table_words(uint32_t max_vars) { return ((max_vars >> 4) + 1u + 3u) & ~3u; }
constexpr uint32_t tr_side_words(uint32_t max_vars) { return ((max_vars >> 5) + 1u + 3u) & ~3u; }
constexpr uint32_t tr_trail_words(uint32_t max_vars) { return (((max_vars + 1u) >> 1) + 3u) & ~3u; }
constexpr uint32_t tr_reason_words(uint32_t max_vars) { return (max_vars + 3u) & ~3u; }
constexpr uint32_t tr_region_words(uint32_t max_vars) {
    return tr_table_words(max_vars) + tr_side_words(max_vars) + tr_trail_words(max_vars) + tr_reason_words(max_vars);
}
static_assert(SATMI_TRIM_MAX_VARS <= 0xFFFF, "a trail entry is 16 bits");
static_assert(4u * tr_table_words(SATMI_TRIM_MAX_VARS) == 4u * 1024u && 4u * tr_side_words(SATMI_TRIM_MAX_VARS) == 2u * 1024u &&
                  4u * tr_trail_words(SATMI_TRIM_MAX_VARS) == 32u * 1024u &&
                  4u * tr_reason_words(SATMI_TRIM_MAX_VARS) == 64u * 1024u &&
                  4u * tr_region_words(SATMI_TRIM_MAX_VARS) == 102u * 1024u && 102u * 1024u <= LDS_PER_CU,
              "at the variable limit a region is 4 + 2 + 32 + 64 KiB, one to a CU");

struct TrimArgs {
    const int32_t *icb, *clb, *lits;      // the formulas (CSR)
    const int32_t *pib, *pcb, *plits;     // the proofs (CSR): instance -> lemmas -> literals
    int32_t *out;                         // [B x SATMI_TRIM_NWORDS]
    int32_t *core;                        // [C]
    int32_t *lemma;                       // [P]
    int num_instances;
    uint32_t max_vars;
    uint32_t table_words, side_words, trail_words;   // LDS words of the region's first three parts
    uint32_t region_words;                           // ... of the whole region
};

// A wave's state.  Everything but the pointers' targets is wave-uniform.
struct TrWave {
    uint32_t *table, *side, *reason;
    uint16_t *trail;
    uint32_t max_vars;
    int trail_len;
    bool conflict;
    uint32_t cc0, cc1;   // the conflict's clause; the second reason clause of a both-signs conflict, or TR_NO_CLAUSE
};

// |l| (INT32_MIN: 2^31)
__device__ __forceinline__ uint32_t tr_var(int32_t l) { return l < 0 ? 0u - (uint32_t)l : (uint32_t)l; }
__device__ __forceinline__ bool tr_bad(int32_t l, uint32_t max_vars) { return tr_var(l) - 1u >= max_vars; }

// What the table says of a literal it holds: 0 unassigned, bit 0 = l is true, bit 1 = -l is.
__device__ __forceinline__ uint32_t tr_lookup(const uint32_t *table, int32_t l) {
    const uint32_t v = tr_var(l);
    const uint32_t pair = (table[v >> 4] >> (2u * (v & 15u))) & 3u;
    return l < 0 ? ((pair >> 1) | (pair << 1)) & 3u : pair;
}

// Same-CU visibility of the mark arrays.  A mark is stored by one lane and read
// later by another lane of the same wave.  The rule relied on: a
// workgroup-scope fence is what orders global accesses among the waves of one
// CU (it reaches nothing another CU can observe, and needs nothing more: the
// waves of a CU share its vector L1, through which their stores are written).
// It drains the wave's outstanding vector-memory operations, so every mark
// stored before it is in that L1 before any load after it is issued.  No other
// wave, on this CU or another, reads or writes an instance's marks.
__device__ __forceinline__ void tr_marks_visible() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// The lanes with `on` set their literal `l` (which the table holds) true, with
// reason `r` (per lane).  All 64 lanes call.  Returns, per lane, whether -l was
// true already.  A lane pushes its variable only if its atomic gave the
// variable its first bit, so the trail never holds more than max_vars entries.
__device__ __forceinline__ bool tr_assign(TrWave &w, bool on, int32_t l, uint32_t r) {
    bool opposite = false, fresh = false;
    const uint32_t v = tr_var(l);
    if (on) {
        const uint32_t sh = 2u * (v & 15u) + (l < 0 ? 1u : 0u);
        const uint32_t old = atomicOr(w.table + (v >> 4), 1u << sh);
        opposite = (old >> (sh ^ 1u)) & 1u;
        fresh = ((old >> (sh & ~1u)) & 3u) == 0u;
    }
    const uint64_t fm = __ballot(fresh);
    if (fresh) {
        const int at = w.trail_len + __popcll(fm & lanemask_lt());   // < max_vars: one push per variable
        w.trail[at] = (uint16_t)v;
        w.reason[at] = r;
    }
    w.trail_len += __popcll(fm);
    return opposite;
}

// One propagation round over clauses [0, n) of a clause list, clause c's reason
// word being base + c: lane-per-clause.  Everything a step decides is settled
// in registers before its atomics (see the head of the file).
__device__ __forceinline__ void tr_scan_short(TrWave &w, const int32_t *clb, const int32_t *lits, int n, uint32_t base) {
    const int ln = lane_id();
    for (int cb = 0; cb < n && !w.conflict; cb += 64) {
        const int c = cb + ln;
        bool unit = false, fals = false;
        int32_t u = 0;
        if (c < n) {
            const int s = clb[c], e = clb[c + 1];
            bool sat = false, many = false, have = false;
            for (int j = s; j < e; ++j) {
                const int32_t l = lits[j];
                if (tr_bad(l, w.max_vars)) {
                    sat = true;   // not a premise
                    continue;
                }
                const uint32_t st = tr_lookup(w.table, l);
                sat |= (st & 1u) != 0u;
                if (st == 0u) {
                    many |= have && l != u;
                    if (!have) u = l;
                    have = true;
                }
            }
            fals = !sat && !have;
            unit = !sat && have && !many;
        }
        // ---- leaders: the lowest lane of every unit literal; `clash`: the lowest lane that holds
        // the opposite of this lane's unit literal (64: none).  At most 64 distinct literals.
        bool lead = unit;
        int clash = 64;
        uint64_t rest = __ballot(unit);
        for (int it = 0; it < 64 && rest != 0ull; ++it) {
            const int first = (int)__builtin_ctzll(rest);
            const int32_t ul = __builtin_amdgcn_readlane(u, first);
            const bool same = unit && u == ul;
            if (same && ln != first) lead = false;
            if (unit && u == -ul) clash = first;   // (-ul exists: a unit literal is not INT32_MIN)
            rest &= ~__ballot(same);
        }
        const uint64_t cm = __ballot(fals || (lead && clash < 64));
        if (cm != 0ull) {
            const int at = (int)__builtin_ctzll(cm);   // the lowest clause of the step that conflicts
            const int other = __builtin_amdgcn_readlane(clash, at);
            w.conflict = true;
            w.cc0 = base + (uint32_t)(cb + at);
            // (a falsified clause has no unit literal and its `clash` stayed 64)
            w.cc1 = other < 64 ? base + (uint32_t)(cb + other) : TR_NO_CLAUSE;
        } else {
            tr_assign(w, lead, u, base + (uint32_t)c);   // distinct unassigned variables: every leader pushes
        }
        wave_sync();
    }
}

// The same, the whole wave on one clause at a time.
__device__ __forceinline__ void tr_scan_long(TrWave &w, const int32_t *clb, const int32_t *lits, int n, uint32_t base) {
    const int ln = lane_id();
    for (int c = 0; c < n && !w.conflict; ++c) {
        const int s = uniform_i32(clb[c]), e = uniform_i32(clb[c + 1]);
        bool sat = false, many = false, have = false;   // wave-uniform
        int32_t u = 0;
        for (int j0 = s; j0 < e && !sat; j0 += 64) {
            const int j = j0 + ln;
            bool bad = false, open = false;
            uint32_t st = 2u;   // a lane past the clause's end decides nothing
            int32_t l = 0;
            if (j < e) {
                l = lits[j];
                bad = tr_bad(l, w.max_vars);
                if (!bad) st = tr_lookup(w.table, l);
                open = !bad && st == 0u;
            }
            sat = __ballot(bad || (st & 1u) != 0u) != 0ull;   // a bad literal: not a premise
            const uint64_t om = __ballot(open);
            if (om) {
                if (!have) u = __builtin_amdgcn_readlane(l, (int)__builtin_ctzll(om));
                have = true;
                many |= __ballot(open && l != u) != 0ull;
            }
        }
        if (sat) continue;
        if (!have) {
            w.conflict = true;
            w.cc0 = base + (uint32_t)c;
            w.cc1 = TR_NO_CLAUSE;
        } else if (!many) {
            // (a unit under the table it was read from: -u is not true, so this cannot conflict)
            tr_assign(w, ln == 0, u, base + (uint32_t)c);
            wave_sync();
        }
    }
}

// Mark clause `r` (a reason word: < m a formula clause, else lemma r - m) and put
// its false literals on the conflict side.  Its unassigned literal, if it has
// one (the variable of a both-signs conflict), has no trail entry and gets no bit.
__device__ __forceinline__ void tr_mark(TrWave &w, const TrimArgs &A, uint32_t r, int m, int c0, int p0,
                                        const int32_t *fclb, const int32_t *pclb) {
    const int ln = lane_id();
    const bool is_lemma = r >= (uint32_t)m;
    const int idx = is_lemma ? (int)(r - (uint32_t)m) : (int)r;
    const int32_t *clb = is_lemma ? pclb : fclb;
    const int32_t *lits = is_lemma ? A.plits : A.lits;
    if (ln == 0) (is_lemma ? A.lemma + p0 : A.core + c0)[idx] = 1;
    const int s = uniform_i32(clb[idx]), e = uniform_i32(clb[idx + 1]);
    for (int j = s + ln; j < e; j += 64) {
        const int32_t l = lits[j];
        if (tr_bad(l, w.max_vars)) continue;   // (a premise holds none; the guard keeps the index inside the region)
        if (tr_lookup(w.table, l) == 2u) {
            const uint32_t v = tr_var(l);
            atomicOr(w.side + (v >> 5), 1u << (v & 31u));
        }
    }
    wave_sync();
}

template <bool LONG>
__global__ void __launch_bounds__(256) trim_kernel(TrimArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tr_lds[];
    const int ln = lane_id(), wv = (int)threadIdx.x >> 6, wpg = (int)blockDim.x >> 6;
    TrWave w;
    w.table = tr_lds + (size_t)wv * A.region_words;
    w.side = w.table + A.table_words;
    w.trail = (uint16_t *)(w.side + A.side_words);
    w.reason = w.side + A.side_words + A.trail_words;
    w.max_vars = A.max_vars;
    w.trail_len = 0;
    w.conflict = false;
    w.cc0 = w.cc1 = TR_NO_CLAUSE;
    for (uint32_t t = (uint32_t)ln; t < A.table_words + A.side_words; t += 64u) w.table[t] = 0u;   // table and side, once
    wave_sync();
    const int64_t W = (int64_t)gridDim.x * wpg;
    for (int64_t b = (int64_t)blockIdx.x * wpg + wv; b < A.num_instances; b += W) {
        const int c0 = A.icb[b], m = A.icb[b + 1] - c0;
        const int p0 = A.pib[b], k = A.pib[b + 1] - p0;
        const int32_t *fclb = A.clb + c0, *pclb = A.pcb + p0;
        int32_t *core = A.core + c0, *lemma = A.lemma + p0;
        int flags = 0, failed = 0, first = -1;
        // ---- the instance's marks: nothing in the core, no lemma needed
        for (int t = ln; t < m; t += 64) core[t] = 0;
        for (int t = ln; t < k; t += 64) lemma[t] = -1;
        // ---- bad literals of the formula (its clauses are skipped as premises)
        {
            const int s = fclb[0], e = fclb[m];
            bool bad = false;
            for (int j = s + ln; j < e; j += 64) bad |= tr_bad(A.lits[j], A.max_vars);
            if (__ballot(bad)) flags |= SATMI_REFUTE_BAD_LITERAL;
        }
        // ---- the first empty lemma
        int end = -1;
        for (int j0 = 0; j0 < k && end < 0; j0 += 64) {
            const int j = j0 + ln;
            const uint64_t em = __ballot(j < k && pclb[j + 1] == pclb[j]);
            if (em) end = j0 + (int)__builtin_ctzll(em);
        }
        tr_marks_visible();   // the initial marks before the first one set
        if (end >= 0 && ln == 0) lemma[end] = 1;
        // ---- the walk: i only decreases
        for (int i = end; i >= 0; --i) {
            // the needed lemma nearest below or at i, 64 marks at a time
            tr_marks_visible();
            {
                const int lo = i & ~63, j = lo + ln;
                const uint64_t nm = __ballot(j <= i && lemma[j] >= 0);
                if (nm == 0ull) {
                    i = lo;   // (the loop's step takes it below the chunk)
                    continue;
                }
                i = lo + 63 - (int)__builtin_clzll(nm);
            }
            const int s = uniform_i32(pclb[i]), e = uniform_i32(pclb[i + 1]);
            // ---- every literal of the lemma false
            bool lemma_bad = false, taut = false;
            for (int j0 = s; j0 < e; j0 += 64) {
                const int j = j0 + ln;
                bool bad = false, good = false;
                int32_t l = 0;
                if (j < e) {
                    l = A.plits[j];
                    bad = tr_bad(l, A.max_vars);
                    good = !bad;
                }
                const bool opposite = tr_assign(w, good, good ? -l : 0, TR_NO_REASON);   // (-l exists: l is not INT32_MIN)
                lemma_bad |= __ballot(bad) != 0ull;
                taut |= __ballot(opposite) != 0ull;
            }
            wave_sync();
            if (lemma_bad) flags |= SATMI_REFUTE_BAD_LITERAL;
            if (taut) flags |= SATMI_REFUTE_TAUTOLOGY;
            // ---- unit propagation to a conflict or a fixpoint
            w.conflict = false;
            if (!lemma_bad && !taut) {
                for (uint32_t round = 0; round <= A.max_vars && !w.conflict; ++round) {
                    const int before = w.trail_len;
                    if (LONG) {
                        tr_scan_long(w, fclb, A.lits, m, 0u);
                        tr_scan_long(w, pclb, A.plits, i, (uint32_t)m);
                    } else {
                        tr_scan_short(w, fclb, A.lits, m, 0u);
                        tr_scan_short(w, pclb, A.plits, i, (uint32_t)m);
                    }
                    if (w.trail_len == before) break;   // nothing assigned: the fixpoint
                }
            }
            const bool ok = !lemma_bad && (taut || w.conflict);
            if (!ok) {
                first = i;   // the walk runs downwards: the last one found is the lowest
                ++failed;
                if (ln == 0) lemma[i] = 0;
            }
            // ---- the analysis: the conflict's antecedents, from the trail's end
            if (ok && !taut) {
                tr_mark(w, A, w.cc0, m, c0, p0, fclb, pclb);
                if (w.cc1 != TR_NO_CLAUSE) tr_mark(w, A, w.cc1, m, c0, p0, fclb, pclb);
                for (int hi = w.trail_len; hi > 0; hi -= 64) {
                    const int lo = hi > 64 ? hi - 64 : 0, t = lo + ln;
                    uint32_t v = 0u, r = TR_NO_REASON;
                    if (t < hi) {
                        v = w.trail[t];
                        r = w.reason[t];
                    }
                    int below = 64;   // only the entries under the one just marked can still turn up
                    for (int it = 0; it < 64 && below > 0; ++it) {
                        const bool want = ln < below && r != TR_NO_REASON && ((w.side[v >> 5] >> (v & 31u)) & 1u) != 0u;
                        const uint64_t wm = __ballot(want);
                        if (wm == 0ull) break;
                        below = 63 - (int)__builtin_clzll(wm);
                        tr_mark(w, A, (uint32_t)__builtin_amdgcn_readlane((int)r, below), m, c0, p0, fclb, pclb);
                    }
                }
            }
            // ---- clear what the lemma assigned and what the analysis put on the side
            for (int t = ln; t < w.trail_len; t += 64) {
                const uint32_t v = w.trail[t];
                w.table[v >> 4] = 0u;
                w.side[v >> 5] = 0u;
            }
            w.trail_len = 0;
            wave_sync();
        }
        // ---- the words: the sums of the marks
        tr_marks_visible();
        int ncore = 0, nkept = 0;
        for (int t = ln; t < m; t += 64) ncore += core[t] == 1;
        for (int t = ln; t < k; t += 64) nkept += lemma[t] >= 0;
        ncore = lane63(wave_incl_scan(ncore));
        nkept = lane63(wave_incl_scan(nkept));
        const int status = end < 0 ? SATMI_REFUTE_OPEN : failed ? SATMI_REFUTE_FAILED : SATMI_REFUTE_PROVEN;
        if (ln < SATMI_TRIM_NWORDS)
            A.out[b * SATMI_TRIM_NWORDS + ln] =
                ln == 0 ? status : ln == 1 ? failed : ln == 2 ? first : ln == 3 ? flags : ln == 4 ? ncore : nkept;
    }
}

// ------------------------------------------------------------------ host side
namespace {

constexpr OomText TR_OOM{"satmi_trim_refutations_host", "split the batch"};

std::atomic<int> g_dbg_grid{0}, g_dbg_wpg{0};   // satmi_trim_debug_grid

struct TrimWork : BatchWork {};   // a pool of its own (keys_out, rec_off stay empty)

int too_large(const char *who, int64_t max_vars) {
    set_error(std::string(who) + ": variable " + std::to_string(max_vars) + " is beyond the table's " +
              std::to_string(SATMI_TRIM_MAX_VARS));
    return SATMI_ERR_TOO_LARGE;
}

// One launch on `s`; every argument is checked by the caller.
int trim_launch(const char *who, TrimArgs A, int max_clause_len, hipStream_t s) {
    A.table_words = tr_table_words(A.max_vars);
    A.side_words = tr_side_words(A.max_vars);
    A.trail_words = tr_trail_words(A.max_vars);
    A.region_words = tr_region_words(A.max_vars);
    const size_t region = 4 * (size_t)A.region_words;
    // waves per workgroup: the most waves resident on a CU by LDS, the wider on a tie
    int wpg = g_dbg_wpg;
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
                  std::to_string(A.max_vars) + " variables");
        return SATMI_ERR_TOO_LARGE;
    }
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts));
    const int wgs = (int)(((int64_t)A.num_instances + wpg - 1) / wpg);
    const int grid = batch_grid(facts, lds_bytes, 0, 64 * wpg, wgs, g_dbg_grid);
    const bool long_form = max_clause_len <= 0 || max_clause_len > TR_SHORT_MAX;
    const void *fn = long_form ? (const void *)trim_kernel<true> : (const void *)trim_kernel<false>;
    SATMI_TRY(batch_allow_lds(fn, lds_bytes));
    if (long_form)
        hipLaunchKernelGGL(trim_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    else
        hipLaunchKernelGGL(trim_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

}  // namespace

}  // namespace satmi

using namespace satmi;

extern "C" int satmi_trim_debug_grid(int workgroups, int waves_per_wg) {
    if (workgroups < 0 || !(waves_per_wg == 0 || waves_per_wg == 1 || waves_per_wg == 2 || waves_per_wg == 4))
        return fail_arg("satmi_trim_debug_grid", "workgroups >= 0 and waves_per_wg one of 0, 1, 2, 4");
    g_dbg_grid = workgroups;
    g_dbg_wpg = waves_per_wg;
    return SATMI_OK;
}

extern "C" int satmi_trim_refutations_device(int num_instances, const int32_t *d_inst_clause_begin,
                                             const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                             const int32_t *d_proof_inst_begin, const int32_t *d_proof_clause_begin,
                                             const int32_t *d_proof_lits, int max_vars, int max_clause_len,
                                             int32_t *d_out, int32_t *d_core, int32_t *d_lemma, void *stream) {
    const char *who = "satmi_trim_refutations_device";
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (max_vars < 0 || max_clause_len < 0) return fail_arg(who, "negative max_vars / max_clause_len");
    if (num_instances == 0) return SATMI_OK;
    // (the marks are the walk's own state: the device form needs both arrays)
    if (!d_inst_clause_begin || !d_clause_lit_begin || !d_lits || !d_proof_inst_begin || !d_proof_clause_begin ||
        !d_proof_lits || !d_out || !d_core || !d_lemma)
        return fail_arg(who, "null pointer");
    if (max_vars > SATMI_TRIM_MAX_VARS) return too_large(who, max_vars);
    TrimArgs A{};
    A.icb = d_inst_clause_begin;
    A.clb = d_clause_lit_begin;
    A.lits = d_lits;
    A.pib = d_proof_inst_begin;
    A.pcb = d_proof_clause_begin;
    A.plits = d_proof_lits;
    A.out = d_out;
    A.core = d_core;
    A.lemma = d_lemma;
    A.num_instances = num_instances;
    A.max_vars = (uint32_t)max_vars;
    return trim_launch(who, A, max_clause_len, (hipStream_t)stream);
}

extern "C" int satmi_trim_refutations_host(int num_instances, const int32_t *h_inst_clause_begin,
                                           const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                           const int32_t *h_proof_inst_begin, const int32_t *h_proof_clause_begin,
                                           const int32_t *h_proof_lits, int32_t *h_out, int32_t *h_core,
                                           int32_t *h_lemma) {
    const char *who = "satmi_trim_refutations_host";
    // ---- check: all of it before any HIP call
    CsrShape fs, ps;
    if (const char *bad = batch_csr_check(num_instances, h_inst_clause_begin, h_clause_lit_begin, h_lits, nullptr,
                                          h_out != nullptr, &fs))
        return fail_arg(who, (std::string("formulas: ") + bad).c_str());
    if (const char *bad = batch_csr_check(num_instances, h_proof_inst_begin, h_proof_clause_begin, h_proof_lits,
                                          nullptr, true, &ps))
        return fail_arg(who, (std::string("proofs: ") + bad).c_str());
    if (num_instances == 0) return SATMI_OK;
    const int B = num_instances, C = fs.C, P = ps.C;
    const int max_vars = std::max(fs.max_var, ps.max_var);
    if (max_vars > SATMI_TRIM_MAX_VARS) return too_large(who, max_vars);

    // ---- lease the workspace
    int dev = 0;
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts, &dev));
    Lease<TrimWork> lease{Pool<TrimWork>::get().acquire(dev)};
    if (!lease.w) {
        set_error(std::string(who) + ": hipStreamCreate failed");
        return SATMI_ERR_HIP;
    }
    lease.ok = true;   // whatever the call's outcome (see BatchWork)
    TrimWork &wk = *lease.w;
    hipStream_t s = wk.stream;
    // ---- carve.  Inputs, one copy: the two CSR triples.  Outputs, one copy back: the words, the two mark arrays
    const size_t n_icb = 4 * (size_t)(B + 1), n_clb = 4 * ((size_t)C + 1), n_lits = 4 * (size_t)fs.Ltot;
    const size_t n_pcb = 4 * ((size_t)P + 1), n_plits = 4 * (size_t)ps.Ltot;
    Carve cu, co;
    const size_t u_icb = cu.take(n_icb), u_clb = cu.take(n_clb), u_lits = cu.take(std::max<size_t>(n_lits, 4));
    const size_t u_pib = cu.take(n_icb), u_pcb = cu.take(n_pcb), u_plits = cu.take(std::max<size_t>(n_plits, 4));
    const size_t out_words = 4 * (size_t)B * SATMI_TRIM_NWORDS, core_words = 4 * (size_t)C, lemma_words = 4 * (size_t)P;
    const size_t o_out = co.take(out_words), o_core = co.take(std::max<size_t>(core_words, 4)),
                 o_lemma = co.take(std::max<size_t>(lemma_words, 4));
    SATMI_TRY(wk.up.reserve(cu.at, &TR_OOM));
    SATMI_TRY(wk.out.reserve(co.at, &TR_OOM));
    SATMI_TRY(wk.up_h.grow(cu.at));
    SATMI_TRY(wk.out_h.grow(co.at));
    std::memcpy(wk.up_h.p + u_icb, h_inst_clause_begin, n_icb);
    std::memcpy(wk.up_h.p + u_clb, h_clause_lit_begin, n_clb);
    if (n_lits) std::memcpy(wk.up_h.p + u_lits, h_lits, n_lits);
    std::memcpy(wk.up_h.p + u_pib, h_proof_inst_begin, n_icb);
    std::memcpy(wk.up_h.p + u_pcb, h_proof_clause_begin, n_pcb);
    if (n_plits) std::memcpy(wk.up_h.p + u_plits, h_proof_lits, n_plits);
    const Staged in{wk.up.as<unsigned char>(), s}, res{wk.out.as<unsigned char>(), s};
    SATMI_TRY(in.up(0, wk.up_h.p, cu.at));
    // (the kernel initialises its instances' ranges; clauses and lemmas of the arrays before the
    // first instance's belong to no instance: they read 0 / -1)
    const size_t pre_core = 4 * (size_t)h_inst_clause_begin[0], pre_lemma = 4 * (size_t)h_proof_inst_begin[0];
    if (pre_core) SATMI_HIP(hipMemsetAsync(res.at<int32_t>(o_core), 0, pre_core, s));
    if (pre_lemma) SATMI_HIP(hipMemsetAsync(res.at<int32_t>(o_lemma), 0xFF, pre_lemma, s));

    TrimArgs A{};
    A.icb = in.at<const int32_t>(u_icb);
    A.clb = in.at<const int32_t>(u_clb);
    A.lits = in.at<const int32_t>(u_lits);
    A.pib = in.at<const int32_t>(u_pib);
    A.pcb = in.at<const int32_t>(u_pcb);
    A.plits = in.at<const int32_t>(u_plits);
    A.out = res.at<int32_t>(o_out);
    A.core = res.at<int32_t>(o_core);
    A.lemma = res.at<int32_t>(o_lemma);
    A.num_instances = B;
    A.max_vars = (uint32_t)max_vars;
    if (const int rc = trim_launch(who, A, std::max(fs.max_len, ps.max_len), s)) {
        (void)hipStreamSynchronize(s);   // the upload still reads the pinned words the next call fills
        return rc;
    }
    // one copy back: the words, and the marks behind them as far as they are wanted
    const size_t back = h_lemma && lemma_words ? o_lemma + lemma_words : h_core && core_words ? o_core + core_words : out_words;
    SATMI_TRY(res.down(wk.out_h.p, 0, back));
    SATMI_HIP(hipStreamSynchronize(s));
    std::memcpy(h_out, wk.out_h.p + o_out, out_words);
    if (h_core && core_words) std::memcpy(h_core, wk.out_h.p + o_core, core_words);
    if (h_lemma && lemma_words) std::memcpy(h_lemma, wk.out_h.p + o_lemma, lemma_words);
    return SATMI_OK;
}
