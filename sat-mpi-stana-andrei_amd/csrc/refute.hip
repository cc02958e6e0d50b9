// refute.hip -- batched refutation check on gfx950: forward reverse-unit-
// propagation (RUP) over B clause sets, each with an ordered list of lemma
// clauses, in one launch.  Lemma i of an instance is VERIFIED if assigning every
// literal of it false and propagating unit clauses to a fixpoint over the
// formula and the lemmas 0 .. i-1 reaches a conflict (a clause whose literals
// are all false, or a variable needed with both signs).  A record of
// satmi_resolution_*_host or satmi_dp_*_host followed by the empty clause is
// such a list (satmi/refute.py).
//
//   * One wavefront per instance, persistent over the batch: wave w of W takes
//     instances w, w + W, ... (no work counter, so the device form owns no
//     device memory and a launch is one kernel on the caller's stream).  The
//     wave checks the instance's lemmas one after the other and stops behind
//     the first empty one.
//   * The wave's LDS region holds a truth table and a trail.  The table has two
//     bits per variable v of 1 .. max_vars: bit 2(v & 15) of word v >> 4 for
//     "+v is true", the bit above it for "-v is true".  A literal is set true
//     with an LDS atomicOr; the word it returns tells the lane whether the
//     opposite bit was there (a conflict, also between two lanes of one step)
//     and whether the variable had no bit at all: only that lane pushes the
//     variable onto the trail (16 bits per entry), so 64 copies of one unit
//     clause push one entry and the trail never holds more than max_vars.
//   * After a lemma the wave stores 0 to the table words of the trail's
//     variables (every bit of such a word belongs to a variable on the trail:
//     nothing is kept across lemmas); the table is wiped whole only once.
//   * A propagation round scans the formula's clauses and then the lemmas
//     0 .. i-1 from global memory.  A clause with a true literal is passed; one
//     with no unassigned literal is a conflict; one whose unassigned literals
//     are all the same literal assigns it (a repeated literal counts once).  A
//     round that neither conflicts nor assigns ends the lemma.  Every other
//     round puts at least one variable on the trail, so there are at most
//     max_vars + 1 rounds: the loop's own condition.
//   * Unit propagation is confluent about reaching a conflict, so the verdicts
//     do not depend on the scan order, on the clause form or on which lane's
//     atomic comes first; nothing else (a round count, the conflict clause) is
//     written.
//   * Two clause forms, chosen per launch from max_clause_len (over formula
//     and lemmas), as in check.hip and for its reason:
//       short  1 <= max_clause_len <= RF_SHORT_MAX (8): a lane per clause, 64
//              clauses per wave step; the units of a step are assigned at its end;
//       long   anything else (0 = unknown): the whole wave takes a clause in
//              64-literal steps, settles it by ballots and assigns its unit at once.
//   * A literal 0, INT32_MIN or beyond max_vars can come through the device
//     form only.  A formula clause or earlier lemma that holds one is skipped
//     as a premise (dropping a premise is sound), a lemma that holds one fails;
//     SATMI_REFUTE_BAD_LITERAL is set for any in the formula (one pass over its
//     literals per instance) or in a checked lemma.
//   * Workgroups hold 4, 2 or 1 waves by check.hip's rule.  At
//     SATMI_REFUTE_MAX_VARS = 32,767 the table is 8 KiB and the trail 64 KiB.
//
// Plain C++ and vector memory operations only.  The translation unit shares no
// device code with the solver kernels, whose machine code stays what it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>

#include "batch_host.h"
#include "common.h"

namespace satmi {

constexpr int RF_SHORT_MAX = 8;   // longest clause of the lane-per-clause form
// LDS words of one wave's table and of its trail (16 bits per variable), each a multiple of 4
constexpr uint32_t rf_table_words(uint32_t max_vars) { return ((max_vars >> 4) + 1u + 3u) & ~3u; }
constexpr uint32_t rf_trail_words(uint32_t max_vars) { return (((max_vars + 1u) >> 1) + 3u) & ~3u; }
static_assert(SATMI_REFUTE_MAX_VARS <= 0xFFFF, "a trail entry is 16 bits");
static_assert(4u * (rf_table_words(SATMI_REFUTE_MAX_VARS) + rf_trail_words(SATMI_REFUTE_MAX_VARS)) == 72u * 1024u &&
                  2u * 72u * 1024u <= LDS_PER_CU,
              "at the variable limit a region is 8 KiB + 64 KiB, two to a CU");

struct RefuteArgs {
    const int32_t *icb, *clb, *lits;      // the formulas (CSR)
    const int32_t *pib, *pcb, *plits;     // the proofs (CSR): instance -> lemmas -> literals
    int32_t *out;                         // [B x SATMI_REFUTE_NWORDS]
    int32_t *lemma_ok;                    // [P] or null
    int num_instances;
    uint32_t max_vars;
    uint32_t table_words;                 // LDS words of one wave's table, a multiple of 4
    uint32_t region_words;                // ... of its table and trail, a multiple of 4
};

// A wave's propagation state.  `trail_len` and `conflict` are wave-uniform.
struct RfWave {
    uint32_t *table;
    uint16_t *trail;
    uint32_t max_vars;
    int trail_len;
    bool conflict;
};

// |l| (INT32_MIN: 2^31)
__device__ __forceinline__ uint32_t rf_var(int32_t l) { return l < 0 ? 0u - (uint32_t)l : (uint32_t)l; }
__device__ __forceinline__ bool rf_bad(int32_t l, uint32_t max_vars) { return rf_var(l) - 1u >= max_vars; }

// What the table says of a literal it holds: 0 unassigned, bit 0 = l is true, bit 1 = -l is.
__device__ __forceinline__ uint32_t rf_lookup(const uint32_t *table, int32_t l) {
    const uint32_t v = rf_var(l);
    const uint32_t pair = (table[v >> 4] >> (2u * (v & 15u))) & 3u;
    return l < 0 ? ((pair >> 1) | (pair << 1)) & 3u : pair;
}

// The lanes with `on` set their literal `l` (which the table holds) true.  All
// 64 lanes call.  Returns, per lane, whether -l was true already.
__device__ __forceinline__ bool rf_assign(RfWave &w, bool on, int32_t l) {
    bool opposite = false, fresh = false;
    const uint32_t v = rf_var(l);
    if (on) {
        const uint32_t sh = 2u * (v & 15u) + (l < 0 ? 1u : 0u);
        const uint32_t old = atomicOr(w.table + (v >> 4), 1u << sh);
        opposite = (old >> (sh ^ 1u)) & 1u;
        fresh = ((old >> (sh & ~1u)) & 3u) == 0u;   // this lane's atomic gave the variable its first bit
    }
    const uint64_t fm = __ballot(fresh);
    if (fresh) w.trail[w.trail_len + __popcll(fm & lanemask_lt())] = (uint16_t)v;   // < max_vars: one push per variable
    w.trail_len += __popcll(fm);
    return opposite;
}

// One propagation round over clauses [0, n) of a clause list: lane-per-clause.
__device__ __forceinline__ void rf_scan_short(RfWave &w, const int32_t *clb, const int32_t *lits, int n) {
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
                if (rf_bad(l, w.max_vars)) {
                    sat = true;   // not a premise
                    continue;
                }
                const uint32_t st = rf_lookup(w.table, l);
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
        const bool opposite = rf_assign(w, unit, u);
        w.conflict = __ballot(fals || opposite) != 0ull;
        wave_sync();
    }
}

// The same, the whole wave on one clause at a time.
__device__ __forceinline__ void rf_scan_long(RfWave &w, const int32_t *clb, const int32_t *lits, int n) {
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
                bad = rf_bad(l, w.max_vars);
                if (!bad) st = rf_lookup(w.table, l);
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
        } else if (!many) {
            // (a unit under the table it was read from: -u is not true, so this cannot conflict)
            rf_assign(w, ln == 0, u);
            wave_sync();
        }
    }
}

template <bool LONG>
__global__ void __launch_bounds__(256) refute_kernel(RefuteArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t rf_lds[];
    const int ln = lane_id(), wv = (int)threadIdx.x >> 6, wpg = (int)blockDim.x >> 6;
    RfWave w;
    w.table = rf_lds + (size_t)wv * A.region_words;
    w.trail = (uint16_t *)(w.table + A.table_words);
    w.max_vars = A.max_vars;
    w.trail_len = 0;
    w.conflict = false;
    for (uint32_t t = (uint32_t)ln; t < A.table_words; t += 64u) w.table[t] = 0u;
    wave_sync();
    const int64_t W = (int64_t)gridDim.x * wpg;
    for (int64_t b = (int64_t)blockIdx.x * wpg + wv; b < A.num_instances; b += W) {
        const int c0 = A.icb[b], m = A.icb[b + 1] - c0;
        const int p0 = A.pib[b], k = A.pib[b + 1] - p0;
        const int32_t *fclb = A.clb + c0, *pclb = A.pcb + p0;
        int flags = 0, failed = 0, first = -1;
        // ---- bad literals of the formula (its clauses are skipped as premises)
        {
            const int s = fclb[0], e = fclb[m];
            bool bad = false;
            for (int j = s + ln; j < e; j += 64) bad |= rf_bad(A.lits[j], A.max_vars);
            if (__ballot(bad)) flags |= SATMI_REFUTE_BAD_LITERAL;
        }
        int i = 0;
        bool ended = false;   // behind the first empty lemma
        for (; i < k && !ended; ++i) {
            const int s = uniform_i32(pclb[i]), e = uniform_i32(pclb[i + 1]);
            // ---- every literal of the lemma false
            bool lemma_bad = false, taut = false;
            for (int j0 = s; j0 < e; j0 += 64) {
                const int j = j0 + ln;
                bool bad = false, good = false;
                int32_t l = 0;
                if (j < e) {
                    l = A.plits[j];
                    bad = rf_bad(l, A.max_vars);
                    good = !bad;
                }
                const bool opposite = rf_assign(w, good, good ? -l : 0);   // (-l exists: l is not INT32_MIN)
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
                        rf_scan_long(w, fclb, A.lits, m);
                        rf_scan_long(w, pclb, A.plits, i);
                    } else {
                        rf_scan_short(w, fclb, A.lits, m);
                        rf_scan_short(w, pclb, A.plits, i);
                    }
                    if (w.trail_len == before) break;   // nothing assigned: the fixpoint
                }
            }
            const bool ok = !lemma_bad && (taut || w.conflict);
            if (!ok) {
                if (failed == 0) first = i;
                ++failed;
            }
            if (A.lemma_ok && ln == 0) A.lemma_ok[p0 + i] = ok ? 1 : 0;
            ended = e == s;
            // ---- clear what the lemma assigned
            for (int t = ln; t < w.trail_len; t += 64) w.table[w.trail[t] >> 4] = 0u;
            w.trail_len = 0;
            wave_sync();
        }
        if (A.lemma_ok)
            for (int t = i + ln; t < k; t += 64) A.lemma_ok[p0 + t] = -1;   // not checked
        const int status = failed ? SATMI_REFUTE_FAILED : ended ? SATMI_REFUTE_PROVEN : SATMI_REFUTE_OPEN;
        if (ln < SATMI_REFUTE_NWORDS)
            A.out[b * SATMI_REFUTE_NWORDS + ln] = ln == 0 ? status : ln == 1 ? failed : ln == 2 ? first : flags;
    }
}

// ------------------------------------------------------------------ host side
namespace {

constexpr OomText RF_OOM{"satmi_check_refutations_host", "split the batch"};

std::atomic<int> g_dbg_grid{0}, g_dbg_wpg{0};   // satmi_refute_debug_grid

struct RefuteWork : BatchWork {};   // a pool of its own (keys_out, rec_off stay empty)

int too_large(const char *who, int64_t max_vars) {
    set_error(std::string(who) + ": variable " + std::to_string(max_vars) + " is beyond the table's " +
              std::to_string(SATMI_REFUTE_MAX_VARS));
    return SATMI_ERR_TOO_LARGE;
}

// One launch on `s`; every argument is checked by the caller.
int refute_launch(const char *who, RefuteArgs A, int max_clause_len, hipStream_t s) {
    A.table_words = rf_table_words(A.max_vars);
    A.region_words = A.table_words + rf_trail_words(A.max_vars);
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
    const bool long_form = max_clause_len <= 0 || max_clause_len > RF_SHORT_MAX;
    const void *fn = long_form ? (const void *)refute_kernel<true> : (const void *)refute_kernel<false>;
    SATMI_TRY(batch_allow_lds(fn, lds_bytes));
    if (long_form)
        hipLaunchKernelGGL(refute_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    else
        hipLaunchKernelGGL(refute_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

}  // namespace

}  // namespace satmi

using namespace satmi;

extern "C" int satmi_refute_debug_grid(int workgroups, int waves_per_wg) {
    if (workgroups < 0 || !(waves_per_wg == 0 || waves_per_wg == 1 || waves_per_wg == 2 || waves_per_wg == 4))
        return fail_arg("satmi_refute_debug_grid", "workgroups >= 0 and waves_per_wg one of 0, 1, 2, 4");
    g_dbg_grid = workgroups;
    g_dbg_wpg = waves_per_wg;
    return SATMI_OK;
}

extern "C" int satmi_check_refutations_device(int num_instances, const int32_t *d_inst_clause_begin,
                                              const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                              const int32_t *d_proof_inst_begin, const int32_t *d_proof_clause_begin,
                                              const int32_t *d_proof_lits, int max_vars, int max_clause_len,
                                              int32_t *d_out, int32_t *d_lemma_ok, void *stream) {
    const char *who = "satmi_check_refutations_device";
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (max_vars < 0 || max_clause_len < 0) return fail_arg(who, "negative max_vars / max_clause_len");
    if (num_instances == 0) return SATMI_OK;
    if (!d_inst_clause_begin || !d_clause_lit_begin || !d_lits || !d_proof_inst_begin || !d_proof_clause_begin ||
        !d_proof_lits || !d_out)
        return fail_arg(who, "null pointer");
    if (max_vars > SATMI_REFUTE_MAX_VARS) return too_large(who, max_vars);
    RefuteArgs A{};
    A.icb = d_inst_clause_begin;
    A.clb = d_clause_lit_begin;
    A.lits = d_lits;
    A.pib = d_proof_inst_begin;
    A.pcb = d_proof_clause_begin;
    A.plits = d_proof_lits;
    A.out = d_out;
    A.lemma_ok = d_lemma_ok;
    A.num_instances = num_instances;
    A.max_vars = (uint32_t)max_vars;
    return refute_launch(who, A, max_clause_len, (hipStream_t)stream);
}

extern "C" int satmi_check_refutations_host(int num_instances, const int32_t *h_inst_clause_begin,
                                            const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                            const int32_t *h_proof_inst_begin, const int32_t *h_proof_clause_begin,
                                            const int32_t *h_proof_lits, int32_t *h_out, int32_t *h_lemma_ok) {
    const char *who = "satmi_check_refutations_host";
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
    if (max_vars > SATMI_REFUTE_MAX_VARS) return too_large(who, max_vars);

    // ---- lease the workspace
    int dev = 0;
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts, &dev));
    Lease<RefuteWork> lease{Pool<RefuteWork>::get().acquire(dev)};
    if (!lease.w) {
        set_error(std::string(who) + ": hipStreamCreate failed");
        return SATMI_ERR_HIP;
    }
    lease.ok = true;   // whatever the call's outcome (see BatchWork)
    RefuteWork &wk = *lease.w;
    hipStream_t s = wk.stream;
    // ---- carve.  Inputs, one copy: the two CSR triples.  Outputs, one copy back: the words, the lemma verdicts
    const size_t n_icb = 4 * (size_t)(B + 1), n_clb = 4 * ((size_t)C + 1), n_lits = 4 * (size_t)fs.Ltot;
    const size_t n_pcb = 4 * ((size_t)P + 1), n_plits = 4 * (size_t)ps.Ltot;
    Carve cu, co;
    const size_t u_icb = cu.take(n_icb), u_clb = cu.take(n_clb), u_lits = cu.take(std::max<size_t>(n_lits, 4));
    const size_t u_pib = cu.take(n_icb), u_pcb = cu.take(n_pcb), u_plits = cu.take(std::max<size_t>(n_plits, 4));
    const size_t out_words = 4 * (size_t)B * SATMI_REFUTE_NWORDS, ok_words = 4 * (size_t)P;
    const size_t o_out = co.take(out_words), o_ok = co.take(std::max<size_t>(ok_words, 4));
    SATMI_TRY(wk.up.reserve(cu.at, &RF_OOM));
    SATMI_TRY(wk.out.reserve(co.at, &RF_OOM));
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
    // (lemmas of the arrays before the first instance's belong to no instance: they stay -1)
    if (h_lemma_ok) SATMI_HIP(hipMemsetAsync(res.at<int32_t>(o_ok), 0xFF, std::max<size_t>(ok_words, 4), s));

    RefuteArgs A{};
    A.icb = in.at<const int32_t>(u_icb);
    A.clb = in.at<const int32_t>(u_clb);
    A.lits = in.at<const int32_t>(u_lits);
    A.pib = in.at<const int32_t>(u_pib);
    A.pcb = in.at<const int32_t>(u_pcb);
    A.plits = in.at<const int32_t>(u_plits);
    A.out = res.at<int32_t>(o_out);
    A.lemma_ok = h_lemma_ok ? res.at<int32_t>(o_ok) : nullptr;
    A.num_instances = B;
    A.max_vars = (uint32_t)max_vars;
    if (const int rc = refute_launch(who, A, std::max(fs.max_len, ps.max_len), s)) {
        (void)hipStreamSynchronize(s);   // the upload still reads the pinned words the next call fills
        return rc;
    }
    // one copy back: the words, and the verdicts behind them if they are wanted
    SATMI_TRY(res.down(wk.out_h.p, 0, h_lemma_ok && ok_words ? o_ok + ok_words : out_words));
    SATMI_HIP(hipStreamSynchronize(s));
    std::memcpy(h_out, wk.out_h.p + o_out, out_words);
    if (h_lemma_ok && ok_words) std::memcpy(h_lemma_ok, wk.out_h.p + o_ok, ok_words);
    return SATMI_OK;
}
