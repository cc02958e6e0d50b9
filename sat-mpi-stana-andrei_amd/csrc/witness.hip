// witness.hip -- batched witness models on gfx950: rebuild an assignment from
// the record of a Davis-Putnam elimination or of a resolution saturation that
// answered True, and evaluate it against the formula, in one launch.  Instance
// b has a formula F of m clauses, a record R of P clauses (a second CSR triple,
// shaped like a proof batch) and an ordered list of stages (x, lo, hi): a
// variable and a clause range in the joint numbering of trim.hip's reasons
// (index c < m is formula clause c, index m + j record clause j).
//
//   * The assignment is total: every variable starts False.  A stage reads the
//     clauses of its range under the assignment as it stands.  A clause that
//     holds +x and -x is passed, and with `highest_only` so is one whose largest
//     |literal| is not x.  needP: some clause holds +x and every other literal
//     of it is false; needN likewise with -x.  Both: the stage is stuck.  In
//     every case x becomes needP.  Both needs are functions of the assignment
//     before the stage, so nothing depends on lane order, grid or clause form.
//   * After the last stage every clause of F is evaluated: SATMI_WITNESS_MODEL
//     iff none is falsified, whatever the stages were (sound for any input).
//   * One wavefront per instance, persistent over the batch by a fixed stride:
//     wave w of W takes instances w, w + W, ... (no work counter, so the device
//     form owns no device memory and a launch is one kernel on the caller's
//     stream).
//   * The wave's LDS region holds two bits per variable v of 1 .. max_vars:
//     bit 2(v & 15) of word v >> 4 is v's value, the bit above it "v occurs in
//     F with a good literal".  The occurrence bits are set by LDS atomics, 64
//     literals of F per step; a stage's variable is set or cleared by one lane
//     once the range is read.  The row (check.hip's format) is read off the
//     table: a lane per word, 16 variables, placed by a wave prefix sum of the
//     occurrence counts, up to the word of F's largest variable.
//   * After an instance the wave stores 0 to the words F's literals and the
//     stage variables touched (every bit of such a word is the instance's); the
//     table is wiped whole only once, when the wave starts.
//   * Two clause forms, chosen per launch from max_clause_len (over F and R),
//     as in check.hip and refute.hip and for their reason:
//       short  1 <= max_clause_len <= WT_SHORT_MAX (8): a lane per clause, 64
//              clauses per wave step, the needs by ballot;
//       long   anything else (0 = unknown): the whole wave takes a clause in
//              64-literal steps.
//     Neither form leaves a clause early, so the literals read -- and with them
//     SATMI_WITNESS_BAD_LITERAL -- are the same in both.
//   * A literal 0, INT32_MIN or beyond max_vars can come through the device
//     form only.  It counts as false, and as a magnitude for `highest_only`
//     (INT32_MIN: 2^31); the flag is set for any in F or in a clause a stage reads.
//   * Workgroups hold 4, 2 or 1 waves by check.hip's rule, and the table is
//     check.hip's: 128 KiB at SATMI_WITNESS_MAX_VARS = 524,287.
//
// Plain C++ and vector memory operations only.  The translation unit shares no
// device code with the other kernels, whose machine code stays what it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>

#include "batch_host.h"
#include "common.h"

namespace satmi {

constexpr int WT_SHORT_MAX = 8;   // longest clause of the lane-per-clause form
static_assert(SATMI_WITNESS_MAX_VARS == SATMI_CHECK_MAX_VARS, "any witness can be checked");
static_assert(4u * (((uint32_t)SATMI_WITNESS_MAX_VARS >> 4) + 1u) <= LDS_PER_CU,
              "the largest table is one wave's LDS region");

struct WitnessArgs {
    const int32_t *icb, *clb, *lits;      // the formulas (CSR)
    const int32_t *pib, *pcb, *plits;     // the records (CSR)
    const int32_t *isb;                   // [B + 1] stage ranges
    const int32_t *svar, *slo, *shi;      // the stages
    int32_t *out;                         // [B x SATMI_WITNESS_NWORDS]
    int32_t *row_len, *row_lits;          // [B], [B x stride]
    int num_instances, stride, highest_only;
    uint32_t max_vars;
    uint32_t region_words;                // LDS words of one wave's table, a multiple of 4
};

// |l| (INT32_MIN: 2^31)
__device__ __forceinline__ uint32_t wt_var(int32_t l) { return l < 0 ? 0u - (uint32_t)l : (uint32_t)l; }

// Whether the good literal l of variable v is true under the table.
__device__ __forceinline__ bool wt_true(const uint32_t *table, int32_t l, uint32_t v) {
    return (((table[v >> 4] >> (2u * (v & 15u))) & 1u) != 0u) == (l > 0);
}

// What a stage has found so far: `p` and `n` are wave-uniform, `bad` is the lane's own.
struct WtNeeds {
    bool p, n, bad;
};

// What one literal of a clause says about stage variable x.
struct WtClause {
    bool hp, hn, bigger, other;   // holds +x, holds -x, a larger |literal|, another literal that is true
};

__device__ __forceinline__ void wt_literal(const uint32_t *table, uint32_t max_vars, int32_t x, int32_t l,
                                           WtClause &k, bool &bad) {
    const uint32_t v = wt_var(l);
    k.bigger |= v > (uint32_t)x;
    if (v - 1u >= max_vars) {   // false
        bad = true;
        return;
    }
    k.hp |= l == x;
    k.hn |= l == -x;
    k.other |= v != (uint32_t)x && wt_true(table, l, v);
}

// The clauses [a, b) of one clause list against stage variable x.
template <bool LONG>
__device__ __forceinline__ void wt_scan(const uint32_t *table, uint32_t max_vars, const int32_t *clb,
                                        const int32_t *lits, int a, int b, int32_t x, bool highest_only,
                                        WtNeeds &nd) {
    const int ln = lane_id();
    if (!LONG) {
        for (int cb = a; cb < b; cb += 64) {
            const int c = cb + ln;
            bool fp = false, fn = false;
            if (c < b) {
                const int s = clb[c], e = clb[c + 1];
                WtClause k{false, false, false, false};
                for (int j = s; j < e; ++j) wt_literal(table, max_vars, x, lits[j], k, nd.bad);
                const bool live = !(k.hp && k.hn) && !(highest_only && k.bigger) && !k.other;
                fp = k.hp && live;
                fn = k.hn && live;
            }
            nd.p |= __ballot(fp) != 0ull;
            nd.n |= __ballot(fn) != 0ull;
        }
    } else {
        for (int c = a; c < b; ++c) {
            const int s = uniform_i32(clb[c]), e = uniform_i32(clb[c + 1]);
            WtClause k{false, false, false, false};   // the lane's share
            for (int j0 = s; j0 < e; j0 += 64) {
                const int j = j0 + ln;
                if (j < e) wt_literal(table, max_vars, x, lits[j], k, nd.bad);
            }
            const bool hp = __ballot(k.hp) != 0ull, hn = __ballot(k.hn) != 0ull;
            const bool live = !(hp && hn) && !(highest_only && __ballot(k.bigger) != 0ull) && __ballot(k.other) == 0ull;
            nd.p |= hp && live;
            nd.n |= hn && live;
        }
    }
}

template <bool LONG>
__global__ void __launch_bounds__(256) witness_kernel(WitnessArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t wt_lds[];
    const int ln = lane_id(), wv = (int)threadIdx.x >> 6, wpg = (int)blockDim.x >> 6;
    uint32_t *table = wt_lds + (size_t)wv * A.region_words;
    for (uint32_t t = (uint32_t)ln; t < A.region_words; t += 64u) table[t] = 0u;
    wave_sync();
    const bool ho = A.highest_only != 0;
    const int64_t W = (int64_t)gridDim.x * wpg;
    for (int64_t b = (int64_t)blockIdx.x * wpg + wv; b < A.num_instances; b += W) {
        const int c0 = A.icb[b], m = A.icb[b + 1] - c0;
        const int p0 = A.pib[b], P = A.pib[b + 1] - p0;
        const int s0 = A.isb[b], ns = A.isb[b + 1] - s0;
        const int32_t *fclb = A.clb + c0, *pclb = A.pcb + p0;
        const int fs = fclb[0], fe = fclb[m];
        int flags = 0;
        // ---- the variables of F: occurrence bits, the largest, bad literals
        int vmax = 0;
        WtNeeds nd{false, false, false};
        for (int j = fs + ln; j < fe; j += 64) {
            const uint32_t v = wt_var(A.lits[j]);
            if (v - 1u >= A.max_vars) {
                nd.bad = true;
            } else {
                atomicOr(table + (v >> 4), 2u << (2u * (v & 15u)));
                vmax = max(vmax, (int)v);
            }
        }
        vmax = wave_max_i32(vmax);
        wave_sync();
        // ---- the stages, in order
        int stuck = 0, first_stuck = -1;
        for (int t = 0; t < ns; ++t) {
            const int32_t x = uniform_i32(A.svar[s0 + t]);
            if ((uint32_t)x - 1u >= A.max_vars) {   // (a negative x: beyond 2^31)
                flags |= SATMI_WITNESS_BAD_STAGE;
                continue;
            }
            // (never read past the two clause lists)
            const int lo = min(max(uniform_i32(A.slo[s0 + t]), 0), m + P);
            const int hi = min(max(uniform_i32(A.shi[s0 + t]), lo), m + P);
            nd.p = nd.n = false;
            wt_scan<LONG>(table, A.max_vars, fclb, A.lits, min(lo, m), min(hi, m), x, ho, nd);
            wt_scan<LONG>(table, A.max_vars, pclb, A.plits, max(lo, m) - m, max(hi, m) - m, x, ho, nd);
            if (nd.p && nd.n) {
                if (stuck == 0) first_stuck = t;
                ++stuck;
            }
            wave_sync();
            if (ln == 0) {
                const uint32_t bit = 1u << (2u * ((uint32_t)x & 15u)), w = table[(uint32_t)x >> 4];
                table[(uint32_t)x >> 4] = nd.p ? w | bit : w & ~bit;
            }
            wave_sync();
        }
        // ---- every clause of F under the final assignment
        int nfals = 0, first = INT_MAX;
        if (!LONG) {
            for (int cb = 0; cb < m; cb += 64) {
                const int c = cb + ln;
                bool fals = false;
                if (c < m) {
                    const int s = fclb[c], e = fclb[c + 1];
                    bool sat = false;
                    for (int j = s; j < e; ++j) {
                        const int32_t l = A.lits[j];
                        const uint32_t v = wt_var(l);
                        sat |= v - 1u < A.max_vars && wt_true(table, l, v);
                    }
                    fals = !sat;
                }
                nfals += __popcll(__ballot(fals));
                if (fals) first = min(first, c);
            }
        } else {
            for (int c = 0; c < m; ++c) {
                const int s = uniform_i32(fclb[c]), e = uniform_i32(fclb[c + 1]);
                bool sat = false;   // the lane's share
                for (int j0 = s; j0 < e; j0 += 64) {
                    const int j = j0 + ln;
                    if (j < e) {
                        const int32_t l = A.lits[j];
                        const uint32_t v = wt_var(l);
                        sat |= v - 1u < A.max_vars && wt_true(table, l, v);
                    }
                }
                if (__ballot(sat) == 0ull) {
                    ++nfals;
                    first = min(first, c);
                }
            }
        }
        first = wave_min_i32(first);
        if (__ballot(nd.bad)) flags |= SATMI_WITNESS_BAD_LITERAL;
        // ---- the row: the variables of F, ascending, signed by their values
        int32_t *row = A.row_lits + b * A.stride;
        int total = 0;
        const uint32_t nwords = ((uint32_t)vmax >> 4) + 1u;   // <= region_words: vmax <= max_vars
        for (uint32_t w0 = 0; w0 < nwords; w0 += 64u) {
            const uint32_t wi = w0 + (uint32_t)ln;
            const uint32_t word = wi < nwords ? table[wi] : 0u;
            uint32_t occ = (word >> 1) & 0x55555555u;   // bit 2k: variable 16 wi + k occurs
            const int cnt = __popc(occ), incl = wave_incl_scan(cnt);
            int pos = total + incl - cnt;
            for (int k = 0; k < 16 && occ != 0u; ++k) {
                const uint32_t bit = (uint32_t)__builtin_ctz(occ);
                occ &= occ - 1u;
                const int32_t v = (int32_t)(16u * wi + (bit >> 1));
                if (pos < A.stride) row[pos] = (word >> bit) & 1u ? v : -v;
                ++pos;
            }
            total += lane63(incl);
        }
        if (total > A.stride) flags |= SATMI_WITNESS_ROW_TRUNCATED;
        if (ln == 0) A.row_len[b] = total;
        if (ln < SATMI_WITNESS_NWORDS)
            A.out[b * SATMI_WITNESS_NWORDS + ln] = ln == 0   ? (nfals == 0 ? SATMI_WITNESS_MODEL : SATMI_WITNESS_NOT_MODEL)
                                                   : ln == 1 ? stuck
                                                   : ln == 2 ? first_stuck
                                                   : ln == 3 ? flags
                                                   : ln == 4 ? nfals
                                                             : (first == INT_MAX ? -1 : first);
        // ---- clear by replay: the words F's literals and the stage variables touched
        wave_sync();
        for (int j = fs + ln; j < fe; j += 64) {
            const uint32_t v = wt_var(A.lits[j]);
            if (v - 1u < A.max_vars) table[v >> 4] = 0u;
        }
        for (int t = ln; t < ns; t += 64) {
            const int32_t x = A.svar[s0 + t];
            if (x > 0 && (uint32_t)x <= A.max_vars) table[(uint32_t)x >> 4] = 0u;
        }
        wave_sync();
    }
}

// ------------------------------------------------------------------ host side
namespace {

constexpr OomText WT_OOM{"satmi_witness_models_host", "split the batch"};

std::atomic<int> g_dbg_grid{0}, g_dbg_wpg{0};   // satmi_witness_debug_grid

struct WitnessWork : BatchWork {};   // a pool of its own (keys_out, rec_off stay empty)

int too_large(const char *who, int64_t max_vars) {
    set_error(std::string(who) + ": variable " + std::to_string(max_vars) + " is beyond the table's " +
              std::to_string(SATMI_WITNESS_MAX_VARS));
    return SATMI_ERR_TOO_LARGE;
}

// One launch on `s`; every argument is checked by the caller.
int witness_launch(const char *who, WitnessArgs A, int max_clause_len, hipStream_t s) {
    const uint32_t words = (A.max_vars >> 4) + 1u;
    A.region_words = (words + 3u) & ~3u;
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
    const bool long_form = max_clause_len <= 0 || max_clause_len > WT_SHORT_MAX;
    const void *fn = long_form ? (const void *)witness_kernel<true> : (const void *)witness_kernel<false>;
    SATMI_TRY(batch_allow_lds(fn, lds_bytes));
    if (long_form)
        hipLaunchKernelGGL(witness_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    else
        hipLaunchKernelGGL(witness_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

}  // namespace

}  // namespace satmi

using namespace satmi;

extern "C" int satmi_witness_debug_grid(int workgroups, int waves_per_wg) {
    if (workgroups < 0 || !(waves_per_wg == 0 || waves_per_wg == 1 || waves_per_wg == 2 || waves_per_wg == 4))
        return fail_arg("satmi_witness_debug_grid", "workgroups >= 0 and waves_per_wg one of 0, 1, 2, 4");
    g_dbg_grid = workgroups;
    g_dbg_wpg = waves_per_wg;
    return SATMI_OK;
}

extern "C" int satmi_witness_models_device(int num_instances, const int32_t *d_inst_clause_begin,
                                           const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                           const int32_t *d_record_inst_begin, const int32_t *d_record_clause_begin,
                                           const int32_t *d_record_lits, const int32_t *d_inst_stage_begin,
                                           const int32_t *d_stage_var, const int32_t *d_stage_lo,
                                           const int32_t *d_stage_hi, int highest_only, int max_vars,
                                           int max_clause_len, int32_t *d_out, int32_t *d_row_len,
                                           int32_t *d_row_lits, int stride, void *stream) {
    const char *who = "satmi_witness_models_device";
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (stride < 1) return fail_arg(who, "stride < 1");
    if (highest_only != 0 && highest_only != 1) return fail_arg(who, "highest_only is 0 or 1");
    if (max_vars < 0 || max_clause_len < 0) return fail_arg(who, "negative max_vars / max_clause_len");
    if (num_instances == 0) return SATMI_OK;
    if (!d_inst_clause_begin || !d_clause_lit_begin || !d_lits || !d_record_inst_begin || !d_record_clause_begin ||
        !d_record_lits || !d_inst_stage_begin || !d_stage_var || !d_stage_lo || !d_stage_hi || !d_out || !d_row_len ||
        !d_row_lits)
        return fail_arg(who, "null pointer");
    if (max_vars > SATMI_WITNESS_MAX_VARS) return too_large(who, max_vars);
    WitnessArgs A{};
    A.icb = d_inst_clause_begin;
    A.clb = d_clause_lit_begin;
    A.lits = d_lits;
    A.pib = d_record_inst_begin;
    A.pcb = d_record_clause_begin;
    A.plits = d_record_lits;
    A.isb = d_inst_stage_begin;
    A.svar = d_stage_var;
    A.slo = d_stage_lo;
    A.shi = d_stage_hi;
    A.out = d_out;
    A.row_len = d_row_len;
    A.row_lits = d_row_lits;
    A.num_instances = num_instances;
    A.stride = stride;
    A.highest_only = highest_only;
    A.max_vars = (uint32_t)max_vars;
    return witness_launch(who, A, max_clause_len, (hipStream_t)stream);
}

extern "C" int satmi_witness_models_host(int num_instances, const int32_t *h_inst_clause_begin,
                                         const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                         const int32_t *h_record_inst_begin, const int32_t *h_record_clause_begin,
                                         const int32_t *h_record_lits, const int32_t *h_inst_stage_begin,
                                         const int32_t *h_stage_var, const int32_t *h_stage_lo,
                                         const int32_t *h_stage_hi, int highest_only, int32_t *h_out,
                                         int32_t *h_row_len, int32_t *h_row_lits, int stride) {
    const char *who = "satmi_witness_models_host";
    // ---- check: all of it before any HIP call
    CsrShape fs, ps;
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (stride < 1) return fail_arg(who, "stride < 1");
    if (highest_only != 0 && highest_only != 1) return fail_arg(who, "highest_only is 0 or 1");
    if (const char *bad = batch_csr_check(num_instances, h_inst_clause_begin, h_clause_lit_begin, h_lits, nullptr,
                                          h_out && h_row_len && h_row_lits, &fs))
        return fail_arg(who, (std::string("formulas: ") + bad).c_str());
    if (const char *bad = batch_csr_check(num_instances, h_record_inst_begin, h_record_clause_begin, h_record_lits,
                                          nullptr, true, &ps))
        return fail_arg(who, (std::string("records: ") + bad).c_str());
    if (num_instances == 0) return SATMI_OK;
    const int B = num_instances, C = fs.C, P = ps.C;
    const int max_vars = std::max(fs.max_var, ps.max_var);
    if (!h_inst_stage_begin) return fail_arg(who, "stages: null pointer");
    if (h_inst_stage_begin[0] < 0) return fail_arg(who, "stages: stage ranges are not ascending");
    for (int b = 0; b < B; ++b)
        if (h_inst_stage_begin[b + 1] < h_inst_stage_begin[b])
            return fail_arg(who, "stages: stage ranges are not ascending");
    const int S = h_inst_stage_begin[B];
    if (S > 0 && (!h_stage_var || !h_stage_lo || !h_stage_hi)) return fail_arg(who, "stages: null pointer");
    for (int b = 0; b < B; ++b) {
        const int64_t top = (int64_t)(h_inst_clause_begin[b + 1] - h_inst_clause_begin[b]) +
                            (int64_t)(h_record_inst_begin[b + 1] - h_record_inst_begin[b]);
        for (int t = h_inst_stage_begin[b]; t < h_inst_stage_begin[b + 1]; ++t) {
            if (h_stage_var[t] < 1 || h_stage_var[t] > max_vars)
                return fail_arg(who, "stages: stage variable outside 1 .. max_vars");
            if (h_stage_lo[t] < 0 || h_stage_lo[t] > h_stage_hi[t] || h_stage_hi[t] > top)
                return fail_arg(who, "stages: clause range outside 0 <= lo <= hi <= m + P");
        }
    }
    if (max_vars > SATMI_WITNESS_MAX_VARS) return too_large(who, max_vars);

    // ---- lease the workspace
    int dev = 0;
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts, &dev));
    Lease<WitnessWork> lease{Pool<WitnessWork>::get().acquire(dev)};
    if (!lease.w) {
        set_error(std::string(who) + ": hipStreamCreate failed");
        return SATMI_ERR_HIP;
    }
    lease.ok = true;   // whatever the call's outcome (see BatchWork)
    WitnessWork &wk = *lease.w;
    hipStream_t s = wk.stream;
    // ---- carve.  Inputs, one copy: the two CSR triples and the stages.  Outputs, one copy back: words, lengths, rows
    const size_t n_ib = 4 * (size_t)(B + 1), n_clb = 4 * ((size_t)C + 1), n_lits = 4 * (size_t)fs.Ltot;
    const size_t n_pcb = 4 * ((size_t)P + 1), n_plits = 4 * (size_t)ps.Ltot, n_st = 4 * (size_t)S;
    Carve cu, co;
    const size_t u_icb = cu.take(n_ib), u_clb = cu.take(n_clb), u_lits = cu.take(std::max<size_t>(n_lits, 4));
    const size_t u_pib = cu.take(n_ib), u_pcb = cu.take(n_pcb), u_plits = cu.take(std::max<size_t>(n_plits, 4));
    const size_t u_isb = cu.take(n_ib), u_var = cu.take(std::max<size_t>(n_st, 4));
    const size_t u_lo = cu.take(std::max<size_t>(n_st, 4)), u_hi = cu.take(std::max<size_t>(n_st, 4));
    const size_t out_bytes = 4 * (size_t)B * SATMI_WITNESS_NWORDS, len_bytes = 4 * (size_t)B;
    const size_t row_bytes = 4 * (size_t)B * (size_t)stride;
    const size_t o_out = co.take(out_bytes), o_len = co.take(len_bytes), o_row = co.take(row_bytes);
    SATMI_TRY(wk.up.reserve(cu.at, &WT_OOM));
    SATMI_TRY(wk.out.reserve(co.at, &WT_OOM));
    SATMI_TRY(wk.up_h.grow(cu.at));
    SATMI_TRY(wk.out_h.grow(co.at));
    std::memcpy(wk.up_h.p + u_icb, h_inst_clause_begin, n_ib);
    std::memcpy(wk.up_h.p + u_clb, h_clause_lit_begin, n_clb);
    if (n_lits) std::memcpy(wk.up_h.p + u_lits, h_lits, n_lits);
    std::memcpy(wk.up_h.p + u_pib, h_record_inst_begin, n_ib);
    std::memcpy(wk.up_h.p + u_pcb, h_record_clause_begin, n_pcb);
    if (n_plits) std::memcpy(wk.up_h.p + u_plits, h_record_lits, n_plits);
    std::memcpy(wk.up_h.p + u_isb, h_inst_stage_begin, n_ib);
    if (n_st) {
        std::memcpy(wk.up_h.p + u_var, h_stage_var, n_st);
        std::memcpy(wk.up_h.p + u_lo, h_stage_lo, n_st);
        std::memcpy(wk.up_h.p + u_hi, h_stage_hi, n_st);
    }
    const Staged in{wk.up.as<unsigned char>(), s}, res{wk.out.as<unsigned char>(), s};
    SATMI_TRY(in.up(0, wk.up_h.p, cu.at));
    // (the words of a row behind its length come back 0)
    SATMI_HIP(hipMemsetAsync(res.at<int32_t>(o_row), 0, row_bytes, s));

    WitnessArgs A{};
    A.icb = in.at<const int32_t>(u_icb);
    A.clb = in.at<const int32_t>(u_clb);
    A.lits = in.at<const int32_t>(u_lits);
    A.pib = in.at<const int32_t>(u_pib);
    A.pcb = in.at<const int32_t>(u_pcb);
    A.plits = in.at<const int32_t>(u_plits);
    A.isb = in.at<const int32_t>(u_isb);
    A.svar = in.at<const int32_t>(u_var);
    A.slo = in.at<const int32_t>(u_lo);
    A.shi = in.at<const int32_t>(u_hi);
    A.out = res.at<int32_t>(o_out);
    A.row_len = res.at<int32_t>(o_len);
    A.row_lits = res.at<int32_t>(o_row);
    A.num_instances = B;
    A.stride = stride;
    A.highest_only = highest_only;
    A.max_vars = (uint32_t)max_vars;
    if (const int rc = witness_launch(who, A, std::max(fs.max_len, ps.max_len), s)) {
        (void)hipStreamSynchronize(s);   // the upload still reads the pinned words the next call fills
        return rc;
    }
    SATMI_TRY(res.down(wk.out_h.p, 0, o_row + row_bytes));
    SATMI_HIP(hipStreamSynchronize(s));
    std::memcpy(h_out, wk.out_h.p + o_out, out_bytes);
    std::memcpy(h_row_len, wk.out_h.p + o_len, len_bytes);
    std::memcpy(h_row_lits, wk.out_h.p + o_row, row_bytes);
    return SATMI_OK;
}
