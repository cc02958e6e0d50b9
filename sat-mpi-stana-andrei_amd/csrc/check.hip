// check.hip -- batched model check on gfx950: evaluate the assignment rows a
// solver left (satmi_dpll_batch_device's d_sol_len / d_sol_lits, or
// satmi_cdcl_batch_host's h_assign_len / h_assign with cap = 1) against their
// clause sets, in one launch.
//
//   * One wavefront per instance, persistent over the batch: wave w of W takes
//     instances w, w + W, ... (no work counter, so the device form owns no
//     device memory and a launch is one kernel on the caller's stream).  The
//     wave checks the instance's rows one after the other.
//   * The truth table of a row lives in the wave's own LDS region: two bits per
//     variable v of 1 .. max_vars, bit 2(v & 15) of word v >> 4 for "+v is in
//     the row", the bit above it for "-v is in the row".  Lanes set the bits
//     with LDS atomics, 64 literals per step; the word an atomic returns tells
//     whether the opposite bit was already there (SATMI_CHECK_CONTRADICTORY:
//     of two opposite literals the one whose atomic comes second sees the
//     first, within a step or across steps).
//   * After a row the wave walks the same literals again and stores 0 to the
//     words they touched (every bit of such a word belongs to the row); the
//     table is wiped whole only once, when the wave starts.  A REF-mode
//     instance carries up to 1,024 rows over a handful of variables, so a wipe
//     per row would cost more than the rows.
//   * A literal l of the formula is true if l is in the row, false if -l is and
//     l is not, else unassigned (also a literal 0 or one beyond max_vars, which
//     the table cannot hold).  A clause is satisfied if some literal is true,
//     falsified if every literal is false (the empty clause always is), else
//     undetermined.
//   * Two clause forms, chosen per launch from max_clause_len:
//       short  1 <= max_clause_len <= CK_SHORT_MAX (8): a lane per clause, 64
//              clauses per wave step, the lane loops over its literals;
//       long   max_clause_len > 8 or 0 (unknown): the whole wave takes a clause
//              in 64-literal steps and settles it by ballots (the first step
//              with a true literal ends the clause).
//     The threshold is reasoned, not measured: a lane of the short form walks
//     its clause alone, so a wave step costs as many dependent loads as the
//     longest of its 64 clauses, and at 8 literals a lane's clause is the 32
//     bytes past which the lanes of one load no longer share cache lines; the
//     long form costs a step per clause, 64 per 64 clauses, whatever its length
//     up to 64.
//   * Counts are ballot popcounts (short form) or wave-uniform increments
//     settled by ballots (long form); the first falsified clause is a wave
//     minimum over the lanes' own first indices, relative to the instance's
//     first clause.
//   * Workgroups hold 4, 2 or 1 waves: whichever keeps the most waves resident
//     on a CU by LDS (the wider on a tie).  The table holds variables
//     1 .. SATMI_CHECK_MAX_VARS = 524,287: 32,768 words, 128 KiB, one one-wave
//     workgroup per CU of the 160 KiB.  Beyond it a call is
//     SATMI_ERR_TOO_LARGE before any launch.
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

constexpr int CK_SHORT_MAX = 8;   // longest clause of the lane-per-clause form
constexpr uint32_t CK_MAX_WORDS = ((uint32_t)SATMI_CHECK_MAX_VARS >> 4) + 1u;   // 32,768 words = 128 KiB
static_assert(4u * CK_MAX_WORDS <= LDS_PER_CU, "the largest table is one wave's LDS region");

struct CheckArgs {
    const int32_t *icb, *clb, *lits;   // the formulas (CSR)
    const int32_t *rows;               // [B] rows to check per instance, or null = cap
    const int32_t *len;                // [B x cap]
    const int32_t *row_lits;           // [B x cap x stride]
    int32_t *out;                      // [B x cap x SATMI_CHECK_NWORDS]
    int num_instances, cap, stride;
    uint32_t max_vars;
    uint32_t region_words;             // LDS words of one wave's table, a multiple of 4
};

// What the table says of literal l: bit 0 = l is in the row, bit 1 = -l is.
// 0 (unassigned) for a literal the table does not hold.
__device__ __forceinline__ uint32_t ck_lookup(const uint32_t *table, int32_t l, uint32_t max_vars) {
    const uint32_t v = l < 0 ? 0u - (uint32_t)l : (uint32_t)l;   // INT32_MIN: 2^31 > max_vars
    if (v - 1u >= max_vars) return 0u;
    const uint32_t pair = (table[v >> 4] >> (2u * (v & 15u))) & 3u;
    return l < 0 ? ((pair >> 1) | (pair << 1)) & 3u : pair;
}

template <bool LONG>
__global__ void __launch_bounds__(256) check_kernel(CheckArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ck_lds[];
    const int ln = lane_id(), wv = (int)threadIdx.x >> 6, wpg = (int)blockDim.x >> 6;
    uint32_t *table = ck_lds + (size_t)wv * A.region_words;
    for (uint32_t t = (uint32_t)ln; t < A.region_words; t += 64u) table[t] = 0u;
    wave_sync();
    const int64_t W = (int64_t)gridDim.x * wpg;
    for (int64_t b = (int64_t)blockIdx.x * wpg + wv; b < A.num_instances; b += W) {
        const int c0 = A.icb[b], m = A.icb[b + 1] - c0;
        const int nrows = A.rows ? min(max(A.rows[b], 0), A.cap) : A.cap;
        for (int r = 0; r < A.cap; ++r) {
            const int64_t row = b * A.cap + r;
            int32_t *o = A.out + row * SATMI_CHECK_NWORDS;
            if (r >= nrows) {   // a row past the instance's count: four zero words
                if (ln < SATMI_CHECK_NWORDS) o[ln] = 0;
                continue;
            }
            const int L = min(max(A.len[row], 0), A.stride);   // never read past the row
            const int32_t *rl = A.row_lits + row * A.stride;
            // ---- the row into the table
            int flags = 0;
            for (int i0 = 0; i0 < L; i0 += 64) {
                const int i = i0 + ln;
                bool bad = false, both = false;
                if (i < L) {
                    const int32_t l = rl[i];
                    const uint32_t v = l < 0 ? 0u - (uint32_t)l : (uint32_t)l;
                    bad = v - 1u >= A.max_vars;   // 0, INT32_MIN, beyond the table: ignored
                    if (!bad) {
                        const uint32_t sh = 2u * (v & 15u) + (l < 0 ? 1u : 0u);
                        const uint32_t old = atomicOr(table + (v >> 4), 1u << sh);
                        both = (old >> (sh ^ 1u)) & 1u;
                    }
                }
                if (__ballot(bad)) flags |= SATMI_CHECK_BAD_LITERAL;
                if (__ballot(both)) flags |= SATMI_CHECK_CONTRADICTORY;
            }
            wave_sync();
            // ---- the clauses
            int nfals = 0, nund = 0, first = INT_MAX;
            if (!LONG) {
                for (int cb = 0; cb < m; cb += 64) {
                    const int c = cb + ln;
                    bool fals = false, und = false;
                    if (c < m) {
                        const int s = A.clb[c0 + c], e = A.clb[c0 + c + 1];
                        bool sat = false, all_false = true;
                        for (int j = s; j < e; ++j) {
                            const uint32_t st = ck_lookup(table, A.lits[j], A.max_vars);
                            sat |= (st & 1u) != 0u;
                            all_false &= st == 2u;
                        }
                        fals = !sat && all_false;
                        und = !sat && !all_false;
                    }
                    nfals += __popcll(__ballot(fals));
                    nund += __popcll(__ballot(und));
                    if (fals) first = min(first, c);
                }
            } else {
                for (int c = 0; c < m; ++c) {
                    const int s = uniform_i32(A.clb[c0 + c]), e = uniform_i32(A.clb[c0 + c + 1]);
                    bool sat = false, open = false;   // open: some literal is not false
                    for (int j0 = s; j0 < e && !sat; j0 += 64) {
                        const int j = j0 + ln;
                        uint32_t st = 2u;   // a lane past the clause's end decides nothing
                        if (j < e) st = ck_lookup(table, A.lits[j], A.max_vars);
                        sat = __ballot((st & 1u) != 0u) != 0ull;
                        open |= __ballot(st != 2u) != 0ull;
                    }
                    if (!sat) {
                        if (open) {
                            ++nund;
                        } else {
                            ++nfals;
                            first = min(first, c);
                        }
                    }
                }
            }
            first = wave_min_i32(first);
            if (ln < SATMI_CHECK_NWORDS)
                o[ln] = ln == 0 ? nfals : ln == 1 ? nund : ln == 2 ? (first == INT_MAX ? -1 : first) : flags;
            // ---- clear by replay: the words this row's literals touched
            wave_sync();
            for (int i0 = 0; i0 < L; i0 += 64) {
                const int i = i0 + ln;
                if (i < L) {
                    const int32_t l = rl[i];
                    const uint32_t v = l < 0 ? 0u - (uint32_t)l : (uint32_t)l;
                    if (v - 1u < A.max_vars) table[v >> 4] = 0u;
                }
            }
            wave_sync();
        }
    }
}

// ------------------------------------------------------------------ host side
namespace {

constexpr OomText CK_OOM{"satmi_check_models_host", "split the batch"};

std::atomic<int> g_dbg_grid{0}, g_dbg_wpg{0};   // satmi_check_debug_grid

struct CheckWork : BatchWork {};   // a pool of its own (keys_out, rec_off stay empty)

int too_large(const char *who, int64_t max_vars) {
    set_error(std::string(who) + ": variable " + std::to_string(max_vars) + " is beyond the table's " +
              std::to_string(SATMI_CHECK_MAX_VARS));
    return SATMI_ERR_TOO_LARGE;
}

// One launch on `s`; every argument is checked by the caller.
int check_launch(const char *who, CheckArgs A, int max_clause_len, hipStream_t s) {
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
    const bool long_form = max_clause_len <= 0 || max_clause_len > CK_SHORT_MAX;
    const void *fn = long_form ? (const void *)check_kernel<true> : (const void *)check_kernel<false>;
    SATMI_TRY(batch_allow_lds(fn, lds_bytes));
    if (long_form)
        hipLaunchKernelGGL(check_kernel<true>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    else
        hipLaunchKernelGGL(check_kernel<false>, dim3(grid), dim3(64 * wpg), lds_bytes, s, A);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

}  // namespace

}  // namespace satmi

using namespace satmi;

extern "C" int satmi_check_debug_grid(int workgroups, int waves_per_wg) {
    if (workgroups < 0 || !(waves_per_wg == 0 || waves_per_wg == 1 || waves_per_wg == 2 || waves_per_wg == 4))
        return fail_arg("satmi_check_debug_grid", "workgroups >= 0 and waves_per_wg one of 0, 1, 2, 4");
    g_dbg_grid = workgroups;
    g_dbg_wpg = waves_per_wg;
    return SATMI_OK;
}

extern "C" int satmi_check_models_device(int num_instances, const int32_t *d_inst_clause_begin,
                                         const int32_t *d_clause_lit_begin, const int32_t *d_lits, int max_vars,
                                         int max_clause_len, const int32_t *d_rows, const int32_t *d_len,
                                         const int32_t *d_row_lits, int cap, int stride, int32_t *d_out,
                                         void *stream) {
    const char *who = "satmi_check_models_device";
    if (num_instances < 0) return fail_arg(who, "negative formula count");
    if (cap < 1) return fail_arg(who, "cap < 1");
    if (stride < 1) return fail_arg(who, "stride < 1");
    if (max_vars < 0 || max_clause_len < 0) return fail_arg(who, "negative max_vars / max_clause_len");
    if (num_instances == 0) return SATMI_OK;
    if (!d_inst_clause_begin || !d_clause_lit_begin || !d_lits || !d_len || !d_row_lits || !d_out)
        return fail_arg(who, "null pointer");
    if (max_vars > SATMI_CHECK_MAX_VARS) return too_large(who, max_vars);
    CheckArgs A{};
    A.icb = d_inst_clause_begin;
    A.clb = d_clause_lit_begin;
    A.lits = d_lits;
    A.rows = d_rows;
    A.len = d_len;
    A.row_lits = d_row_lits;
    A.out = d_out;
    A.num_instances = num_instances;
    A.cap = cap;
    A.stride = stride;
    A.max_vars = (uint32_t)max_vars;
    return check_launch(who, A, max_clause_len, (hipStream_t)stream);
}

extern "C" int satmi_check_models_host(int num_instances, const int32_t *h_inst_clause_begin,
                                       const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                       const int32_t *h_rows, const int32_t *h_len, const int32_t *h_row_lits,
                                       int cap, int stride, int32_t *h_out) {
    const char *who = "satmi_check_models_host";
    // ---- check: all of it before any HIP call
    CsrShape sh;
    if (const char *bad = batch_csr_check(num_instances, h_inst_clause_begin, h_clause_lit_begin, h_lits,
                                          cap < 1 ? "cap < 1" : stride < 1 ? "stride < 1" : nullptr,
                                          h_len && h_row_lits && h_out, &sh))
        return fail_arg(who, bad);
    if (num_instances == 0) return SATMI_OK;
    const int B = num_instances, C = sh.C, max_clause_len = sh.max_len;
    const int64_t Ltot = sh.Ltot;
    const size_t nrow = (size_t)B * (size_t)cap;
    int64_t max_vars = sh.max_var;
    for (int b = 0; b < B; ++b) {
        const int nr = h_rows ? h_rows[b] : cap;
        if (nr < 0 || nr > cap) return fail_arg(who, "row count outside 0 .. cap");
        for (int r = 0; r < nr; ++r) {
            const size_t row = (size_t)b * (size_t)cap + (size_t)r;
            const int n = h_len[row];
            if (n < 0 || n > stride) return fail_arg(who, "row length outside 0 .. stride");
            const int32_t *rl = h_row_lits + row * (size_t)stride;
            // (a literal 0 / INT32_MIN of a row is the kernel's to flag, not a variable)
            for (int i = 0; i < n; ++i)
                if (rl[i] != INT32_MIN) max_vars = std::max<int64_t>(max_vars, std::abs((int64_t)rl[i]));
        }
    }
    if (max_vars > SATMI_CHECK_MAX_VARS) return too_large(who, max_vars);

    // ---- lease the workspace
    int dev = 0;
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts, &dev));
    Lease<CheckWork> lease{Pool<CheckWork>::get().acquire(dev)};
    if (!lease.w) {
        set_error(std::string(who) + ": hipStreamCreate failed");
        return SATMI_ERR_HIP;
    }
    lease.ok = true;   // whatever the call's outcome (see BatchWork)
    CheckWork &wk = *lease.w;
    hipStream_t s = wk.stream;
    // ---- carve.  Inputs, one copy: clause ranges, literal ranges, literals, row counts, row lengths, rows
    Carve cu;
    const size_t u_icb = cu.take(4 * (size_t)(B + 1)), u_clb = cu.take(4 * ((size_t)C + 1));
    const size_t u_lits = cu.take(4 * (size_t)std::max<int64_t>(Ltot, 1)), u_rows = cu.take(4 * (size_t)B);
    const size_t u_len = cu.take(4 * nrow), u_rl = cu.take(4 * nrow * (size_t)stride), up_bytes = cu.at;
    const size_t out_bytes = 4 * nrow * SATMI_CHECK_NWORDS;
    SATMI_TRY(wk.up.reserve(up_bytes, &CK_OOM));
    SATMI_TRY(wk.out.reserve(out_bytes, &CK_OOM));
    SATMI_TRY(wk.up_h.grow(up_bytes));
    SATMI_TRY(wk.out_h.grow(out_bytes));
    std::memcpy(wk.up_h.p + u_icb, h_inst_clause_begin, 4 * (size_t)(B + 1));
    std::memcpy(wk.up_h.p + u_clb, h_clause_lit_begin, 4 * ((size_t)C + 1));
    if (Ltot > 0) std::memcpy(wk.up_h.p + u_lits, h_lits, 4 * (size_t)Ltot);
    if (h_rows) std::memcpy(wk.up_h.p + u_rows, h_rows, 4 * (size_t)B);
    std::memcpy(wk.up_h.p + u_len, h_len, 4 * nrow);
    std::memcpy(wk.up_h.p + u_rl, h_row_lits, 4 * nrow * (size_t)stride);
    SATMI_HIP(hipMemcpyAsync(wk.up.p, wk.up_h.p, up_bytes, hipMemcpyHostToDevice, s));

    const unsigned char *up = wk.up.as<unsigned char>();
    CheckArgs A{};
    A.icb = (const int32_t *)(up + u_icb);
    A.clb = (const int32_t *)(up + u_clb);
    A.lits = (const int32_t *)(up + u_lits);
    A.rows = h_rows ? (const int32_t *)(up + u_rows) : nullptr;
    A.len = (const int32_t *)(up + u_len);
    A.row_lits = (const int32_t *)(up + u_rl);
    A.out = wk.out.as<int32_t>();
    A.num_instances = B;
    A.cap = cap;
    A.stride = stride;
    A.max_vars = (uint32_t)max_vars;
    if (const int rc = check_launch(who, A, max_clause_len, s)) {
        (void)hipStreamSynchronize(s);   // the upload still reads the pinned words the next call fills
        return rc;
    }
    SATMI_HIP(hipMemcpyAsync(wk.out_h.p, wk.out.p, out_bytes, hipMemcpyDeviceToHost, s));
    SATMI_HIP(hipStreamSynchronize(s));
    std::memcpy(h_out, wk.out_h.p, out_bytes);
    return SATMI_OK;
}
