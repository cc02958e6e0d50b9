// dpll_scan.h -- launch interface of the clause-scan DPLL kernel (dpll_scan.hip),
// the SOUND-mode fast path behind satmi_dpll_batch_device (dpll.hip dispatches).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host.h"

namespace satmi {

constexpr int SPLIT_HELPERS_PER_CU = 1;   // measured: 1 best with two pipelined streams (4: -6 %, 8: -48 % at the N=8 share)
// nodes a search visits before it may donate: short searches (most of
// configs[1]) would only ship overhead to the helpers
constexpr int SPLIT_WARMUP_NODES = 256;

// What the caller of satmi_dpll_batch_device hands over (device pointers), the
// same for every DPLL kernel: the CSR batch, the limits, the outputs.
struct DpllBatch {
    const int32_t *inst_clause_begin, *clause_lit_begin, *lits, *inst_nvars;
    int num_instances, sol_cap, sol_stride;
    int64_t max_solutions, node_limit;
    uint64_t time_limit_ticks;
    int32_t *status;
    int64_t *counters;
    int32_t *sol_len, *sol_lits, *root_len, *root_lits;
};

// The batch into a kernel-argument struct (DpllArgs, ScanArgs), by field name:
// those keep their own member order, which the kernels' code depends on.
template <class Args>
void bind_batch(Args &A, const DpllBatch &B) {
    A.inst_clause_begin = B.inst_clause_begin;
    A.clause_lit_begin = B.clause_lit_begin;
    A.lits = B.lits;
    A.inst_nvars = B.inst_nvars;
    A.num_instances = B.num_instances;
    A.sol_cap = B.sol_cap;
    A.sol_stride = B.sol_stride;
    A.max_solutions = B.max_solutions;
    A.node_limit = B.node_limit;
    A.time_limit_ticks = B.time_limit_ticks;
    A.status = B.status;
    A.counters = B.counters;
    A.sol_len = B.sol_len;
    A.sol_lits = B.sol_lits;
    A.root_len = B.root_len;
    A.root_lits = B.root_lits;
}

struct ScanLaunch {
    DpllBatch batch;
    int max_vars, max_clauses, max_lits, max_clause_len;
    int num_cus;
    // the launch's stream with its work counter and scratch: the occurrence
    // lists of the incremental kernel and the splitting scratch come from it
    DpllStream *st;
    bool inc = false;   // incremental propagation (occurrence lists) instead of full clause scans
    // branch splitting of the launch's tail (dpll_scan.hip, "Splitting the tail")
    bool split = false;
    bool split_always = false;   // split any eligible launch (else only 1 <= instances per resident wave <= 8)
    int split_helpers_per_cu = SPLIT_HELPERS_PER_CU;   // waves per CU that stay as helpers once the queue drains
    int split_warmup = SPLIT_WARMUP_NODES;   // nodes of a search before its first donation
};

// Can the scan kernel take a batch of this shape (SOUND mode, no caller
// assignment)?  Fills *lds_bytes with the per-wave LDS it would use.
bool dpll_scan_eligible(int max_vars, int max_clauses, int max_lits, int max_clause_len, bool inc,
                        uint32_t *lds_bytes);

// Waves of the scan kernel resident per CU for this shape (LDS and registers),
// and the LDS bytes per wave of that launch (dynamic image + static literal states).
int dpll_scan_resident(int max_vars, int max_clauses, int max_clause_len, bool inc, int *waves_per_cu,
                       uint32_t *lds_per_wave = nullptr);

// The kernel form dpll_scan_launch would take for this shape: clause-word
// slots K (3 / 5), the static literal-state class (256 / 512 / 1024 / 4096; 0 =
// lv in each wave's dynamic image: the multi-wave workgroup form, and
// dpll_fixed_kernel), waves per workgroup, and whether it is dpll_fixed_kernel.
int dpll_scan_shape(int max_vars, int max_clauses, int max_clause_len, bool inc, int *K, int *lv_class,
                    int *waves_per_wg, int *fixed);

// Bytes of the splitting scratch head, and its statistics decoded from a host
// copy of it: [donations, tickets, claims, reclaims, helpers, handoffs, done].
constexpr int SPLIT_HEAD_BYTES = 512;
void dpll_split_decode(const void *head, int64_t out[7]);
int64_t dpll_split_busy(const void *head);   // wave ticks the launch's waves spent searching

// Launch on L.st->stream (asynchronous).  The caller has checked eligibility and
// zeroed L.st->counter on the stream.
int dpll_scan_launch(const ScanLaunch &L);

}  // namespace satmi
