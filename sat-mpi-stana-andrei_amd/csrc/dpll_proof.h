// dpll_proof.h -- the pack step of satmi_dpll_refutations_device (dpll_proof.hip):
// the per-instance lemma logs of a logging DPLL launch (dpll.hip) become the
// compact CSR triple the refutation check reads.  Host declarations only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace satmi {

struct ProofPack {
    int32_t num_instances;
    const int32_t *status;       // [B]       the logging launch's statuses
    const int64_t *counters;     // [B x 8]   ... and counters
    const int32_t *log;          // the log, instance b's records from log_begin[b]
    const int64_t *log_begin;    // [B + 1]
    int64_t *info;               // [B x SATMI_DPLL_PROOF_NWORDS]; the pack writes word 3
    int32_t *pib;                // [B + 1]             proof_inst_begin
    int32_t *pcb;                // [clause_cap + 1]    proof_clause_begin
    int32_t *plits;              // [lit_cap]           proof_lits
    int64_t clause_cap, lit_cap;
    int64_t *totals;             // [2] lemmas and literals of the whole proof
};

// Two launches on `s`: the scan over the instances (one workgroup), then the
// copy (one wavefront per instance).  Every argument is checked by the caller.
int dpll_proof_pack(const ProofPack &P, hipStream_t s);

}  // namespace satmi
