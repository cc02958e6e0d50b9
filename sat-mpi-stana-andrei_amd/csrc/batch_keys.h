// batch_keys.h -- what the entry points that take CSR host arrays do to a batch
// without the device: the check of the arrays and, from the same walk, the
// batch's shape (every host entry point; one formula is a batch of one), and
// for the two batched key solvers (resolution_batch.hip, dp_batch.hip) every
// clause as one 64-bit key over its formula's dense variable index, and a key
// back into literals.  Standard library only, so a plain host compiler builds
// it (`make keys-check`, tools/batch_keys_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

namespace satmi {

constexpr int BATCH_MAXVARS = 31;      // distinct variables of a formula whose clauses are keys
constexpr int BATCH_D2V_STRIDE = 32;   // ints of a formula's dense index -> variable id row

// ---------------------------------------------------------------- the check
// What the walk over a batch's arrays measures.  The arrays hold clauses
// 0 .. C and literals L0 .. Ltot, all of which a call uploads: max_len,
// min_len and max_var are over all of them; max_clauses and max_lits are one
// formula's.
struct CsrShape {
    int C = 0;                           // icb[B]
    int64_t L0 = 0, Ltot = 0;            // clb[0], clb[C]
    int max_clauses = 0, max_lits = 0;
    int max_len = 0, min_len = INT32_MAX;   // (min_len: INT32_MAX without a clause)
    int max_var = 0;                     // largest |literal|
};

constexpr const char *CSR_BAD_LITERAL = "literal 0 / INT32_MIN";

// What is wrong with a batch in CSR form (formula b's clauses are
// icb[b] .. icb[b + 1], clause c's literals clb[c] .. clb[c + 1]), or nullptr;
// then `shape`, if given, is the batch's, and `nvars`, if given, holds the
// largest |literal| of each of the B formulas.
// The caller's own checks keep their rank: `own`, its complaint about its other
// arguments, goes right behind the count; `outs`, whether the output pointers
// of a non-empty batch are all there, goes with the input pointers.
// (The loops over clauses and literals are flat and without early exits, so
// the compiler vectorises them: a batch of 32,768 menu formulas is ~5 M
// literals, read once per call.)
inline const char *batch_csr_check(int B, const int32_t *icb, const int32_t *clb, const int32_t *lits,
                                   const char *own = nullptr, bool outs = true, CsrShape *shape = nullptr,
                                   int32_t *nvars = nullptr) {
    if (B < 0) return "negative formula count";
    if (own) return own;
    CsrShape sh;
    if (shape) *shape = sh;
    if (B == 0) return nullptr;
    if (!icb || !clb || !outs) return "null pointer";
    if (icb[0] < 0) return "clause ranges are not ascending";
    for (int b = 0; b < B; ++b)
        if (icb[b + 1] < icb[b]) return "clause ranges are not ascending";
    const int C = sh.C = icb[B];
    int bad = clb[0] < 0;
    for (int c = 0; c < C; ++c) {
        bad |= clb[c + 1] < clb[c];
        const int len = (int)((uint32_t)clb[c + 1] - (uint32_t)clb[c]);
        sh.max_len = std::max(sh.max_len, len);
        sh.min_len = std::min(sh.min_len, len);
    }
    if (bad) return "literal ranges are not ascending";
    sh.L0 = clb[0];
    sh.Ltot = clb[C];
    if (sh.Ltot > 0 && !lits) return "null pointer";
    bad = 0;
    const auto scan = [&](int64_t lo, int64_t hi) {   // largest |literal| of lo .. hi
        uint32_t m = 0;
        for (int64_t j = lo; j < hi; ++j) {
            const int32_t x = lits[j];
            bad |= (x == 0) | (x == INT32_MIN);
            m = std::max(m, x < 0 ? 0u - (uint32_t)x : (uint32_t)x);
        }
        return (int)std::min<uint32_t>(m, INT32_MAX);
    };
    // (with icb[0] > 0 the arrays hold clauses before the first formula's)
    sh.max_var = nvars ? scan(sh.L0, clb[icb[0]]) : scan(sh.L0, sh.Ltot);
    for (int b = 0; b < B; ++b) {
        const int cb = icb[b], ce = icb[b + 1];
        sh.max_clauses = std::max(sh.max_clauses, ce - cb);
        sh.max_lits = std::max(sh.max_lits, clb[ce] - clb[cb]);
        if (nvars) sh.max_var = std::max(sh.max_var, nvars[b] = scan(clb[cb], clb[ce]));
    }
    if (bad) return CSR_BAD_LITERAL;
    if (shape) *shape = sh;
    return nullptr;
}

// One formula (clause c's literals clause_off[c] .. clause_off[c + 1]) as a
// batch of one.  Without clauses it reads neither array.
inline const char *formula_csr_check(int nclauses, const int32_t *clause_off, const int32_t *lits,
                                     const char *own, bool outs, CsrShape *shape) {
    static const int32_t none[1] = {0};
    const int32_t icb[2] = {0, nclauses};
    return batch_csr_check(1, icb, nclauses == 0 ? none : clause_off, lits,
                           nclauses < 0 ? "negative clause count" : own, outs, shape);
}

// ---------------------------------------------------------------- the encoder
struct BatchKeys {
    std::vector<int32_t> nvars;   // [B] distinct variables of each formula (past 2^20: 2^20)
    std::vector<uint64_t> keys;   // [max(C, 1)] every clause's key; 0 for a formula of more than 31 variables
    std::vector<int32_t> d2v;     // [B x 32] dense index -> variable id; zeros for such a formula
};

// The dense variable index of every formula of a checked batch (variables in
// ascending order of their ids, as host.h's dense_var_index numbers them) and
// the keys P | N << 32 of its clauses: bit i of P for +d2v[i], of N for
// -d2v[i].  A repeated literal is one bit, a tautological clause keeps both of
// its bits, the empty clause is key 0; bit 31 of P and N is never set.
inline void batch_encode(int B, const int32_t *icb, const int32_t *clb, const int32_t *lits, BatchKeys *out) {
    const int C = B > 0 ? icb[B] : 0;
    out->nvars.assign((size_t)B, 0);
    out->keys.assign((size_t)std::max(C, 1), 0ull);
    out->d2v.assign((size_t)B * BATCH_D2V_STRIDE, 0);
    std::vector<int32_t> vars;
    for (int b = 0; b < B; ++b) {
        const int cb = icb[b], ce = icb[b + 1];
        const int64_t lb = clb[cb], le = clb[ce];
        int32_t *dv = out->d2v.data() + (size_t)b * BATCH_D2V_STRIDE;
        uint32_t mv = 0;
        for (int64_t j = lb; j < le; ++j) mv = std::max(mv, (uint32_t)std::abs(lits[j]));
        const auto encode = [&](auto index_of) {   // the formula's keys, by its variables' dense index
            for (int c = cb; c < ce; ++c) {
                uint64_t k = 0;
                for (int64_t j = clb[c]; j < clb[c + 1]; ++j)
                    k |= 1ull << (index_of(std::abs(lits[j])) + (lits[j] < 0 ? 32 : 0));
                out->keys[(size_t)c] = k;
            }
        };
        int d;
        if (mv <= 63) {   // the common case: the variable set is one word
            uint64_t used = 0;
            for (int64_t j = lb; j < le; ++j) used |= 1ull << std::abs(lits[j]);
            d = __builtin_popcountll(used);
            if (d <= BATCH_MAXVARS) {
                encode([&](int v) { return __builtin_popcountll(used & ((1ull << v) - 1ull)); });
                for (int v = 1, n = 0; v <= 63; ++v)
                    if ((used >> v) & 1ull) dv[n++] = v;
            }
        } else {
            vars.clear();
            for (int64_t j = lb; j < le; ++j) vars.push_back(std::abs(lits[j]));
            std::sort(vars.begin(), vars.end());
            vars.erase(std::unique(vars.begin(), vars.end()), vars.end());
            d = (int)std::min<size_t>(vars.size(), 1 << 20);
            if (d <= BATCH_MAXVARS) {
                encode([&](int v) { return (int)(std::lower_bound(vars.begin(), vars.end(), v) - vars.begin()); });
                std::copy(vars.begin(), vars.end(), dv);
            }
        }
        out->nvars[(size_t)b] = d;
    }
}

// ---------------------------------------------------------------- the decoder
// A key's literals through its formula's d2v row `dv` of `nvars` <= 32 ids, in
// ascending variable id, +v before -v, into lits[64]; returns how many.
inline int batch_decode(uint64_t key, const int32_t *dv, int nvars, int32_t *lits) {
    int n = 0;
    for (int i = 0; i < nvars; ++i) {
        if ((key >> i) & 1ull) lits[n++] = dv[i];
        if ((key >> (32 + i)) & 1ull) lits[n++] = -dv[i];
    }
    return n;
}

}  // namespace satmi
