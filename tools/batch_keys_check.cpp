// batch_keys_check.cpp -- csrc/batch_keys.h against a naive restatement, as a
// stand-alone host program (`make keys-check` builds it under AddressSanitizer
// and UBSan and runs it; no GPU, no HIP).  Seeded random batches mix, in one
// batch, formulas on the encoder's one-word path (ids <= 63) and on its sorted
// path (an id above 63, INT32_MAX among them), with 30 .. 33 distinct variables
// on either, repeated literals, tautologies, empty clauses and empty formulas;
// the naive side is a std::map from variable id to rank and one bit per
// literal.  Every key is decoded back and compared with the clause's literal
// set in the decoder's order, and every message of the CSR check is provoked.
// The shape the check measures (CsrShape, nvars) is held to a restatement over
// the formulas themselves: on every batch above, on every formula of them as a
// batch of one, and on the batches laid out as a window into larger arrays
// (icb[0] > 0, clb[0] > 0).  Exit status 1 on the first mismatch.
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "batch_keys.h"

using namespace satmi;
using Formula = std::vector<std::vector<int32_t>>;

static int g_checks = 0;
#define CHECK(cond, ...)                                    \
    do {                                                    \
        ++g_checks;                                         \
        if (!(cond)) {                                      \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                       \
            std::printf("\n");                              \
            std::exit(1);                                   \
        }                                                   \
    } while (0)

// `fs` in CSR form; as a window: behind `pad` literals that belong to no clause
// (zeros: never read) and the clauses `pre` that belong to no formula
struct Csr {
    std::vector<int32_t> icb, clb, lits;
    explicit Csr(const std::vector<Formula> &fs, const Formula &pre = {}, size_t pad = 0) : lits(pad, 0) {
        clb.push_back((int32_t)pad);
        for (const auto &c : pre) {
            lits.insert(lits.end(), c.begin(), c.end());
            clb.push_back((int32_t)lits.size());
        }
        icb.push_back((int32_t)pre.size());
        for (const Formula &f : fs) {
            for (const auto &c : f) {
                lits.insert(lits.end(), c.begin(), c.end());
                clb.push_back((int32_t)lits.size());
            }
            icb.push_back((int32_t)clb.size() - 1);
        }
    }
};

// d distinct variable ids: all <= 63 (`sparse` false: the one-word path), or
// with at least one above 63 (the sorted path)
static std::vector<int32_t> draw_ids(std::mt19937_64 &rng, int d, bool sparse) {
    std::set<int32_t> ids;
    if (!sparse) {
        while ((int)ids.size() < d) ids.insert(1 + (int32_t)(rng() % 63));
    } else {
        static const int32_t far[] = {64, 65, 127, 128, 1000, 65536, INT32_MAX - 1, INT32_MAX};
        ids.insert(far[rng() % 8]);
        if (rng() % 2) ids.insert(INT32_MAX);
        while ((int)ids.size() < d) {
            const int kind = (int)(rng() % 3);
            ids.insert(kind == 0 ? 1 + (int32_t)(rng() % 63)                      // below the threshold as well
                       : kind == 1 ? 64 + (int32_t)(rng() % 200)                  // dense just above it
                                   : 1 + (int32_t)(rng() % (uint64_t)INT32_MAX)); // anywhere
        }
        while ((int)ids.size() > d) ids.erase(ids.begin());   // (keeps the largest: still sparse)
    }
    return {ids.begin(), ids.end()};
}

// A formula over exactly the ids given: a cover that uses every id, then
// random clauses -- empty ones, repeated literals, tautologies
static Formula draw_formula(std::mt19937_64 &rng, const std::vector<int32_t> &ids) {
    Formula f;
    const int d = (int)ids.size();
    for (int i = 0; i < d; i += 3) {
        std::vector<int32_t> c;
        for (int k = i; k < std::min(i + 3, d); ++k) c.push_back(rng() % 2 ? ids[(size_t)k] : -ids[(size_t)k]);
        f.push_back(c);
    }
    const int extra = (int)(rng() % 8);
    for (int e = 0; e < extra; ++e) {
        std::vector<int32_t> c;
        const int len = (int)(rng() % 6);   // 0: the empty clause
        for (int k = 0; k < len; ++k) {
            const int32_t v = ids[rng() % (size_t)d];
            c.push_back(rng() % 2 ? v : -v);
        }
        if (len && rng() % 3 == 0) c.push_back(c[0]);      // a repeated literal
        if (len && rng() % 3 == 0) c.push_back(-c[0]);     // a tautology
        f.insert(f.begin() + (long)(rng() % (f.size() + 1)), c);
    }
    return f;
}

static uint32_t mag(int32_t l) { return l < 0 ? 0u - (uint32_t)l : (uint32_t)l; }

// The shape of `fs` behind `pad` literals and the clauses `pre`, restated over
// the formulas: clause by clause, literal by literal
static CsrShape naive_shape(const std::vector<Formula> &fs, const Formula &pre, size_t pad, std::vector<int32_t> *nvars) {
    CsrShape n;
    n.L0 = n.Ltot = (int64_t)pad;
    const auto clause = [&](const std::vector<int32_t> &c) {
        uint32_t m = 0;
        for (int32_t l : c) m = std::max(m, mag(l));
        ++n.C;
        n.Ltot += (int64_t)c.size();
        n.max_len = std::max(n.max_len, (int)c.size());
        n.min_len = std::min(n.min_len, (int)c.size());
        n.max_var = std::max(n.max_var, (int)m);
        return (int)m;
    };
    for (const auto &c : pre) clause(c);
    nvars->clear();
    for (const Formula &f : fs) {
        int nv = 0, nl = 0;
        for (const auto &c : f) nv = std::max(nv, clause(c)), nl += (int)c.size();
        nvars->push_back(nv);
        n.max_clauses = std::max(n.max_clauses, (int)f.size());
        n.max_lits = std::max(n.max_lits, nl);
    }
    return n;
}

static void check_same_shape(const CsrShape &g, const CsrShape &n, const char *what, const char *form) {
    CHECK(g.C == n.C && g.L0 == n.L0 && g.Ltot == n.Ltot, "%s (%s): C %d L0 %lld Ltot %lld, want %d %lld %lld", what,
          form, g.C, (long long)g.L0, (long long)g.Ltot, n.C, (long long)n.L0, (long long)n.Ltot);
    CHECK(g.max_clauses == n.max_clauses && g.max_lits == n.max_lits, "%s (%s): max_clauses %d max_lits %d, want %d %d",
          what, form, g.max_clauses, g.max_lits, n.max_clauses, n.max_lits);
    CHECK(g.max_len == n.max_len && g.min_len == n.min_len, "%s (%s): max_len %d min_len %d, want %d %d", what, form,
          g.max_len, g.min_len, n.max_len, n.min_len);
    CHECK(g.max_var == n.max_var, "%s (%s): max_var %d, want %d", what, form, g.max_var, n.max_var);
}

// The shape and every nvars[b] of a good batch, with and without nvars asked
// for, in the layout given; at offset 0 every formula as a batch of one besides
static void check_shape(const std::vector<Formula> &fs, const char *what, const Formula &pre = {}, size_t pad = 0) {
    const Csr a(fs, pre, pad);
    const int B = (int)fs.size();
    std::vector<int32_t> want_nv, nv((size_t)B, -7);
    const CsrShape want = naive_shape(fs, pre, pad, &want_nv);
    CsrShape got;
    got.C = -7;   // (an empty batch's shape is written too)
    CHECK(batch_csr_check(B, a.icb.data(), a.clb.data(), a.lits.data(), nullptr, true, &got) == nullptr,
          "%s: a good batch is refused (shape)", what);
    check_same_shape(got, B ? want : CsrShape{}, what, "shape");
    CHECK(batch_csr_check(B, a.icb.data(), a.clb.data(), a.lits.data(), nullptr, true, &got, nv.data()) == nullptr,
          "%s: a good batch is refused (shape, nvars)", what);
    check_same_shape(got, B ? want : CsrShape{}, what, "shape, nvars");
    for (int b = 0; b < B; ++b)
        CHECK(nv[(size_t)b] == want_nv[(size_t)b], "%s: formula %d: largest variable %d, want %d", what, b,
              nv[(size_t)b], want_nv[(size_t)b]);
    if (!pre.empty() || pad) return;
    for (int b = 0; b < B; ++b) {   // clause_off is the formula's slice of clb, rebased
        const Csr one({fs[(size_t)b]});
        std::vector<int32_t> one_nv;
        const CsrShape w1 = naive_shape({fs[(size_t)b]}, {}, 0, &one_nv);
        CHECK(formula_csr_check((int)fs[(size_t)b].size(), one.clb.data(), one.lits.data(), nullptr, true, &got) == nullptr,
              "%s: formula %d alone is refused", what, b);
        check_same_shape(got, w1, what, "batch of one");
        CHECK(got.max_var == one_nv[0] && got.max_clauses == got.C && got.max_lits == got.Ltot,
              "%s: formula %d alone: its shape is not the formula's", what, b);
    }
}

static void check_batch(const std::vector<Formula> &fs, const char *what) {
    const Csr a(fs);
    const int B = (int)fs.size();
    CHECK(batch_csr_check(B, a.icb.data(), a.clb.data(), a.lits.data()) == nullptr, "%s: a good batch is refused", what);
    check_shape(fs, what);
    BatchKeys K;
    batch_encode(B, a.icb.data(), a.clb.data(), a.lits.data(), &K);
    const size_t C = a.clb.size() - 1;
    CHECK(K.nvars.size() == (size_t)B && K.keys.size() == std::max<size_t>(C, 1) &&
              K.d2v.size() == (size_t)B * BATCH_D2V_STRIDE,
          "%s: array sizes", what);
    if (C == 0) CHECK(K.keys[0] == 0, "%s: the padding key", what);
    size_t c = 0;
    for (int b = 0; b < B; ++b) {
        std::map<int32_t, int> rank;   // variable id -> rank among the formula's ids
        for (const auto &cl : fs[(size_t)b])
            for (int32_t l : cl) rank[std::abs(l)] = 0;
        int n = 0;
        for (auto &kv : rank) kv.second = n++;
        const int d = (int)std::min<size_t>(rank.size(), (size_t)1 << 20);
        CHECK(K.nvars[(size_t)b] == d, "%s: formula %d: nvars %d, want %d", what, b, K.nvars[(size_t)b], d);
        const int32_t *dv = K.d2v.data() + (size_t)b * BATCH_D2V_STRIDE;
        const bool fit = d <= BATCH_MAXVARS;
        std::vector<int32_t> row(BATCH_D2V_STRIDE, 0);
        if (fit)
            for (const auto &kv : rank) row[(size_t)kv.second] = kv.first;
        CHECK(std::equal(row.begin(), row.end(), dv), "%s: formula %d: d2v row", what, b);
        for (const auto &cl : fs[(size_t)b]) {
            uint64_t want = 0;
            std::set<std::pair<int32_t, bool>> litset;   // (variable id, negative): the decoder's order
            for (int32_t l : cl) {
                if (fit) want |= 1ull << (rank[std::abs(l)] + (l < 0 ? 32 : 0));
                litset.insert({std::abs(l), l < 0});
            }
            CHECK(K.keys[c] == want, "%s: formula %d clause %zu: key %016llx, want %016llx", what, b, c,
                  (unsigned long long)K.keys[c], (unsigned long long)want);
            CHECK(!((K.keys[c] >> 31) & 1ull) && !(K.keys[c] >> 63), "%s: bit 31 of P or N is set", what);
            if (fit) {
                int32_t got[64];
                const int ng = batch_decode(K.keys[c], dv, d, got);
                std::vector<int32_t> exp;
                for (const auto &p : litset) exp.push_back(p.second ? -p.first : p.first);
                CHECK(ng == (int)exp.size() && std::equal(exp.begin(), exp.end(), got),
                      "%s: formula %d clause %zu: decode(encode) is not the clause", what, b, c);
            }
            ++c;
        }
    }
    CHECK(c == C, "%s: clause count", what);
}

static void check_named() {
    check_batch({}, "empty batch");
    check_batch({{}}, "one empty formula");
    check_batch({{}, {{}}, {{}, {}}}, "empty formulas and empty clauses");
    check_batch({{{1, 70, INT32_MAX}, {-INT32_MAX, -1}, {70, 70, -70}}}, "{1, 70, INT32_MAX}");
    check_batch({{{63, -63, 1}}, {{64, -64, 1}}}, "ids 63 and 64: either side of the threshold");
    Formula chain31, chain32, wide31, wide32;
    for (int i = 100; i < 130; ++i) chain31.push_back({i, -(i + 1)});
    for (int i = 100; i < 131; ++i) chain32.push_back({i, -(i + 1)});
    for (int i = 1; i < 31; ++i) wide31.push_back({2 * i, -(2 * i + 2)});
    for (int i = 1; i < 32; ++i) wide32.push_back({2 * i - 1, -(2 * i + 1)});
    check_batch({chain31, chain32, wide31, wide32}, "31 / 32 variables on both paths");
    // the variable count past 2^20 is reported as 2^20
    Formula huge(1);
    for (int32_t v = 64; v < 64 + (1 << 20) + 5; ++v) huge[0].push_back(v & 1 ? v : -v);
    check_batch({{{1}}, huge, {{-2}}}, "more than 2^20 variables");
}

static void check_shapes() {
    const Formula six = {{}, {1, -2, 3, -4, 5, -6}}, two = {{7, -8}, {9}}, pre = {{40, -41, 42}, {}, {-43}};
    check_shape({six}, "an empty clause beside a six-literal clause");
    {
        CsrShape sh;
        const Csr a({two, six});
        CHECK(batch_csr_check(2, a.icb.data(), a.clb.data(), a.lits.data(), nullptr, true, &sh) == nullptr &&
                  sh.min_len == 0 && sh.max_len == 6,
              "min_len 0 and max_len 6");
    }
    check_shape({{}, two, six}, "an empty formula first");
    check_shape({two, {}, six}, "an empty formula in the middle");
    check_shape({two, six, {}}, "an empty formula last");
    check_shape({{}, {}}, "no clause at all");
    // windows into larger arrays: clb[0] > 0, icb[0] > 0, both; the clauses
    // before the first formula's count for max_len, min_len and max_var only
    check_shape({two, {}, six}, "window: clb[0] > 0", {}, 5);
    check_shape({two, {}, six}, "window: icb[0] > 0", pre, 0);
    check_shape({two, {}, six}, "window: icb[0] > 0 and clb[0] > 0", pre, 5);
    check_shape({{}, two}, "window: an empty formula first", pre, 3);
    check_shape({two}, "window: a longer clause before the window", {{1, 2, 3, 4, 5, 6, 7, -99}}, 1);
    {   // the batch of one reads neither array without clauses, and names its count
        CsrShape sh;
        CHECK(formula_csr_check(0, nullptr, nullptr, nullptr, true, &sh) == nullptr && sh.C == 0 && sh.Ltot == 0,
              "a formula without clauses");
        const int32_t off[2] = {0, 1}, lit[1] = {5};
        CHECK(!std::strcmp(formula_csr_check(-1, off, lit, "own", true, &sh), "negative clause count"), "formula: count");
        CHECK(!std::strcmp(formula_csr_check(1, off, lit, "own", true, &sh), "own"), "formula: own");
        CHECK(!std::strcmp(formula_csr_check(1, nullptr, lit, nullptr, true, &sh), "null pointer"), "formula: clause_off");
        CHECK(!std::strcmp(formula_csr_check(1, off, nullptr, nullptr, true, &sh), "null pointer"), "formula: lits");
        CHECK(!std::strcmp(formula_csr_check(1, off, lit, nullptr, false, &sh), "null pointer"), "formula: outputs");
    }
}

static void check_random() {
    for (uint64_t seed = 1; seed <= 200; ++seed) {
        std::mt19937_64 rng(seed);
        std::vector<Formula> fs;
        // both paths at every variable count around the bound, in every batch
        for (int d : {30, 31, 32, 33})
            for (bool sparse : {false, true}) fs.push_back(draw_formula(rng, draw_ids(rng, d, sparse)));
        const int more = (int)(rng() % 24);
        for (int k = 0; k < more; ++k) {
            const int kind = (int)(rng() % 8);
            if (kind == 0) fs.push_back({});                           // an empty formula
            else if (kind == 1) fs.push_back(Formula(1 + rng() % 3));   // empty clauses only
            else fs.push_back(draw_formula(rng, draw_ids(rng, 1 + (int)(rng() % 40), rng() % 2)));
        }
        std::shuffle(fs.begin(), fs.end(), rng);
        char what[32];
        std::snprintf(what, sizeof what, "seed %llu", (unsigned long long)seed);
        check_batch(fs, what);
        check_shape(fs, what, draw_formula(rng, draw_ids(rng, 1 + (int)(rng() % 40), rng() % 2)), rng() % 9);
    }
}

static bool is(const char *got, const char *want) { return got && want ? !std::strcmp(got, want) : got == want; }

static void check_messages() {
    const std::vector<Formula> fs = {{{1, -2}, {3}}, {}, {{-70, 2}}};
    const Csr good(fs);
    const int B = 3;
    const int32_t *icb = good.icb.data(), *clb = good.clb.data(), *lits = good.lits.data();
    CsrShape sh;   // the same messages with the shape and nvars asked for
    int32_t nv[3];
    CHECK(is(batch_csr_check(B, icb, clb, lits), nullptr), "good");
    CHECK(is(batch_csr_check(-1, icb, clb, lits), "negative formula count"), "count");
    // the caller's own complaint ranks behind the count and before everything else
    CHECK(is(batch_csr_check(-1, nullptr, nullptr, nullptr, "own"), "negative formula count"), "count before own");
    CHECK(is(batch_csr_check(B, nullptr, clb, lits, "own"), "own"), "own before null");
    CHECK(is(batch_csr_check(0, nullptr, nullptr, nullptr, "own"), "own"), "own on an empty batch");
    // an empty batch has nothing else to check
    CHECK(is(batch_csr_check(0, nullptr, nullptr, nullptr, nullptr, false), nullptr), "empty batch");
    CHECK(is(batch_csr_check(B, nullptr, clb, lits), "null pointer"), "icb");
    CHECK(is(batch_csr_check(B, icb, nullptr, lits), "null pointer"), "clb");
    CHECK(is(batch_csr_check(B, icb, clb, nullptr), "null pointer"), "lits");
    CHECK(is(batch_csr_check(B, icb, clb, lits, nullptr, false), "null pointer"), "outputs");
    {   // no literals: the literal pointer is not needed
        const Csr e({{{}}, {}});
        CHECK(is(batch_csr_check(2, e.icb.data(), e.clb.data(), nullptr), nullptr), "no literals");
    }
    for (int at : {0, 1, 3}) {
        Csr x(fs);
        x.icb[(size_t)at] = at == 0 ? -1 : x.icb[(size_t)at - 1] - 1;
        CHECK(is(batch_csr_check(B, x.icb.data(), clb, lits), "clause ranges are not ascending"), "icb[%d]", at);
        CHECK(is(batch_csr_check(B, x.icb.data(), clb, lits, nullptr, true, &sh, nv), "clause ranges are not ascending"),
              "icb[%d] (shape)", at);
    }
    for (int at : {0, 2, 3}) {
        Csr x(fs);
        x.clb[(size_t)at] = at == 0 ? -1 : x.clb[(size_t)at - 1] - 1;
        CHECK(is(batch_csr_check(B, icb, x.clb.data(), lits), "literal ranges are not ascending"), "clb[%d]", at);
        CHECK(is(batch_csr_check(B, icb, x.clb.data(), lits, nullptr, true, &sh, nv), "literal ranges are not ascending"),
              "clb[%d] (shape)", at);
    }
    for (int32_t bad : {0, INT32_MIN})
        for (size_t at : {(size_t)0, good.lits.size() - 1}) {
            Csr x(fs);
            x.lits[at] = bad;
            CHECK(is(batch_csr_check(B, icb, clb, x.lits.data()), "literal 0 / INT32_MIN"), "literal %d", (int)bad);
            CHECK(batch_csr_check(B, icb, clb, x.lits.data(), nullptr, true, &sh, nv) == CSR_BAD_LITERAL,
                  "literal %d (shape)", (int)bad);
        }
    // the order among them: ranges before literals, clause ranges before literal ranges
    Csr x(fs);
    x.lits[0] = 0;
    x.clb[1] = -5;
    CHECK(is(batch_csr_check(B, icb, x.clb.data(), x.lits.data()), "literal ranges are not ascending"), "order");
    x.icb[2] = 0;
    CHECK(is(batch_csr_check(B, x.icb.data(), x.clb.data(), x.lits.data()), "clause ranges are not ascending"), "order");
}

int main() {
    check_messages();
    check_named();
    check_shapes();
    check_random();
    std::printf("batch_keys_check: ok (%d checks)\n", g_checks);
    return 0;
}
