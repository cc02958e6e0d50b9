// carry_records_check.cpp -- csrc/carry_records.h against a naive restatement, as a
// stand-alone host program (`make carry-check` builds it under AddressSanitizer
// and UBSan and runs it; no GPU, no HIP).  Seeded random carries, per instance a
// list of clauses, are written as a triple (also as a window into larger
// arrays: cib[0] > 0, ccb[cib[0]] > 0) into arrays of exactly the size the
// triple needs, so a read or write past one is caught; the layout is compared
// with the records built clause by clause.  Then every refusal is provoked, at
// random positions of random triples, and held to the naive side's verdict.
// Exit status 1 on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "carry_records.h"

using namespace satmi;
using Clauses = std::vector<std::vector<int32_t>>;

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

static bool is(const char *got, const char *want) { return got && want ? !std::strcmp(got, want) : got == want; }

// Per-instance clause lists as a triple, behind `pre` clauses of `pad` literals each that belong to no instance
struct Triple {
    std::vector<int32_t> cib, ccb, lits;
    Triple(const std::vector<Clauses> &cs, int pre, int pad) {
        ccb.push_back(0);
        for (int c = 0; c < pre; ++c) {
            for (int j = 0; j < pad; ++j) lits.push_back(0);   // never read
            ccb.push_back((int32_t)lits.size());
        }
        cib.push_back(pre);
        for (const Clauses &cl : cs) {
            for (const auto &c : cl) {
                lits.insert(lits.end(), c.begin(), c.end());
                ccb.push_back((int32_t)lits.size());
            }
            cib.push_back((int32_t)ccb.size() - 1);
        }
    }
};

// The naive side: the first complaint in the header's order of checks, over the lists themselves
static const char *naive_check(const std::vector<Clauses> &cs, const std::vector<int32_t> &nv, int64_t *words) {
    *words = 0;
    for (const Clauses &cl : cs)
        for (const auto &c : cl)
            if (c.empty()) return "empty carried clause";
    for (size_t b = 0; b < cs.size(); ++b)
        for (const auto &c : cs[b])
            for (int32_t l : c) {
                if (l == 0 || l == INT32_MIN) return "carried literal 0 / INT32_MIN";
                if (std::llabs((long long)l) > nv[b]) return "carried literal beyond inst_nvars";
            }
    for (const Clauses &cl : cs)
        for (const auto &c : cl) *words += 1 + (int64_t)c.size();
    return nullptr;
}

static std::vector<Clauses> draw(std::mt19937_64 &rng, int B, const std::vector<int32_t> &nv) {
    std::vector<Clauses> cs((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (nv[(size_t)b] == 0 || rng() % 4 == 0) continue;   // nothing carried
        const int n = 1 + (int)(rng() % 6);
        for (int c = 0; c < n; ++c) {
            const int len = rng() % 8 == 0 ? 60 + (int)(rng() % 10) : 1 + (int)(rng() % 5);
            std::vector<int32_t> cl;
            for (int j = 0; j < len; ++j) {
                const int32_t v = 1 + (int32_t)(rng() % (uint64_t)nv[(size_t)b]);
                cl.push_back(rng() % 2 ? v : -v);
            }
            cs[(size_t)b].push_back(cl);
        }
    }
    return cs;
}

// check + layout of a good or bad carry in the layout given, against the naive side
static void check_one(const std::vector<Clauses> &cs, const std::vector<int32_t> &nv, int pre, int pad, const char *what) {
    const int B = (int)cs.size();
    const Triple t(cs, pre, pad);
    int64_t want_words = 0, got_words = -7;
    const char *want = naive_check(cs, nv, &want_words);
    const char *got = carry_triple_check(B, t.cib.data(), t.ccb.data(), t.lits.data(), nv.data(), &got_words);
    CHECK(is(got, want), "%s: verdict '%s', want '%s'", what, got ? got : "ok", want ? want : "ok");
    if (want) {
        CHECK(got_words == 0, "%s: words of a refused carry", what);
        return;
    }
    CHECK(got_words == want_words, "%s: %lld words, want %lld", what, (long long)got_words, (long long)want_words);
    std::vector<int64_t> begin((size_t)B + 1, -7), carry((size_t)2 * B, -7);
    std::vector<int32_t> image((size_t)want_words, -7);   // exactly as large as the check said
    carry_records_layout(B, t.cib.data(), t.ccb.data(), t.lits.data(), begin.data(), image.data(), carry.data());
    std::vector<int32_t> rec;
    for (int b = 0; b < B; ++b) {
        CHECK(begin[(size_t)b] == (int64_t)rec.size(), "%s: instance %d begins at %lld", what, b, (long long)begin[(size_t)b]);
        int64_t w = 0;
        for (const auto &c : cs[(size_t)b]) {
            rec.push_back((int32_t)c.size());
            rec.insert(rec.end(), c.begin(), c.end());
            w += 1 + (int64_t)c.size();
        }
        CHECK(carry[(size_t)2 * b] == (int64_t)cs[(size_t)b].size() && carry[(size_t)2 * b + 1] == w,
              "%s: instance %d carries (%lld, %lld)", what, b, (long long)carry[(size_t)2 * b], (long long)carry[(size_t)2 * b + 1]);
    }
    CHECK(begin[(size_t)B] == want_words && rec == image, "%s: the records differ", what);
}

static void check_random() {
    for (uint64_t seed = 1; seed <= 400; ++seed) {
        std::mt19937_64 rng(seed);
        const int B = 1 + (int)(rng() % 12);
        std::vector<int32_t> nv;
        for (int b = 0; b < B; ++b) nv.push_back(rng() % 5 == 0 ? 0 : 1 + (int32_t)(rng() % 200));
        if (rng() % 10 == 0) nv[rng() % (size_t)B] = INT32_MAX;
        std::vector<Clauses> cs = draw(rng, B, nv);
        char what[48];
        std::snprintf(what, sizeof what, "seed %llu", (unsigned long long)seed);
        check_one(cs, nv, 0, 0, what);
        check_one(cs, nv, 1 + (int)(rng() % 3), (int)(rng() % 4), what);
        // one defect at a random place
        std::vector<std::pair<int, int>> at;   // (instance, clause)
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < (int)cs[(size_t)b].size(); ++c) at.push_back({b, c});
        if (at.empty()) continue;
        const auto pick = at[rng() % at.size()];
        auto &cl = cs[(size_t)pick.first][(size_t)pick.second];
        const size_t j = rng() % cl.size();
        const int kind = (int)(rng() % 5);
        std::snprintf(what, sizeof what, "seed %llu defect %d", (unsigned long long)seed, kind);
        if (kind == 0) cl.clear();
        else if (kind == 1) cl[j] = 0;
        else if (kind == 2) cl[j] = INT32_MIN;
        else if (nv[(size_t)pick.first] == INT32_MAX) continue;   // nothing lies beyond it
        else cl[j] = (kind == 3 ? 1 : -1) * (nv[(size_t)pick.first] + 1);
        int64_t w;
        CHECK(naive_check(cs, nv, &w) != nullptr, "%s: the defect is none", what);
        check_one(cs, nv, 0, 0, what);
        check_one(cs, nv, 2, 1, what);
    }
}

static void check_messages() {
    const std::vector<Clauses> cs = {{{-3}, {1, 2}}, {}, {{6, -4, 5}}};
    const std::vector<int32_t> nv = {3, 0, 6};
    const Triple good(cs, 0, 0);
    const int B = 3;
    int64_t w = -7;
    CHECK(is(carry_triple_check(B, good.cib.data(), good.ccb.data(), good.lits.data(), nv.data(), &w), nullptr) && w == 9,
          "good");
    // no triple at all carries nothing; a part of one is refused
    CHECK(is(carry_triple_check(B, nullptr, nullptr, nullptr, nv.data(), &w), nullptr) && w == 0, "no triple");
    CHECK(is(carry_triple_check(B, nullptr, good.ccb.data(), good.lits.data(), nv.data(), &w), "null pointer"), "cib");
    CHECK(is(carry_triple_check(B, good.cib.data(), nullptr, good.lits.data(), nv.data(), &w), "null pointer"), "ccb");
    CHECK(is(carry_triple_check(B, good.cib.data(), good.ccb.data(), nullptr, nv.data(), &w), "null pointer"), "lits");
    {   // no literals: the literal pointer is not needed, and every count is 0
        const int32_t cib[4] = {0, 0, 0, 0}, ccb[1] = {0};
        CHECK(is(carry_triple_check(B, cib, ccb, nullptr, nv.data(), &w), nullptr) && w == 0, "an empty triple");
        int64_t begin[4], carry[6];
        carry_records_layout(B, cib, ccb, nullptr, begin, nullptr, carry);
        for (int i = 0; i < 6; ++i) CHECK(carry[i] == 0 && begin[i % 4] == 0, "an empty triple's layout");
        carry_records_layout(B, nullptr, nullptr, nullptr, begin, nullptr, carry);
        for (int i = 0; i < 6; ++i) CHECK(carry[i] == 0 && begin[i % 4] == 0, "no triple's layout");
    }
    for (int at : {0, 1, 3}) {
        Triple x(cs, 0, 0);
        x.cib[(size_t)at] = at == 0 ? -1 : x.cib[(size_t)at - 1] - 1;
        CHECK(is(carry_triple_check(B, x.cib.data(), good.ccb.data(), good.lits.data(), nv.data(), &w),
                 "carry clause ranges are not ascending"), "cib[%d]", at);
    }
    for (int at : {0, 2, 3}) {
        Triple x(cs, 0, 0);
        x.ccb[(size_t)at] = at == 0 ? -1 : x.ccb[(size_t)at - 1] - 1;
        CHECK(is(carry_triple_check(B, good.cib.data(), x.ccb.data(), good.lits.data(), nv.data(), &w),
                 "carry literal ranges are not ascending"), "ccb[%d]", at);
    }
    // the order among them: ranges before empty clauses before literals; 0 before beyond
    Triple x(cs, 0, 0);
    x.lits[0] = 0;
    x.lits[1] = 9;
    CHECK(is(carry_triple_check(B, x.cib.data(), x.ccb.data(), x.lits.data(), nv.data(), &w), "carried literal 0 / INT32_MIN"),
          "order");
    x.ccb[2] = x.ccb[1];
    CHECK(is(carry_triple_check(B, x.cib.data(), x.ccb.data(), x.lits.data(), nv.data(), &w), "empty carried clause"), "order");
    x.cib[2] = 1;
    CHECK(is(carry_triple_check(B, x.cib.data(), x.ccb.data(), x.lits.data(), nv.data(), &w),
             "carry clause ranges are not ascending"), "order");
}

int main() {
    check_messages();
    check_random();
    std::printf("carry_records_check: ok (%d checks)\n", g_checks);
    return 0;
}
