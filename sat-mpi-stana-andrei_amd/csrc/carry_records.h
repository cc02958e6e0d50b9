// carry_records.h -- what satmi_cdcl_carry_batch_host does to its carried lemmas
// without the device: the check of the carry triple (a CSR pair: instance b
// carries clauses cib[b] .. cib[b + 1], clause c's literals are
// clits[ccb[c] .. ccb[c + 1])) and the records the kernel reads, one
// `len, lit_1 .. lit_len` per clause, every instance's chain behind the one
// before it.  Standard library only, as batch_keys.h is, so a plain host
// compiler builds it (`make carry-check`, tools/carry_records_check.cpp).
#pragma once
#include <stdint.h>

namespace satmi {

// What is wrong with a carry triple over B > 0 instances of inst_nvars[b]
// variables, or nullptr; then *image_words is the number of words of all the
// records.  Three null pointers carry nothing.  No clause may be empty (the
// closing record of an earlier answer is never carried), and every literal is
// one over its instance's variables.
inline const char *carry_triple_check(int B, const int32_t *cib, const int32_t *ccb, const int32_t *clits,
                                      const int32_t *inst_nvars, int64_t *image_words) {
    *image_words = 0;
    if (!cib && !ccb && !clits) return nullptr;
    if (!cib || !ccb) return "null pointer";
    if (cib[0] < 0) return "carry clause ranges are not ascending";
    for (int b = 0; b < B; ++b)
        if (cib[b + 1] < cib[b]) return "carry clause ranges are not ascending";
    const int c0 = cib[0], c1 = cib[B];
    if (ccb[c0] < 0) return "carry literal ranges are not ascending";
    for (int c = c0; c < c1; ++c)
        if (ccb[c + 1] < ccb[c]) return "carry literal ranges are not ascending";
    for (int c = c0; c < c1; ++c)
        if (ccb[c + 1] == ccb[c]) return "empty carried clause";
    if (ccb[c1] > ccb[c0] && !clits) return "null pointer";
    for (int b = 0; b < B; ++b)
        for (int j = ccb[cib[b]]; j < ccb[cib[b + 1]]; ++j) {
            const int32_t x = clits[j];
            if (x == 0 || x == INT32_MIN) return "carried literal 0 / INT32_MIN";
            if ((x < 0 ? -(int64_t)x : (int64_t)x) > (int64_t)inst_nvars[b]) return "carried literal beyond inst_nvars";
        }
    *image_words = ((int64_t)c1 - c0) + ((int64_t)ccb[c1] - ccb[c0]);
    return nullptr;
}

// The records of a checked triple: instance b's chain is image[begin[b] ..
// begin[b + 1]) (begin has B + 1 entries, from 0), and carry[2b], carry[2b + 1]
// are its record and word counts, the kernel's carry_in.  Without a triple
// every count is 0.
inline void carry_records_layout(int B, const int32_t *cib, const int32_t *ccb, const int32_t *clits, int64_t *begin,
                                 int32_t *image, int64_t *carry) {
    int64_t at = 0;
    begin[0] = 0;
    for (int b = 0; b < B; ++b) {
        const int cb = cib ? cib[b] : 0, ce = cib ? cib[b + 1] : 0;
        for (int c = cb; c < ce; ++c) {
            const int s = ccb[c], e = ccb[c + 1];
            image[at++] = e - s;
            for (int j = s; j < e; ++j) image[at++] = clits[j];
        }
        carry[2 * b] = ce - cb;
        carry[2 * b + 1] = at - begin[b];
        begin[b + 1] = at;
    }
}

}  // namespace satmi
