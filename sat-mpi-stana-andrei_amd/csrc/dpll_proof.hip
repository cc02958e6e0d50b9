// dpll_proof.hip -- pack the lemma logs of a logging DPLL launch (dpll.hip's
// dpll_log_batch_kernel / dpll_log_wide_kernel) into the refutation check's
// CSR triple, on the launch's stream.
//
//   * An instance contributes its lemmas when it ended EXHAUSTED with no
//     solution and its log was not truncated, else none: the check then
//     reports it SATMI_REFUTE_OPEN.
//   * proof_scan_kernel (one workgroup) sums the contributions, decides whether
//     the totals fit the caller's capacities, and writes proof_inst_begin and
//     every instance's first literal offset by an exclusive scan.  Totals that
//     do not fit leave every instance with no lemma (proof_inst_begin all 0):
//     the caller reads the totals and calls again, and no consumer is handed
//     offsets into arrays that do not hold them.
//   * proof_copy_kernel (one wavefront per instance) walks the instance's
//     records `len, lit_1 .. lit_len` 64 log words at a time.  Which words are
//     record headers is a chain (a header tells where the next one is), walked
//     in scalar registers over the 64 loaded words; a lane then knows from the
//     header bitmap how many headers precede its word, which is all a header
//     needs for its clause offset and a literal for its place in proof_lits.
#include <hip/hip_runtime.h>

#include "dpll_proof.h"
#include "host.h"

namespace satmi {

namespace {

constexpr int SCAN_THREADS = 1024, SCAN_WAVES = SCAN_THREADS / 64;

__device__ __forceinline__ int64_t wave_incl_scan64(int64_t x) {
    const int ln = lane_id();
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up(x, d, 64);
        if (ln >= d) x += y;
    }
    return x;
}

// Lemmas and literals instance b contributes.
__device__ __forceinline__ void contribution(const ProofPack &P, int b, int64_t *n, int64_t *l) {
    const int64_t *w = P.info + (int64_t)b * SATMI_DPLL_PROOF_NWORDS;
    const bool whole = P.status[b] == SATMI_DPLL_EXHAUSTED &&
                       P.counters[(int64_t)b * SATMI_NCOUNTERS + SATMI_CTR_SOLUTIONS] == 0 &&
                       !(w[2] & SATMI_DPLL_PROOF_TRUNCATED);
    *n = whole ? w[0] : 0;
    *l = whole ? w[1] - w[0] : 0;
}

__global__ void __launch_bounds__(SCAN_THREADS) proof_scan_kernel(ProofPack P) {
    __shared__ int64_t wave_n[SCAN_WAVES], wave_l[SCAN_WAVES];
    __shared__ int64_t carry[2];
    __shared__ int fits_s;
    const int t = threadIdx.x, ln = t & 63, wv = t >> 6;
    const int B = P.num_instances;
    // ---- the totals
    int64_t sn = 0, sl = 0;
    for (int b = t; b < B; b += SCAN_THREADS) {
        int64_t n, l;
        contribution(P, b, &n, &l);
        sn += n;
        sl += l;
    }
    sn = wave_incl_scan64(sn);
    sl = wave_incl_scan64(sl);
    if (ln == 63) {
        wave_n[wv] = sn;
        wave_l[wv] = sl;
    }
    __syncthreads();
    if (t == 0) {
        int64_t tn = 0, tl = 0;
        for (int w = 0; w < SCAN_WAVES; ++w) {
            tn += wave_n[w];
            tl += wave_l[w];
        }
        P.totals[0] = tn;
        P.totals[1] = tl;
        const bool fits = tn <= P.clause_cap && tl <= P.lit_cap && tn <= INT32_MAX && tl <= INT32_MAX;
        fits_s = fits ? 1 : 0;
        carry[0] = carry[1] = 0;
        P.pib[B] = fits ? (int32_t)tn : 0;
        P.pcb[fits ? tn : 0] = fits ? (int32_t)tl : 0;
    }
    __syncthreads();
    const bool fits = fits_s != 0;
    // ---- the offsets: an exclusive scan, 1024 instances at a time
    for (int b0 = 0; b0 < B; b0 += SCAN_THREADS) {
        const int b = b0 + t;
        int64_t n = 0, l = 0;
        if (b < B) contribution(P, b, &n, &l);
        const int64_t in = wave_incl_scan64(n), il = wave_incl_scan64(l);
        if (ln == 63) {
            wave_n[wv] = in;
            wave_l[wv] = il;
        }
        __syncthreads();
        int64_t bn = carry[0], bl = carry[1];
        for (int w = 0; w < wv; ++w) {
            bn += wave_n[w];
            bl += wave_l[w];
        }
        if (b < B) {
            P.pib[b] = fits ? (int32_t)(bn + in - n) : 0;
            P.info[(int64_t)b * SATMI_DPLL_PROOF_NWORDS + 3] = fits ? bl + il - l : 0;
        }
        __syncthreads();
        if (t == SCAN_THREADS - 1) {
            carry[0] = bn + in;
            carry[1] = bl + il;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) proof_copy_kernel(ProofPack P) {
    const int ln = lane_id();
    const uint64_t lt = lanemask_lt();
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int b = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); b < P.num_instances; b += waves) {
        const int cb = P.pib[b];
        const int n = P.pib[b + 1] - cb;
        if (n <= 0) continue;   // no contribution, or totals that do not fit
        const int64_t *w = P.info + (int64_t)b * SATMI_DPLL_PROOF_NWORDS;
        const int64_t words = w[1], lbase = w[3];
        const int32_t *rec = P.log + P.log_begin[b];
        int64_t p = 0;   // the next header's word
        int64_t k = 0;   // headers before this chunk
        for (int64_t base = 0; base < words; base += 64) {
            const int64_t i = base + ln;
            const int32_t x = i < words ? rec[i] : 0;
            uint64_t hdr = 0;
            while (p < base + 64 && p < words) {
                const int at = uniform_i32((int)(p - base));
                const int len = __builtin_amdgcn_readlane(x, at);
                hdr |= 1ull << at;
                p += 1 + (int64_t)max(len, 0);
            }
            const int64_t kk = k + __popcll(hdr & lt);   // headers before this lane's word
            if (i < words) {
                if ((hdr >> ln) & 1ull) {
                    if (kk < n && cb + kk < P.clause_cap) P.pcb[cb + kk] = (int32_t)(lbase + i - kk);
                } else {
                    const int64_t at = lbase + i - kk;
                    if (at < P.lit_cap) P.plits[at] = x;
                }
            }
            k += __popcll(hdr);
        }
    }
}

}  // namespace

int dpll_proof_pack(const ProofPack &P, hipStream_t s) {
    hipLaunchKernelGGL(proof_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, P);
    SATMI_HIP(hipGetLastError());
    const int wgs = std::min((P.num_instances + 3) / 4, 8192);
    hipLaunchKernelGGL(proof_copy_kernel, dim3(wgs), dim3(256), 0, s, P);
    SATMI_HIP(hipGetLastError());
    return SATMI_OK;
}

}  // namespace satmi
