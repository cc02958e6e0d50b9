// dp_batch.hip -- Davis-Putnam elimination (REF.py:98-130) of a batch of small
// clause sets in one launch on gfx950: one workgroup per formula, every step
// of the elimination in LDS.
//
// satmi_dp_host (dp.hip) eliminates one clause set per call, a chain of
// dependent launches per step, and a small step costs the chain whatever its
// work.  With at most 31 distinct variables a clause is one 64-bit key
// P | N << 32 over the formula's dense variable index (the packed resolution
// path's key; bit 31 of P and of N is never set, so ~0 is no key and key 0, the
// empty clause, is an ordinary one).  Then
//
//   * a persistent grid of workgroups draws formula indices from an atomic
//     work counter (as the resolution batch does);
//   * LDS per workgroup: the clause list and the next one (clause_cap keys
//     each), the pos and neg lists of the step (clause_cap each), and two
//     chunk buffers of DPB_CHUNK keys;
//   * a step: the live variable mask (an OR over the list), the variable
//     `variables.pop()` returns (below), the split into pos / neg / rest in
//     list order (ballot + prefix: no atomic decides an order; rest is the
//     head of the next list), then the pairs (i, j), pos-major, streamed in
//     chunks of DPB_CHUNK pairs in pair order;
//   * a chunk: (A) resolvent key and flags of every pair; the non-tautological
//     ones are counted and compacted in order; the first empty resolvent and
//     the resolvent that takes the count over clause_limit are events, the
//     earlier pair index wins; (B) every candidate is tested against the next
//     list as it stands (rest, then what earlier chunks kept: REF.py:122-125's
//     greedy filter as written), survivors compacted in order; (C) every
//     survivor is tested against the earlier survivors of its chunk -- by
//     induction one of those that is itself dropped has a kept subset earlier
//     still, which is a subset of the later survivor too -- and the kept ones
//     are appended to the next list in order.  A duplicate resolvent is the
//     superset of its first occurrence (or of what dropped that), so no table
//     of seen keys is needed for the result;
//   * the tested key stays in registers, the others are read as broadcasts,
//     two keys per 16-byte LDS read;
//   * a next list that outgrows clause_cap makes the formula UNFIT -- after the
//     step's remaining pairs were still scanned for an event, which ends the
//     elimination before the list would exist.
//
// The variable order without set images.  REF.py:103 pops from a set built
// afresh each step from n distinct positive ints.  Its table has 8 slots for
// n <= 4, 32 for n <= 18, 128 for n <= 76 (py_size_after, pyset_dev.h), and
// when the home slots id & mask are pairwise distinct every id sits at its
// home whatever the insertion order, so pop() returns the id of the lowest
// home slot.  The kernel keeps dense index -> id in LDS and applies that rule;
// a step whose live ids collide makes the formula UNFIT (the order is then not
// recoverable from the keys).
//
// The host side is shared with resolution_batch.hip: the check, the encoder and
// the decoder are batch_keys.h's, the workspace, the carving of the blocks and
// the grid size batch_host.h's.  The kernel's split, resolvent and filter
// restate dp.hip's: device code is not shared, so those kernels' machine code,
// which the bench's rooflines are keyed by, stays what it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "batch_host.h"
#include "common.h"

namespace satmi {

constexpr int DPB_CHUNK = 1024;      // pairs per chunk
constexpr int DPB_MAXVARS = BATCH_MAXVARS;   // distinct variables of a formula
constexpr int DPB_STEPS_MAX = 64;    // steps the device keeps rows for: a variable is popped at most twice
constexpr int DPB_NOEVENT = INT_MAX;

struct DpBatchArgs {
    const int32_t *icb;        // [B + 1] clause range of each formula
    const uint64_t *keys_in;   // [C] the input clauses' keys (host-encoded)
    const int32_t *nvars;      // [B] distinct variables of each formula
    const int32_t *d2v;        // [B x 32] dense index -> variable id
    int num_instances;
    int clause_cap;            // clauses a list may hold
    int64_t step_limit, clause_limit;
    int32_t *result, *steps;
    int32_t *trace;            // [B x step_cap]
    int64_t *step_clauses;     // [B x step_cap], zeroed before the launch
    int step_cap;
    uint64_t *keys_out;        // record: formula b's lists at rec_off[b] .. rec_off[b + 1]; or null
    const int64_t *rec_off;    // [B + 1]
    uint32_t *work;            // the work counter
};

// Three flags per lane -> each flag's exclusive prefix over the workgroup (in
// thread order) and its total, packed 21 bits apiece.  One barrier; `par`
// alternates the two count rows, so a row is rewritten only after a barrier
// that every reader of it has passed.
__device__ __forceinline__ uint64_t dpb_scan3(bool f0, bool f1, bool f2, uint64_t (*sh_w)[16], int &par,
                                              uint64_t *total) {
    const int wv = threadIdx.x >> 6, nwv = blockDim.x >> 6;
    const uint64_t m0 = __ballot(f0), m1 = __ballot(f1), m2 = __ballot(f2), lt = lanemask_lt();
    if (lane_id() == 0)
        sh_w[par][wv] = (uint64_t)__popcll(m0) | ((uint64_t)__popcll(m1) << 21) | ((uint64_t)__popcll(m2) << 42);
    __syncthreads();
    uint64_t pre = 0, tot = 0;
    for (int w = 0; w < nwv; ++w) {
        const uint64_t c = sh_w[par][w];
        if (w < wv) pre += c;
        tot += c;
    }
    par ^= 1;
    *total = tot;
    return pre + ((uint64_t)__popcll(m0 & lt) | ((uint64_t)__popcll(m1 & lt) << 21) |
                  ((uint64_t)__popcll(m2 & lt) << 42));
}
__device__ __forceinline__ int dpb_scan(bool f, uint64_t (*sh_w)[16], int &par, int *total) {
    uint64_t tot;
    const uint64_t pre = dpb_scan3(f, false, false, sh_w, par, &tot);
    *total = (int)(tot & 0x1FFFFFu);
    return (int)(pre & 0x1FFFFFu);
}

// Is one of list[0 .. n) a subset of r?  `want` is false for idle lanes; the
// loop runs while a lane of the wave still looks.  list is 16-byte aligned.
__device__ __forceinline__ bool dpb_subsumed(const uint64_t *list, int n, uint64_t r, bool want) {
    bool sub = false;
    const uint64_t nr = ~r;
    int e = 0;
    for (; e + 1 < n; e += 2) {
        if (!__ballot(want && !sub)) return sub;
        const ulonglong2 s = *(const ulonglong2 *)(list + e);
        sub |= !(s.x & nr) | !(s.y & nr);
    }
    if (e < n) sub |= !(list[e] & nr);
    return sub;
}

__global__ void __launch_bounds__(1024) dp_batch_kernel(DpBatchArgs A) {
    extern __shared__ __align__(16) uint64_t dpb_lds[];   // cur, next, pos, neg [clause_cap each], cand, surv [DPB_CHUNK each]
    __shared__ uint64_t sh_w[2][16];
    __shared__ int sh_d2v[32];
    __shared__ int sh_b, sh_pop, sh_evE, sh_evL;
    __shared__ uint32_t sh_live;
    const int cap = A.clause_cap, stride = (cap + 1) & ~1;   // every list starts 16-byte aligned
    uint64_t *cur = dpb_lds, *nxt = dpb_lds + stride;
    uint64_t *const pos = dpb_lds + 2 * (size_t)stride, *const neg = dpb_lds + 3 * (size_t)stride;
    uint64_t *const cand = dpb_lds + 4 * (size_t)stride, *const surv = cand + DPB_CHUNK;
    const int tid = threadIdx.x, T = blockDim.x, ln = lane_id();
    int par = 0;
    for (;;) {
        __syncthreads();   // the formula before this one is done with sh_b and the lists
        if (tid == 0) sh_b = (int)atomicAdd(A.work, 1u);
        __syncthreads();
        const int b = sh_b;
        if (b >= A.num_instances) break;   // workgroup-uniform
        const int c0 = A.icb[b], m = A.icb[b + 1] - c0, d = A.nvars[b];
        int result = 1, steps = 0, ncl = m;
        bool unfit = d > DPB_MAXVARS || m > cap;
        if (!unfit) {
            for (int c = tid; c < m; c += T) cur[c] = A.keys_in[c0 + c];
            if (tid < 32) sh_d2v[tid] = tid < d ? A.d2v[(size_t)b * 32 + tid] : 0;
        }
        int64_t rec_at = 0, rec_end = 0;
        if (A.keys_out) {
            rec_at = A.rec_off[b];
            rec_end = A.rec_off[b + 1];
        }
        while (!unfit) {
            if (tid == 0) {
                sh_live = 0u;
                sh_evE = sh_evL = DPB_NOEVENT;
            }
            __syncthreads();   // ... and the list is whole
            // ---- variables = {abs(lit) for clause in clauses for lit in clause}
            uint32_t lm = 0u;
            for (int c = tid; c < ncl; c += T) {
                const uint64_t k = cur[c];
                lm |= (uint32_t)k | (uint32_t)(k >> 32);
            }
            for (int o = 32; o; o >>= 1) lm |= (uint32_t)__shfl_xor((int)lm, o);
            if (ln == 0 && lm) atomicOr(&sh_live, lm);
            __syncthreads();
            const uint32_t live = sh_live;
            if (!live) break;                                          // while variables: (result stays True)
            if (A.step_limit > 0 && steps >= A.step_limit) {
                result = -1;
                break;
            }
            // ---- var = variables.pop(): the live id of the lowest home slot
            if (tid < 64) {
                const int n = __popc(live);
                const int mask = n <= 4 ? 7 : n <= 18 ? 31 : 127;   // py_size_after(n) - 1 for n <= 31
                const bool alive = ln < 32 && ((live >> (ln & 31)) & 1u);
                const int home = sh_d2v[ln & 31] & mask;
                bool coll = false;
                for (int k = 0; k < 32; ++k) {
                    const int hk = __shfl(home, k);
                    coll |= alive && k != ln && ((live >> k) & 1u) && hk == home;
                }
                const bool any = __ballot(coll) != 0ull;
                const int best = wave_min_i32(alive ? (home << 5) | ln : INT_MAX);
                if (tid == 0) sh_pop = any ? -1 : (best & 31);
            }
            __syncthreads();
            const int vi = sh_pop;
            if (vi < 0) {
                unfit = true;
                break;
            }
            if (tid == 0 && steps < A.step_cap) A.trace[(size_t)b * A.step_cap + steps] = sh_d2v[vi];
            ++steps;
            // ---- pos / neg / rest in list order (REF.py:106-108); rest heads the next list
            const uint32_t vb = 1u << vi;
            int np = 0, nn = 0, nr = 0;
            for (int base = 0; base < ncl; base += T) {
                const int c = base + tid;
                const bool have = c < ncl;
                const uint64_t k = have ? cur[c] : 0ull;
                const bool inP = have && ((uint32_t)k & vb), inN = have && ((uint32_t)(k >> 32) & vb);
                const bool inR = have && !inP && !inN;
                uint64_t tot;
                const uint64_t pre = dpb_scan3(inP, inN, inR, sh_w, par, &tot);
                if (inP) pos[np + (int)(pre & 0x1FFFFFu)] = k;
                if (inN) neg[nn + (int)((pre >> 21) & 0x1FFFFFu)] = k;
                if (inR) nxt[nr + (int)(pre >> 42)] = k;
                np += (int)(tot & 0x1FFFFFu);
                nn += (int)((tot >> 21) & 0x1FFFFFu);
                nr += (int)(tot >> 42);
            }
            __syncthreads();
            // ---- the resolvents, pair (i, j) = pair index i * nn + j (REF.py:111-119)
            const int npairs = np * nn;   // <= clause_cap^2 <= 2^22
            const int64_t trip = A.clause_limit <= 0 ? INT64_MAX : A.clause_limit - nr + 1 > 1 ? A.clause_limit - nr + 1 : 1;
            int64_t cnt = 0;              // non-tautological resolvents so far
            int nnext = nr;
            bool over = false;            // the next list outgrew clause_cap
            int event = 0;
            for (int cbase = 0; cbase < npairs; cbase += DPB_CHUNK) {
                // (A) keys, flags, events; candidates compacted in pair order
                int ncand = 0;
                for (int q = cbase; q < cbase + DPB_CHUNK && q < npairs; q += T) {
                    const int p = q + tid;
                    bool f = false;
                    uint64_t r = 0;
                    if (p < npairs && p < cbase + DPB_CHUNK) {
                        const int i = p / nn, j = p - i * nn;
                        const uint64_t a = pos[i], c = neg[j];
                        const uint32_t P = ((uint32_t)a & ~vb) | (uint32_t)c;
                        const uint32_t N = (uint32_t)(a >> 32) | ((uint32_t)(c >> 32) & ~vb);
                        if (!(P & N)) {
                            if (!(P | N)) atomicMin(&sh_evE, p);   // REF.py:117-118
                            else {
                                f = true;
                                r = (uint64_t)P | ((uint64_t)N << 32);
                            }
                        }
                    }
                    int tot;
                    const int pre = dpb_scan(f, sh_w, par, &tot);
                    if (f) {
                        if (cnt + pre + 1 == trip) atomicMin(&sh_evL, p);   // takes nr + count over clause_limit
                        if (!over) cand[ncand + pre] = r;
                    }
                    ncand += tot;
                    cnt += tot;
                }
                __syncthreads();
                const int evE = sh_evE, evL = sh_evL;
                if (evE != DPB_NOEVENT || evL != DPB_NOEVENT) {   // the first event in pair order
                    event = evL < evE ? -1 : 1;
                    break;
                }
                if (over) continue;
                // (B) against rest and what earlier chunks kept
                int nsurv = 0;
                for (int q = 0; q < ncand; q += T) {
                    const int x = q + tid;
                    const bool have = x < ncand;
                    const uint64_t r = have ? cand[x] : 0ull;
                    const bool keep = have && !dpb_subsumed(nxt, nnext, r, have);
                    int tot;
                    const int pre = dpb_scan(keep, sh_w, par, &tot);
                    if (keep) surv[nsurv + pre] = r;
                    nsurv += tot;
                }
                __syncthreads();
                // (C) against the earlier survivors of this chunk; the kept ones join the next list
                for (int q = 0; q < nsurv; q += T) {
                    const int y = q + tid;
                    const bool have = y < nsurv;
                    const uint64_t nr_ = have ? ~surv[y] : 0ull;
                    bool sub = false;
                    const int ymax = min(q + T, nsurv) - 1;   // the last lane's y: x < y for every lane
                    for (int x = 0; x < ymax; ++x) {
                        if (!__ballot(have && !sub && x < y)) break;
                        sub |= x < y && !(surv[x] & nr_);
                    }
                    const bool keep = have && !sub;
                    int tot;
                    const int pre = dpb_scan(keep, sh_w, par, &tot);
                    if (keep && nnext + pre < cap) nxt[nnext + pre] = ~nr_;
                    nnext += tot;
                }
                if (nnext > cap) {
                    over = true;
                    nnext = cap;
                }
                __syncthreads();
            }
            if (event) {
                result = event < 0 ? -1 : 0;
                break;
            }
            if (over) {
                unfit = true;
                break;
            }
            // ---- clauses = remaining_clauses + unique_new
            uint64_t *const t = cur;
            cur = nxt;
            nxt = t;
            ncl = nnext;
            if (steps - 1 < A.step_cap) {
                if (tid == 0) A.step_clauses[(size_t)b * A.step_cap + steps - 1] = ncl;
                if (A.keys_out) {
                    const int nw = rec_end - rec_at < ncl ? (int)(rec_end - rec_at) : ncl;
                    for (int c = tid; c < nw; c += T) A.keys_out[rec_at + c] = cur[c];
                    rec_at += nw;
                }
            }
        }
        if (tid == 0) {
            A.result[b] = unfit ? SATMI_DP_BATCH_UNFIT : result;
            A.steps[b] = unfit ? 0 : steps;
        }
    }
}

// ------------------------------------------------------------------ host side
namespace {

constexpr OomText DPB_OOM{"satmi_dp_batch_host", "split the batch (the record keeps every formula's clause lists)"};

// Capacity tiers: clauses per list and workgroup width.  The largest list of
// an elimination is not known before it ran, so the launch takes the smallest
// tier that holds d x m clauses for every formula of the batch with d <= 31
// variables and m clauses (3-SAT sets of 12 variables / 60 clauses reach 280,
// of 16 / 96 about 900), else the largest.  The chunk buffers need no tier:
// candidates and survivors are per chunk.  DESIGN.md "Batched Davis-Putnam" has
// the measurements behind the widths.
struct Tier {
    int clause_cap;
    int threads;       // workgroup width
    int threads_few;   // ... of a batch of no more formulas than CUs
};
constexpr Tier DPB_TIERS[] = {
    {512, 256, 512},    // 32 KiB
    {1024, 256, 1024},  // 48 KiB
    {1920, 512, 1024},  // 76 KiB: two workgroups on a CU
};
constexpr int DPB_NTIERS = (int)(sizeof(DPB_TIERS) / sizeof(DPB_TIERS[0]));
constexpr int DPB_CLAUSE_CAP_MAX = DPB_TIERS[DPB_NTIERS - 1].clause_cap;
constexpr size_t DPB_LDS_SLACK = 512;   // static LDS of a workgroup, rounded up

std::atomic<int> g_dbg_grid{0}, g_dbg_cap{0};   // satmi_dp_debug_batch

struct DpBatchWork : BatchWork {};   // a pool of its own

int fail_arg(const char *what) {
    set_error(std::string("satmi_dp_batch_host: ") + what);
    return SATMI_ERR_ARG;
}

}  // namespace

}  // namespace satmi

using namespace satmi;

extern "C" int satmi_dp_debug_batch(int grid, int clause_cap) {
    if (grid < 0 || clause_cap < 0 || clause_cap > DPB_CLAUSE_CAP_MAX) {
        set_error("satmi_dp_debug_batch: grid >= 0 and 0 <= clause_cap <= " + std::to_string(DPB_CLAUSE_CAP_MAX));
        return SATMI_ERR_ARG;
    }
    g_dbg_grid = grid;
    g_dbg_cap = clause_cap;
    return SATMI_OK;
}

extern "C" int satmi_dp_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                   const int32_t *h_clause_lit_begin, const int32_t *h_lits, int64_t step_limit,
                                   int64_t clause_limit, int32_t *h_result, int32_t *h_steps, int32_t *h_trace_vars,
                                   int64_t *h_step_clauses, int step_cap, int32_t *h_rec_lits, int64_t rec_lit_cap,
                                   int64_t *h_rec_clause_off, int64_t rec_clause_cap, int64_t *h_rec_step_off) {
    // ---- check: all of it before any HIP call
    const int nrec = (h_rec_lits != nullptr) + (h_rec_clause_off != nullptr) + (h_rec_step_off != nullptr);
    const bool record = nrec == 3;
    const char *own = nullptr;   // this entry point's own arguments, behind the count
    if (step_cap < 0) own = "step_cap < 0";
    else if (nrec != 0 && nrec != 3) own = "the record needs all of its pointers or none";
    else if (record && (rec_lit_cap < 0 || rec_clause_cap < 0)) own = "negative record capacity";
    if (const char *bad = batch_csr_check(num_instances, h_inst_clause_begin, h_clause_lit_begin, h_lits, own,
                                          h_result && h_steps && (step_cap <= 0 || (h_trace_vars && h_step_clauses))))
        return fail_arg(bad);
    if (num_instances == 0) return SATMI_OK;
    const int B = num_instances;

    // ---- encode; the tier: the smallest that holds d x m clauses for every formula that can fit
    BatchKeys K;
    batch_encode(B, h_inst_clause_begin, h_clause_lit_begin, h_lits, &K);
    int64_t need = 1;
    for (int b = 0; b < B; ++b)
        if (K.nvars[(size_t)b] <= DPB_MAXVARS)
            need = std::max<int64_t>(need, (int64_t)K.nvars[(size_t)b] * (h_inst_clause_begin[b + 1] - h_inst_clause_begin[b]));
    Tier tier = DPB_TIERS[DPB_NTIERS - 1];
    for (int t = DPB_NTIERS - 1; t >= 0; --t)
        if (need <= DPB_TIERS[t].clause_cap) tier = DPB_TIERS[t];
    const int dbg_cap = g_dbg_cap, dbg_grid = g_dbg_grid;
    if (dbg_cap > 0 && dbg_cap < tier.clause_cap) tier.clause_cap = dbg_cap;   // test knob: shorter lists, the tier's width
    const size_t lds_bytes = 8 * (4 * (((size_t)tier.clause_cap + 1) & ~(size_t)1) + 2 * (size_t)DPB_CHUNK);
    const int PC = std::min(step_cap, DPB_STEPS_MAX);   // rows the device keeps per formula
    const size_t PCa = (size_t)std::max(PC, 1);

    // ---- lease the workspace
    int dev = 0;
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts, &dev));
    Lease<DpBatchWork> lease{Pool<DpBatchWork>::get().acquire(dev)};
    if (!lease.w) {
        set_error("satmi_dp_batch_host: hipStreamCreate failed");
        return SATMI_ERR_HIP;
    }
    lease.ok = true;   // whatever the call's outcome (see BatchWork)
    DpBatchWork &wk = *lease.w;
    hipStream_t s = wk.stream;
    // ---- carve.  Inputs, one copy: clause ranges, variable counts, index -> id, keys
    Carve cu;
    const size_t u_icb = cu.take(4 * (size_t)(B + 1)), u_nv = cu.take(4 * (size_t)B);
    const size_t u_d2v = cu.take(4 * K.d2v.size()), u_keys = cu.take(8 * K.keys.size()), up_bytes = cu.at;
    // outputs, zeroed, one copy back: work word, results, steps, trace rows, clause-count rows
    Carve co;
    const size_t o_work = co.take(4), o_res = co.take(4 * (size_t)B), o_stp = co.take(4 * (size_t)B);
    const size_t o_trc = co.take(4 * (size_t)B * PCa), o_sc = co.take(8 * (size_t)B * PCa), out_bytes = co.at;
    SATMI_TRY(wk.up.reserve(up_bytes, &DPB_OOM));
    SATMI_TRY(wk.out.reserve(out_bytes, &DPB_OOM));
    SATMI_TRY(wk.up_h.grow(up_bytes));
    SATMI_TRY(wk.out_h.grow(out_bytes));
    std::memcpy(wk.up_h.p + u_icb, h_inst_clause_begin, 4 * (size_t)(B + 1));
    std::memcpy(wk.up_h.p + u_nv, K.nvars.data(), 4 * (size_t)B);
    std::memcpy(wk.up_h.p + u_d2v, K.d2v.data(), 4 * K.d2v.size());
    std::memcpy(wk.up_h.p + u_keys, K.keys.data(), 8 * K.keys.size());
    SATMI_HIP(hipMemcpyAsync(wk.up.p, wk.up_h.p, up_bytes, hipMemcpyHostToDevice, s));

    unsigned char *up = wk.up.as<unsigned char>(), *out = wk.out.as<unsigned char>();
    DpBatchArgs A;
    A.icb = (const int32_t *)(up + u_icb);
    A.nvars = (const int32_t *)(up + u_nv);
    A.d2v = (const int32_t *)(up + u_d2v);
    A.keys_in = (const uint64_t *)(up + u_keys);
    A.num_instances = B;
    A.clause_cap = tier.clause_cap;
    A.step_limit = step_limit;
    A.clause_limit = clause_limit;
    A.result = (int32_t *)(out + o_res);
    A.steps = (int32_t *)(out + o_stp);
    A.trace = (int32_t *)(out + o_trc);
    A.step_clauses = (int64_t *)(out + o_sc);
    A.step_cap = PC;
    A.keys_out = nullptr;
    A.rec_off = nullptr;
    A.work = (uint32_t *)(out + o_work);

    // ---- launch: one persistent grid, a second time when the record is kept
    int threads = B <= facts.cus ? tier.threads_few : tier.threads;
    if (const char *e = std::getenv("SATMI_DP_BATCH_WIDTH")) {   // measurement knob (tools/dp_batch_time.py --sweep)
        const int w = std::atoi(e);
        if (w >= 64 && w <= 1024 && w % 64 == 0) threads = w;
    }
    const int grid = batch_grid(facts, lds_bytes, DPB_LDS_SLACK, threads, B, dbg_grid);
    SATMI_TRY(batch_allow_lds((const void *)dp_batch_kernel, lds_bytes));
    const auto launch = [&]() -> int {
        SATMI_HIP(hipMemsetAsync(wk.out.p, 0, out_bytes, s));
        hipLaunchKernelGGL(dp_batch_kernel, dim3(grid), dim3(threads), lds_bytes, s, A);
        SATMI_HIP(hipGetLastError());
        SATMI_HIP(hipMemcpyAsync(wk.out_h.p, wk.out.p, out_bytes, hipMemcpyDeviceToHost, s));
        SATMI_HIP(hipStreamSynchronize(s));
        return SATMI_OK;
    };
    SATMI_TRY(launch());

    const unsigned char *oh = wk.out_h.p;
    const int32_t *r_res = (const int32_t *)(oh + o_res), *r_stp = (const int32_t *)(oh + o_stp);
    const int32_t *r_trc = (const int32_t *)(oh + o_trc);
    const int64_t *r_sc = (const int64_t *)(oh + o_sc);

    // ---- the record: the elimination is deterministic, so the lists' sizes of
    // the first launch place every formula's keys for a second one that keeps
    // them (as many as the caller's clause offsets can hold)
    std::vector<uint64_t> hk;
    std::vector<int64_t> roff;
    if (record) {
        roff.assign((size_t)B + 1, 0);
        const int64_t room = std::max<int64_t>(rec_clause_cap - 1, 0);
        for (int b = 0; b < B; ++b) {
            int64_t n = 0;
            if (r_res[b] != SATMI_DP_BATCH_UNFIT)
                for (int k = 0; k < std::min(r_stp[b], PC); ++k) n += r_sc[(size_t)b * PCa + k];
            roff[(size_t)b + 1] = std::min(roff[(size_t)b] + n, room);
        }
        const int64_t nkeys = roff[(size_t)B];
        if (nkeys > 0) {
            SATMI_TRY(wk.keys_out.reserve(8 * (size_t)nkeys, &DPB_OOM));
            SATMI_TRY(wk.rec_off.reserve(8 * ((size_t)B + 1), &DPB_OOM));
            SATMI_HIP(hipMemcpyAsync(wk.rec_off.p, roff.data(), 8 * ((size_t)B + 1), hipMemcpyHostToDevice, s));
            A.keys_out = wk.keys_out.as<uint64_t>();
            A.rec_off = wk.rec_off.as<int64_t>();
            SATMI_TRY(launch());
            hk.resize((size_t)nkeys);
            SATMI_HIP(hipMemcpyAsync(hk.data(), wk.keys_out.p, 8 * (size_t)nkeys, hipMemcpyDeviceToHost, s));
            SATMI_HIP(hipStreamSynchronize(s));
            wk.drop_large_record();
        }
    }

    // ---- copy back
    for (int b = 0; b < B; ++b) {
        const bool unfit = r_res[b] == SATMI_DP_BATCH_UNFIT;
        h_result[b] = r_res[b];
        h_steps[b] = unfit ? 0 : r_stp[b];
        if (step_cap > 0) {
            int32_t *trow = h_trace_vars + (size_t)b * (size_t)step_cap;
            int64_t *crow = h_step_clauses + (size_t)b * (size_t)step_cap;
            std::memset(trow, 0, 4 * (size_t)step_cap);
            std::memset(crow, 0, 8 * (size_t)step_cap);
            if (!unfit) {   // (a formula that turned out UNFIT in a later step leaves no rows)
                const int n = std::min(PC, r_stp[b]);
                std::memcpy(trow, r_trc + (size_t)b * PCa, 4 * (size_t)n);
                std::memcpy(crow, r_sc + (size_t)b * PCa, 8 * (size_t)n);
            }
        }
    }
    if (!record) return SATMI_OK;

    // ---- decode the record: formula after formula, the list after every
    // completed step, clauses in list order, literals ascending by variable id
    // (+v before -v), with satmi_dp_host's truncation: a clause needs a free
    // clause offset, a literal past rec_lit_cap is dropped
    int64_t rec_clauses = 0, rec_lits = 0;
    if (rec_clause_cap > 0) h_rec_clause_off[0] = 0;
    for (int b = 0; b < B; ++b) {
        int64_t *srow = h_rec_step_off + (size_t)b * ((size_t)step_cap + 1);
        srow[0] = rec_clauses;
        const bool unfit = r_res[b] == SATMI_DP_BATCH_UNFIT;
        const int ns = unfit ? 0 : std::min(r_stp[b], PC);
        const int32_t *dv = K.d2v.data() + (size_t)b * BATCH_D2V_STRIDE;
        const int V = std::min(K.nvars[(size_t)b], BATCH_D2V_STRIDE);
        int64_t at = roff[(size_t)b];
        const int64_t end = roff[(size_t)b + 1];
        for (int k = 0; k < ns; ++k) {
            // (the step that ended the elimination completed no list: its count is 0)
            const int64_t n = r_sc[(size_t)b * PCa + k];
            for (int64_t c = 0; c < n && at < end && rec_clauses + 1 < rec_clause_cap; ++c, ++at) {
                int32_t cl[64];
                const int64_t nl = std::min<int64_t>(batch_decode(hk[(size_t)at], dv, V, cl), rec_lit_cap - rec_lits);
                std::copy(cl, cl + nl, h_rec_lits + rec_lits);
                rec_lits += nl;
                h_rec_clause_off[++rec_clauses] = rec_lits;
            }
            srow[k + 1] = rec_clauses;
        }
        for (int k = ns; k < step_cap; ++k) srow[k + 1] = rec_clauses;
    }
    return SATMI_OK;
}
