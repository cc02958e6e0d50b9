// resolution_batch.hip -- resolution saturation (REF.py:63-95) of a batch of
// small clause sets in one launch on gfx950: one workgroup per formula, the
// whole saturation in LDS.
//
// satmi_resolution_host (resolution.hip) saturates one clause set per call and
// is bound by the call itself for small sets (an upload, a graph replay, a
// flag spin).  With at most 31 distinct variables a clause is one 64-bit key
// P | N << 32 over the formula's dense variable index (the packed path's key),
// and a formula of d variables and m input clauses never holds more than
// 3^d + m keys, so its clause list and its `seen` set fit in LDS:
//
//   * a persistent grid of workgroups draws formula indices from an atomic
//     work counter (as the DPLL / CDCL kernels do);
//   * LDS per workgroup: the key list in append order (key_cap keys), an
//     open-addressing table of every key seen (a power of two of slots, more
//     than key_cap: RB_TIERS; seeded with the input clauses, REF.py:65), an
//     append counter and a stop word;
//   * a pass is semi-naive like the packed path: pairs (i < j) with j among the
//     clauses the previous pass added (all pairs in pass 1); a wave takes a
//     clause j (its key a broadcast read), its lanes the clauses i;
//   * a resolvent that claims its table slot (64-bit LDS compare-and-swap: the
//     key was absent) is appended behind the list, with one counter atomic per
//     wave step (ballot + popcount);
//   * a workgroup barrier ends the pass; the verdicts are taken after it;
//   * a formula that outgrows key_cap (or has more than 31 variables) gets
//     SATMI_RES_BATCH_UNFIT and the workgroup goes on: appends past key_cap are
//     counted, never stored, and a probe run is bounded by the table size.
//
// The host checks the batch, builds the dense index and the keys (a batch of
// 4,096 formulas is ~600 k literals), uploads them in one copy, and decodes the
// optional record from the keys the kernel leaves in HBM; that host side is
// shared with dp_batch.hip (batch_keys.h, batch_host.h).
//
// The kernel's pair classification restates res_pass_packed_kernel's
// (resolution.hip): device code is not shared, so that kernel's machine code,
// which the bench's issue rooflines are keyed by, stays what it is.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <vector>

#include "batch_host.h"
#include "common.h"

namespace satmi {

constexpr uint64_t RB_EMPTY = ~0ull;   // bit 31 of P and N is never set: no key equals it
constexpr int RB_STOP_EMPTY = 1, RB_STOP_FULL = 2;

struct ResBatchArgs {
    const int32_t *icb;       // [B + 1] clause range of each formula
    const uint64_t *keys_in;  // [C] the input clauses' keys (host-encoded)
    const int32_t *nvars;     // [B] distinct variables of each formula
    int num_instances;
    int key_cap;              // keys a formula may hold (the LDS key list)
    uint32_t tslots;          // table slots, a power of two > key_cap
    int64_t max_passes, clause_limit;
    int32_t *result, *passes;
    int64_t *pass_new;        // [B x pass_cap], zeroed before the launch
    int pass_cap;
    uint64_t *keys_out;       // record: every formula's new keys, packed by `cursor`; or null
    unsigned long long *key_off;   // [B] where formula b's new keys start in keys_out
    unsigned long long *cursor;    // keys_out's append cursor
    uint32_t *work;           // the work counter
};

__device__ __forceinline__ uint64_t rb_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Claim key r in the LDS table (linear probing; a key sits before the first
// empty slot of its sequence, and a slot only ever changes from RB_EMPTY to a
// key).  1 = r was absent and this call inserted it, 0 = present, -1 = every
// slot probed (the table is full: the formula does not fit).
__device__ __forceinline__ int rb_claim(uint64_t *table, uint32_t mask, uint64_t r) {
    uint32_t s = (uint32_t)rb_mix(r) & mask;
    for (uint32_t n = 0; n <= mask; ++n) {
        uint64_t cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == RB_EMPTY) {
            cur = atomicCAS((unsigned long long *)(table + s), (unsigned long long)RB_EMPTY, (unsigned long long)r);
            if (cur == RB_EMPTY) return 1;
        }
        if (cur == r) return 0;
        s = (s + 1) & mask;
    }
    return -1;
}

__global__ void __launch_bounds__(1024) res_batch_kernel(ResBatchArgs A) {
    extern __shared__ uint64_t rb_lds[];   // keys[key_cap], table[tslots]
    __shared__ int sh_b, sh_app, sh_stop;
    __shared__ unsigned long long sh_out;
    uint64_t *keys = rb_lds, *table = rb_lds + A.key_cap;
    const int tid = threadIdx.x, T = blockDim.x, ln = lane_id(), wv = tid >> 6, nwv = T >> 6;
    const uint32_t mask = A.tslots - 1u;
    for (;;) {
        if (tid == 0) sh_b = (int)atomicAdd(A.work, 1u);
        __syncthreads();
        const int b = sh_b;
        if (b >= A.num_instances) break;   // workgroup-uniform
        const int c0 = A.icb[b], m = A.icb[b + 1] - c0;
        if (A.nvars[b] > 31 || m > A.key_cap) {
            if (tid == 0) {
                A.result[b] = SATMI_RES_BATCH_UNFIT;
                A.passes[b] = 0;
            }
            __syncthreads();   // sh_b is rewritten by the next draw
            continue;
        }
        // everything the next formula reads starts clean: table, counter, stop word
        for (uint32_t t = tid; t < A.tslots; t += T) table[t] = RB_EMPTY;
        if (tid == 0) {
            sh_app = m;
            sh_stop = 0;
        }
        __syncthreads();
        // the input clauses: the list keeps duplicates, `seen` does not (REF.py:64-65)
        for (int c = tid; c < m; c += T) {
            const uint64_t k = A.keys_in[c0 + c];
            keys[c] = k;
            (void)rb_claim(table, mask, k);   // m <= key_cap < tslots: never full
        }
        __syncthreads();
        int jlo = 0, ncl = m, passes = 0, result = -1;
        for (;;) {
            for (int j = jlo + wv; j < ncl; j += nwv) {
                if (uniform_i32(__hip_atomic_load(&sh_stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) break;
                const uint64_t kb = keys[j];
                const uint32_t Pb = (uint32_t)kb, Nb = (uint32_t)(kb >> 32);
                for (int i0 = 0; i0 < j; i0 += 64) {
                    const int i = i0 + ln;
                    bool win = false;
                    uint64_t r = 0;
                    if (i < j) {
                        const uint64_t ka = keys[i];
                        const uint32_t Pa = (uint32_t)ka, Na = (uint32_t)(ka >> 32);
                        const uint32_t clash = (Pa & Nb) | (Na & Pb);
                        // exactly one clashing variable: the resolvent (two or more
                        // make every resolvent a tautology, REF.py:81)
                        if (clash && !(clash & (clash - 1))) {
                            const uint32_t P = (Pa | Pb) & ~clash, N = (Na | Nb) & ~clash;
                            if (!(P & N)) {
                                if (!(P | N)) {
                                    atomicOr(&sh_stop, RB_STOP_EMPTY);   // REF.py:84-85
                                } else {
                                    r = (uint64_t)P | ((uint64_t)N << 32);
                                    const int c = rb_claim(table, mask, r);
                                    win = c > 0;
                                    if (c < 0) atomicOr(&sh_stop, RB_STOP_FULL);
                                }
                            }
                        }
                    }
                    const uint64_t mk = __ballot(win);
                    if (mk) {   // clauses.extend(new): one counter atomic per wave step
                        int pos = 0;
                        if (ln == 0) pos = atomicAdd(&sh_app, __popcll(mk));
                        pos = __shfl(pos, 0) + __popcll(mk & lanemask_lt());
                        if (win) {
                            if (pos < A.key_cap)
                                keys[pos] = r;   // behind ncl: no wave reads it in this pass
                            else                 // counted, not stored
                                atomicOr(&sh_stop, RB_STOP_FULL);
                        }
                    }
                }
            }
            __syncthreads();   // the pass is over: every append and flag is in LDS
            const int stop = sh_stop, app = sh_app;
            __syncthreads();   // ... and read by all before the next pass appends again
            if (stop & RB_STOP_EMPTY) {   // an empty resolvent of clauses that are all there: False
                result = 0;
                break;
            }
            if ((stop & RB_STOP_FULL) || app > A.key_cap) {
                result = SATMI_RES_BATCH_UNFIT;
                break;
            }
            const int nnew = app - ncl;
            if (nnew == 0) {   // no new clauses can be derived (REF.py:91-92)
                result = 1;
                break;
            }
            if (tid == 0 && passes < A.pass_cap) A.pass_new[(int64_t)b * A.pass_cap + passes] = nnew;
            ++passes;
            jlo = ncl;
            ncl = app;
            if ((A.max_passes > 0 && passes >= A.max_passes) || (A.clause_limit > 0 && ncl > A.clause_limit))
                break;   // result stays -1
        }
        if (A.keys_out && result != SATMI_RES_BATCH_UNFIT && ncl > m) {   // workgroup-uniform
            if (tid == 0) sh_out = atomicAdd(A.cursor, (unsigned long long)(ncl - m));
            __syncthreads();
            const unsigned long long base = sh_out;   // the sum over b of ncl - m is <= B x key_cap
            for (int t = tid; t < ncl - m; t += T) A.keys_out[base + t] = keys[m + t];
            if (tid == 0) A.key_off[b] = base;
        }
        if (tid == 0) {
            A.result[b] = result;
            A.passes[b] = result == SATMI_RES_BATCH_UNFIT ? 0 : passes;
        }
        __syncthreads();   // the next formula rewrites sh_b, the keys and the table
    }
}

// ------------------------------------------------------------------ host side
namespace {

constexpr OomText RB_OOM{"satmi_resolution_batch_host", "split the batch (the record keeps every formula's keys)"};

// Capacity tiers: keys per formula, table slots, workgroup width.  The launch
// takes the smallest tier that holds 3^d + m keys for every formula of the
// batch with d <= 31 variables (no such formula can then overflow), else the
// largest; DESIGN.md "Kernel 3" has the measurements behind the widths.
struct Tier {
    int key_cap;
    uint32_t tslots;
    int threads;       // workgroup width
    int threads_few;   // ... of a batch of no more formulas than CUs
};
// (the widths, measured at 64/128/256/256, 128/256/512/512 and 256/512/1024/1024
// with `make variant VFLAGS=-DSATMI_RB_WIDTH_...`: profiles/res_batch/)
#ifndef SATMI_RB_WIDTH_S
#define SATMI_RB_WIDTH_S 64
#endif
#ifndef SATMI_RB_WIDTH_M
#define SATMI_RB_WIDTH_M 512
#endif
#ifndef SATMI_RB_WIDTH_L
#define SATMI_RB_WIDTH_L 512
#endif
#ifndef SATMI_RB_WIDTH_XL
#define SATMI_RB_WIDTH_XL 1024
#endif
// A batch of no more formulas than CUs: each formula has a CU to itself, and
// the widest workgroup (the most waves to hide the LDS probes behind) is the
// fastest; with more formulas the 2,560-key tier keeps 3 workgroups of 512 on a
// CU where 1,024 threads leave room for 2.
constexpr int RB_WIDTH_L_FEW = 1024;
constexpr Tier RB_TIERS[] = {
    {256, 512, SATMI_RB_WIDTH_S, SATMI_RB_WIDTH_S},      //  6 KiB: d <= 4
    {1024, 2048, SATMI_RB_WIDTH_M, SATMI_RB_WIDTH_M},    // 24 KiB: d <= 6
    {2560, 4096, SATMI_RB_WIDTH_L, RB_WIDTH_L_FEW},      // 52 KiB: d = 7 with up to 373 input clauses
    {4096, 8192, SATMI_RB_WIDTH_XL, SATMI_RB_WIDTH_XL},  // 96 KiB
};
constexpr int RB_NTIERS = (int)(sizeof(RB_TIERS) / sizeof(RB_TIERS[0]));
constexpr int RB_KEY_CAP_MAX = RB_TIERS[RB_NTIERS - 1].key_cap;
constexpr size_t RB_LDS_SLACK = 64;   // static LDS of a workgroup, rounded up

std::atomic<int> g_dbg_grid{0}, g_dbg_key_cap{0};   // satmi_resolution_debug_batch

struct ResBatchWork : BatchWork {};   // a pool of its own (rec_off stays empty)

int fail_arg(const char *what) {
    set_error(std::string("satmi_resolution_batch_host: ") + what);
    return SATMI_ERR_ARG;
}

}  // namespace

}  // namespace satmi

using namespace satmi;

extern "C" int satmi_resolution_debug_batch(int grid, int key_cap) {
    if (grid < 0 || key_cap < 0 || key_cap > RB_KEY_CAP_MAX) {
        set_error("satmi_resolution_debug_batch: grid >= 0 and 0 <= key_cap <= " + std::to_string(RB_KEY_CAP_MAX));
        return SATMI_ERR_ARG;
    }
    g_dbg_grid = grid;
    g_dbg_key_cap = key_cap;
    return SATMI_OK;
}

extern "C" int satmi_resolution_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                           const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                           int64_t max_passes, int64_t clause_limit, int32_t *h_result,
                                           int32_t *h_passes, int64_t *h_pass_new, int pass_cap, int32_t *h_rec_lits,
                                           int64_t rec_lit_cap, int64_t *h_rec_clause_off, int64_t rec_clause_cap,
                                           int64_t *h_rec_pass_off) {
    // ---- check: all of it before any HIP call
    if (const char *bad = batch_csr_check(num_instances, h_inst_clause_begin, h_clause_lit_begin, h_lits,
                                          pass_cap < 0 ? "pass_cap < 0" : nullptr,
                                          h_result && h_passes && (pass_cap <= 0 || h_pass_new)))
        return fail_arg(bad);
    if (num_instances == 0) return SATMI_OK;
    const int B = num_instances;
    const bool record = h_rec_lits && h_rec_clause_off && h_rec_pass_off;   // (a partial set: no record)

    // ---- encode; the tier: the smallest that holds 3^d + m keys for every formula that can fit
    BatchKeys K;
    batch_encode(B, h_inst_clause_begin, h_clause_lit_begin, h_lits, &K);
    int64_t need = 1;
    for (int b = 0; b < B; ++b) {
        const int d = K.nvars[(size_t)b];
        if (d > BATCH_MAXVARS) continue;
        int64_t p3 = 1;
        for (int k = 0; k < d && p3 <= RB_KEY_CAP_MAX; ++k) p3 *= 3;
        need = std::max<int64_t>(need, p3 + (h_inst_clause_begin[b + 1] - h_inst_clause_begin[b]));
    }
    Tier tier = RB_TIERS[RB_NTIERS - 1];
    for (int t = RB_NTIERS - 1; t >= 0; --t)
        if (need <= RB_TIERS[t].key_cap) tier = RB_TIERS[t];
    const int dbg_cap = g_dbg_key_cap, dbg_grid = g_dbg_grid;
    if (dbg_cap > 0 && dbg_cap < tier.key_cap) {   // test knob: fewer keys, the tier's width
        tier.key_cap = dbg_cap;
        tier.tslots = 64;
        while (tier.tslots < 2u * (uint32_t)dbg_cap) tier.tslots <<= 1;
    }
    const size_t lds_bytes = 8 * ((size_t)tier.key_cap + tier.tslots);
    // passes that add clauses <= keys: the device keeps min(pass_cap, key_cap) counts per formula
    const int PC = std::min(pass_cap, tier.key_cap);

    // ---- lease the workspace
    int dev = 0;
    DeviceFacts facts;
    SATMI_TRY(device_facts(&facts, &dev));
    Lease<ResBatchWork> lease{Pool<ResBatchWork>::get().acquire(dev)};
    if (!lease.w) {
        set_error("satmi_resolution_batch_host: hipStreamCreate failed");
        return SATMI_ERR_HIP;
    }
    lease.ok = true;   // whatever the call's outcome (see BatchWork)
    ResBatchWork &wk = *lease.w;
    hipStream_t s = wk.stream;
    // ---- carve.  Inputs, one copy: clause ranges, variable counts, keys
    Carve cu;
    const size_t u_icb = cu.take(4 * (size_t)(B + 1)), u_nv = cu.take(4 * (size_t)B);
    const size_t u_keys = cu.take(8 * K.keys.size()), up_bytes = cu.at;
    // outputs, zeroed, one copy back: work word (0) and key cursor (8), results, passes, key offsets, per-pass counts
    Carve co;
    const size_t o_work = co.take(16), o_res = co.take(4 * (size_t)B), o_pas = co.take(4 * (size_t)B);
    const size_t o_off = co.take(8 * (size_t)B), o_pn = co.take(8 * (size_t)B * (size_t)std::max(PC, 1));
    const size_t out_bytes = co.at;
    SATMI_TRY(wk.up.reserve(up_bytes, &RB_OOM));
    SATMI_TRY(wk.out.reserve(out_bytes, &RB_OOM));
    SATMI_TRY(wk.up_h.grow(up_bytes));
    SATMI_TRY(wk.out_h.grow(out_bytes));
    if (record) SATMI_TRY(wk.keys_out.reserve(8 * (size_t)B * (size_t)tier.key_cap, &RB_OOM));
    std::memcpy(wk.up_h.p + u_icb, h_inst_clause_begin, 4 * (size_t)(B + 1));
    std::memcpy(wk.up_h.p + u_nv, K.nvars.data(), 4 * (size_t)B);
    std::memcpy(wk.up_h.p + u_keys, K.keys.data(), 8 * K.keys.size());
    SATMI_HIP(hipMemcpyAsync(wk.up.p, wk.up_h.p, up_bytes, hipMemcpyHostToDevice, s));
    SATMI_HIP(hipMemsetAsync(wk.out.p, 0, out_bytes, s));

    unsigned char *up = wk.up.as<unsigned char>(), *out = wk.out.as<unsigned char>();
    ResBatchArgs A;
    A.icb = (const int32_t *)(up + u_icb);
    A.nvars = (const int32_t *)(up + u_nv);
    A.keys_in = (const uint64_t *)(up + u_keys);
    A.num_instances = B;
    A.key_cap = tier.key_cap;
    A.tslots = tier.tslots;
    A.max_passes = max_passes;
    A.clause_limit = clause_limit;
    A.result = (int32_t *)(out + o_res);
    A.passes = (int32_t *)(out + o_pas);
    A.pass_new = (int64_t *)(out + o_pn);
    A.pass_cap = PC;
    A.keys_out = record ? wk.keys_out.as<uint64_t>() : nullptr;
    A.key_off = (unsigned long long *)(out + o_off);
    A.cursor = (unsigned long long *)(out + o_work + 8);
    A.work = (uint32_t *)(out + o_work);

    // ---- launch: one persistent grid
    if (B <= facts.cus) tier.threads = tier.threads_few;
    const int grid = batch_grid(facts, lds_bytes, RB_LDS_SLACK, tier.threads, B, dbg_grid);
    SATMI_TRY(batch_allow_lds((const void *)res_batch_kernel, lds_bytes));
    hipLaunchKernelGGL(res_batch_kernel, dim3(grid), dim3(tier.threads), lds_bytes, s, A);
    SATMI_HIP(hipGetLastError());
    SATMI_HIP(hipMemcpyAsync(wk.out_h.p, wk.out.p, out_bytes, hipMemcpyDeviceToHost, s));
    SATMI_HIP(hipStreamSynchronize(s));

    // ---- copy back
    const unsigned char *oh = wk.out_h.p;
    const int32_t *r_res = (const int32_t *)(oh + o_res), *r_pas = (const int32_t *)(oh + o_pas);
    const unsigned long long *r_off = (const unsigned long long *)(oh + o_off);
    const int64_t *r_pn = (const int64_t *)(oh + o_pn);
    for (int b = 0; b < B; ++b) {
        const bool unfit = r_res[b] == SATMI_RES_BATCH_UNFIT;
        h_result[b] = r_res[b];
        h_passes[b] = unfit ? 0 : r_pas[b];
        if (pass_cap > 0) {
            int64_t *row = h_pass_new + (size_t)b * (size_t)pass_cap;
            std::memset(row, 0, 8 * (size_t)pass_cap);
            // (a formula that outgrew its capacity in a later pass leaves no counts)
            if (!unfit) std::memcpy(row, r_pn + (size_t)b * (size_t)PC, 8 * (size_t)std::min(PC, r_pas[b]));
        }
    }
    if (!record) return SATMI_OK;

    // ---- decode the record: each formula's passes from its keys, formula
    // after formula, in satmi_resolution_host's format and with its truncation
    const unsigned long long nkeys = *(const unsigned long long *)(oh + o_work + 8);
    std::vector<uint64_t> hk((size_t)nkeys);
    if (nkeys) {
        SATMI_HIP(hipMemcpyAsync(hk.data(), wk.keys_out.p, 8 * (size_t)nkeys, hipMemcpyDeviceToHost, s));
        SATMI_HIP(hipStreamSynchronize(s));
    }
    wk.drop_large_record();   // (B x key_cap keys of room)
    int64_t rec_clauses = 0, rec_lits = 0;
    if (rec_clause_cap > 0) h_rec_clause_off[0] = 0;
    std::vector<std::vector<int32_t>> pass;
    for (int b = 0; b < B; ++b) {
        int64_t *prow = h_rec_pass_off + (size_t)b * ((size_t)pass_cap + 1);
        prow[0] = rec_clauses;
        const int np = r_res[b] == SATMI_RES_BATCH_UNFIT ? 0 : std::min(r_pas[b], PC);
        const int32_t *dv = K.d2v.data() + (size_t)b * BATCH_D2V_STRIDE;
        const int V = std::min(K.nvars[(size_t)b], BATCH_D2V_STRIDE);
        const uint64_t *k = hk.data() + (np > 0 ? r_off[b] : 0ull);
        for (int p = 0; p < np; ++p) {
            const int64_t nnew = r_pn[(size_t)b * (size_t)PC + p];
            // each clause as ascending literals, the clauses in ascending order
            pass.resize((size_t)nnew);
            for (int64_t c = 0; c < nnew; ++c) {
                int32_t cl[64];
                const int n = batch_decode(k[c], dv, V, cl);
                std::sort(cl, cl + n);
                pass[(size_t)c].assign(cl, cl + n);
            }
            k += nnew;
            std::sort(pass.begin(), pass.end());
            for (const auto &cl : pass) {
                if (rec_clauses + 1 >= rec_clause_cap || rec_lits + (int64_t)cl.size() > rec_lit_cap) break;
                std::copy(cl.begin(), cl.end(), h_rec_lits + rec_lits);
                rec_lits += (int64_t)cl.size();
                h_rec_clause_off[++rec_clauses] = rec_lits;
            }
            prow[p + 1] = rec_clauses;
        }
        for (int p = np; p < pass_cap; ++p) prow[p + 1] = rec_clauses;
    }
    return SATMI_OK;
}
