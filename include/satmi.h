/*
 * satmi.h -- C ABI of the MI355X-native clause-set solving path.
 *
 * The reference (andreistana05/SAT-MPI-Stana-Andrei) is one Python script,
 * "comparatie intre algoritmii de rezolvare a seturilor de clauze.py" (REF.py).
 * Its solver entry points are plain Python functions over `List[List[int]]`
 * (REF.py:11-14); the drop-in mirror of those functions lives in
 * sat-mpi-stana-andrei_amd/satmi/solvers.py and calls the entry points below
 * through ctypes (INTEGRATION.md shows the binding).  All pointers are plain
 * C pointers; "d_" pointers are HIP device pointers, "h_" pointers host memory.
 * Every function returns SATMI_OK (0) or a negative error; satmi_last_error()
 * describes the last failure of the calling thread.
 *
 * Formula layout (CSR, the "flat literal/offset arrays in HBM" of the design):
 *   instance b owns clauses  [inst_clause_begin[b], inst_clause_begin[b+1])
 *   clause   c owns literals [clause_lit_begin[c],  clause_lit_begin[c+1])
 *   literals are DIMACS ints (v or -v, v >= 1), exactly the ints of REF.py's
 *   Clause = List[int]; inst_nvars[b] = largest variable index of instance b.
 */
#ifndef SATMI_H
#define SATMI_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SATMI_ABI_VERSION 2

/* return codes */
#define SATMI_OK 0
#define SATMI_ERR_ARG (-1)
#define SATMI_ERR_HIP (-2)
#define SATMI_ERR_TOO_LARGE (-3)
#define SATMI_ERR_NOMEM (-4)

/* per-instance DPLL status (d_status[b]) */
#define SATMI_DPLL_EXHAUSTED 0      /* search tree fully explored                 */
#define SATMI_DPLL_STOPPED 1        /* stopped after max_solutions solutions      */
#define SATMI_DPLL_NODE_LIMIT 2     /* node_limit calls reached                   */
#define SATMI_DPLL_TIMEOUT 3        /* time_limit_s reached (REF.py:17, :417-437)  */
#define SATMI_DPLL_TOO_LARGE 4      /* instance exceeds the launch's LDS layout   */

/* DPLL modes */
#define SATMI_MODE_REF 0    /* dpll_optimized exactly as REF.py:133-214             */
#define SATMI_MODE_SOUND 1  /* same procedure, decisions applied as unit clauses   */

/* counters per instance, d_counters[b*SATMI_NCOUNTERS + k] */
#define SATMI_NCOUNTERS 8
#define SATMI_CTR_NODES 0        /* dpll_optimized calls                         */
#define SATMI_CTR_DECISIONS 1    /* branch assignments (REF.py:212)              */
#define SATMI_CTR_UNIT_PROPS 2   /* unit-propagation assignments (REF.py:154)    */
#define SATMI_CTR_PURE 3         /* pure-literal assignments (REF.py:189)        */
#define SATMI_CTR_CONFLICTS 4    /* unit_propagate returned None (REF.py:168)    */
#define SATMI_CTR_SOLUTIONS 5    /* solutions found (len of REF.py's result)     */
#define SATMI_CTR_ROUNDS 6       /* unit-propagation rounds (clause scans)       */
#define SATMI_CTR_TICKS 7        /* wall-clock ticks the wave spent on the instance (100 MHz s_memrealtime) */

int satmi_abi_version(void);
const char *satmi_last_error(void);
int satmi_device_count(int *count);
int satmi_set_device(int device);
int satmi_synchronize(void);

/* Device memory helpers, so a host program needs no other HIP binding. */
int satmi_malloc(void **d_ptr, uint64_t bytes);
int satmi_free(void *d_ptr);
int satmi_memcpy_h2d(void *d_dst, const void *h_src, uint64_t bytes, void *stream);
int satmi_memcpy_d2h(void *h_dst, const void *d_src, uint64_t bytes, void *stream);
int satmi_stream_synchronize(void *stream);

/*
 * Batched DPLL: one wavefront per instance.  Replaces dpll_optimized
 * (REF.py:133-214) for a batch of formulas.
 *   mode           SATMI_MODE_REF | SATMI_MODE_SOUND
 *   max_solutions  stop after this many solutions (0 = enumerate all, as REF.py)
 *   node_limit     stop after this many dpll calls (0 = none)
 *   time_limit_s   per-instance wall-clock limit (<= 0 = none)
 *   max_vars/max_clauses/max_lits   maxima over the batch (size the LDS layout)
 *   max_clause_len longest clause of the batch; a value of 1..5 also promises
 *                  that every clause is non-empty; 0 = unknown.  SOUND mode
 *                  without a caller assignment and 1 <= max_clause_len <= 5,
 *                  max_vars <= 2047 runs the clause-scan kernel (same results;
 *                  see satmi_dpll_set_kernel); an instance that breaks the
 *                  promise gets SATMI_DPLL_TOO_LARGE.  A value above 255 takes
 *                  the general kernel's wide form (SATMI_KERNEL_WIDE), since
 *                  the LDS form holds clauses of at most 255 literals.  A
 *                  caller that passes 0 is planned by max_vars/max_clauses/
 *                  max_lits alone: where those fit the LDS layout, an instance
 *                  with a longer clause gets SATMI_DPLL_TOO_LARGE, as it does
 *                  under a pinned SATMI_KERNEL_GENERAL.
 *                  satmi_dpll_batch_host passes the true maximum whenever it
 *                  is above 5 or no clause is empty, else 0.
 *   d_init_begin/d_init_lits        optional caller assignment (REF.py:133's
 *                  `assignment`), as signed literals in dict order; may be NULL
 *   sol_cap        solutions stored per instance; sol_stride >= max assignment size
 *   outputs: d_status[B], d_counters[B*8], d_sol_len[B*sol_cap],
 *            d_sol_lits[B*sol_cap*sol_stride] (signed literals in the
 *            assignment dict's insertion order), d_root_len[B],
 *            d_root_lits[B*sol_stride] (the caller's dict after the root's
 *            unit_propagate, REF.py:167, which mutates it in place)
 *   stream         hipStream_t (NULL = default stream); the call is asynchronous
 */
int satmi_dpll_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                            const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                            const int32_t *d_inst_nvars, int max_vars, int max_clauses, int max_lits,
                            int max_clause_len, const int32_t *d_init_begin, const int32_t *d_init_lits,
                            int mode, int64_t max_solutions, int64_t node_limit, double time_limit_s,
                            int sol_cap, int sol_stride,
                            int32_t *d_status, int64_t *d_counters, int32_t *d_sol_len,
                            int32_t *d_sol_lits, int32_t *d_root_len, int32_t *d_root_lits,
                            void *stream);

/* Same, from host arrays (allocates, copies, runs, copies back; synchronous).
 * The arrays are checked first -- the count, the input pointers, both range
 * arrays ascending from >= 0, no literal 0 / INT32_MIN, inst_nvars[b] >= 0, the
 * init ranges and literals likewise -- and a malformed call is SATMI_ERR_ARG
 * with the cause in satmi_last_error(), before any HIP call.  No literal of
 * formula b may lie beyond inst_nvars[b] (the kernels size a formula's image by
 * it); a larger inst_nvars[b] than the formula needs is allowed.  Output
 * pointers that are NULL are outputs the caller does not want. */
int satmi_dpll_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                          const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                          const int32_t *h_inst_nvars,
                          const int32_t *h_init_begin, const int32_t *h_init_lits,
                          int mode, int64_t max_solutions, int64_t node_limit, double time_limit_s,
                          int sol_cap, int sol_stride,
                          int32_t *h_status, int64_t *h_counters, int32_t *h_sol_len,
                          int32_t *h_sol_lits, int32_t *h_root_len, int32_t *h_root_lits);

/*
 * Resolution saturation, replaces resolution_solver (REF.py:63-95) for one
 * clause set (CSR host arrays: clause c = lits[clause_off[c] .. clause_off[c+1])).
 * Clauses are variable bitsets in HBM; each pass resolves all pairs on the GPU
 * (tautologies filtered), dedups through a hash table over every clause key.
 * Thread-safe: a call takes a device workspace (buffers + its own HIP stream)
 * from a process-wide pool and returns it, so calls from several threads overlap.
 *   max_passes / clause_limit / time_limit_s   <= 0: unlimited
 *   *result   1 = True (no new clause derivable), 0 = False (empty resolvent),
 *             -1 = a limit stopped the saturation
 *   *passes   completed passes that added clauses; pass_new[p] = clauses added
 *   optional record (all three non-NULL): clauses new in pass p are
 *   rec_pass_off[p] .. rec_pass_off[p+1] in rec_clause_off / rec_lits, each
 *   clause as ascending literals, the clauses of a pass in ascending order.
 *   The record arrays are truncated at their capacities, silently: a pass's
 *   record stops before the first clause that does not fit rec_lit_cap
 *   literals or rec_clause_cap offsets (it is then a prefix of the pass's
 *   sorted clauses, later passes add what still fits), and passes from
 *   rec_pass_cap - 1 on are not recorded.  Nothing is written past an array's
 *   capacity.  *result, *passes and pass_new are not truncated by the record:
 *   pass_new[p] is exact for every p < pass_cap whatever was recorded.
 * The arrays are checked first (nclauses >= 0, result and passes, with clauses
 * both arrays, clause_off ascending from >= 0, no literal 0 / INT32_MIN): a
 * malformed call is SATMI_ERR_ARG with the cause in satmi_last_error(), before
 * any HIP call (a refused literal leaves *result = -1 and *passes = 0).
 */
int satmi_resolution_host(int nclauses, const int32_t *h_clause_off, const int32_t *h_lits,
                          int64_t max_passes, int64_t clause_limit, double time_limit_s,
                          int32_t *h_result, int32_t *h_passes, int64_t *h_pass_new, int pass_cap,
                          int32_t *h_rec_lits, int64_t rec_lit_cap, int64_t *h_rec_clause_off,
                          int64_t rec_clause_cap, int64_t *h_rec_pass_off, int rec_pass_cap);

/* Work of the last satmi_resolution_host call: pairs resolved, candidate
 * resolvents generated, and the device time of its pair and claim (hash dedup)
 * launches (HIP events on its stream), for rooflines. */
int satmi_resolution_last_stats(int64_t *pairs, int64_t *candidates, double *pair_ms, double *claim_ms);

/* The live shader clock (Hz) of the last satmi_resolution_host call's fused
 * pass kernels (at most 31 variables): shader cycles (s_memtime) over
 * device-clock ticks (s_memrealtime) summed over one block in 64 of every
 * pass, so an issue roofline prices the pipes at the clock the kernel ran
 * at.  0 when no pass kernel ran (the general path beyond 31 variables). */
int satmi_resolution_last_clock(double *shader_hz);

/* What the calling thread's last satmi_resolution_host call regrew or ran
 * again; fills out[0 .. min(n, SATMI_RES_REGROWTHS)).  At most 31 variables
 * (the fused pass; the other words stay 0): passes run again because
 *   out[0]  a stage stripe held only a part of the pass's new keys,
 *   out[1]  the clause list outgrew the key buffer (no stripe spilled),
 *   out[2]  the table stopped the pass (neither of the above).
 * Beyond 31 variables (out[0 .. 3) stay 0):
 *   out[3]  pair chunks run (one per pass unless a pass has more than 2^27 pairs),
 *   out[4]  chunks run again at the counted size of their candidates,
 *   out[5]  tables rebuilt in the middle of a pass,
 *   out[6]  growths of the clause buffer.
 * out[0 .. 3) and out[4], out[6] are zero for a call whose workspace was
 * already large enough. */
#define SATMI_RES_REGROWTHS 7
int satmi_resolution_last_regrowths(int64_t *out, int n);

/* Test knob: the first append slot (default 0) of the pair kernel's candidates
 * (more than 31 variables) or of a pass's new clauses (at most 31), so a small
 * pass exercises the slot arithmetic past 2^31 / 2^32. */
int satmi_resolution_debug_slot_base(int64_t base);

/* Test knob: cap of the candidate buffer of the > 31-variable path in bytes
 * (0 = the default 1 GiB), so a small pass takes the re-run-at-the-counted-size
 * path. */
int satmi_resolution_debug_cand_bytes(int64_t bytes);

/*
 * Batched resolution saturation: many small clause sets in one launch, one
 * workgroup per formula, each saturated entirely in LDS (CSR host arrays as
 * satmi_dpll_batch_host / satmi_cdcl_batch_host).  A formula takes this path
 * when it has at most 31 distinct variables and never holds more keys than the
 * launch's capacity -- chosen from the batch: the smallest of 256 / 1,024 /
 * 2,560 / 4,096 keys that holds 3^d + m for every formula of d <= 31 variables
 * and m clauses, else 4,096; any other formula gets h_result[b] =
 * SATMI_RES_BATCH_UNFIT and is left to satmi_resolution_host.  There is no
 * time limit: a formula's work is bounded by its capacity.
 *   max_passes / clause_limit   <= 0: unlimited (the rule of satmi_resolution_host:
 *                 stop after the first pass that takes the clause count over clause_limit)
 *   h_result[b], h_passes[b]    as satmi_resolution_host's *result / *passes
 *   h_pass_new    [B x pass_cap] rows, zero-filled, exact for every pass < pass_cap
 *   optional record (all three non-NULL): satmi_resolution_host's format and
 *   truncation rules, formula after formula through rec_clause_off / rec_lits;
 *   formula b's pass p is clauses rec_pass_off[b * (pass_cap + 1) + p] ..
 *   rec_pass_off[b * (pass_cap + 1) + p + 1]
 * For an UNFIT formula only h_result[b] carries information: h_passes[b] is 0
 * and its pass_new row all zero.  Arguments are checked before any HIP call
 * (num_instances == 0 returns SATMI_OK).  Thread-safe like satmi_resolution_host.
 */
#define SATMI_RES_BATCH_UNFIT (-2)
int satmi_resolution_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                int64_t max_passes, int64_t clause_limit,
                                int32_t *h_result, int32_t *h_passes, int64_t *h_pass_new, int pass_cap,
                                int32_t *h_rec_lits, int64_t rec_lit_cap, int64_t *h_rec_clause_off,
                                int64_t rec_clause_cap, int64_t *h_rec_pass_off /* [B x (pass_cap + 1)] */);

/* Test knob of satmi_resolution_batch_host (0 = default): at most `grid`
 * workgroups are launched, and a formula holds at most `key_cap` keys, so a few
 * dozen tiny formulas exercise workgroup reuse and the UNFIT path. */
int satmi_resolution_debug_batch(int grid, int key_cap);

/*
 * Davis-Putnam elimination, replaces davis_putnam_solver (REF.py:98-130) for one
 * clause set.  Variables are eliminated in the reference's order (CPython's
 * `set.pop()` on the variable set, modelled on the device), resolvents are
 * generated, tautology-filtered and subsumption-filtered on the GPU.
 *   step_limit / clause_limit / time_limit_s   <= 0: unlimited
 *   *result   1 = True, 0 = False (empty resolvent), -1 = a limit stopped it
 *   trace_vars[k] = variable eliminated at step k; *steps = steps run
 *   optional record (all three non-NULL): the clause list after completed step
 *   s is rec_step_off[s-1] .. rec_step_off[s] in rec_clause_off / rec_lits,
 *   every clause in its Python set iteration order; rec_step_off[s] is left
 *   untouched for a step that ended the elimination.
 * Thread-safe: a call takes a device workspace (buffers kept between calls,
 * its own HIP stream) from a process-wide pool and returns it, so solves from
 * several threads overlap and memory is bounded by the peak concurrency.
 * The arrays are checked first, as satmi_resolution_host checks them: a
 * malformed call is SATMI_ERR_ARG before any HIP call (a refused literal leaves
 * *result = -1 and *steps = 0).
 */
int satmi_dp_host(int nclauses, const int32_t *h_clause_off, const int32_t *h_lits, int64_t step_limit,
                  int64_t clause_limit, double time_limit_s, int32_t *h_result, int32_t *h_trace_vars,
                  int trace_cap, int32_t *h_steps, int32_t *h_rec_lits, int64_t rec_lit_cap,
                  int64_t *h_rec_clause_off, int64_t rec_clause_cap, int64_t *h_rec_step_off, int rec_step_cap);

/*
 * Batched Davis-Putnam elimination: many small clause sets in one launch, one
 * workgroup per formula, every step of the elimination in LDS (CSR host arrays
 * as satmi_resolution_batch_host).  A formula takes this path when
 *   - it has at most 31 distinct variables (a clause is one key P | N << 32
 *     over the dense variable index; the spare bit 31 keeps the all-ones word
 *     from being a key, and key 0, the empty clause, is an ordinary clause);
 *   - no clause list of its elimination, the input included, is longer than
 *     the launch's capacity -- chosen from the batch: the smallest of 512 /
 *     1,024 / 1,920 clauses that holds d x m for every formula of d <= 31
 *     variables and m clauses, else 1,920;
 *   - at every step the live variable ids have pairwise distinct home slots
 *     id & (size - 1) in the table CPython builds for that many ids (8 slots
 *     up to 4 ids, 32 up to 18, 128 up to 76): `variables.pop()` (REF.py:103)
 *     then returns the id of the lowest home slot whatever the insertion
 *     order, which is how the kernel orders the variables.
 * Any other formula gets h_result[b] = SATMI_DP_BATCH_UNFIT and is left to
 * satmi_dp_host; its h_steps[b] is 0 and its rows are zero, whatever progress
 * was made.  There is no time limit: a formula's work is bounded by its capacity.
 *   step_limit / clause_limit   <= 0: unlimited (satmi_dp_host's rules: the step
 *                 limit is checked before the pop; the first event of a step in
 *                 pair order decides between an empty resolvent, 0, and the
 *                 resolvent that takes rest + resolvents over clause_limit, -1)
 *   h_result[b], h_steps[b]     as satmi_dp_host's *result / *steps
 *   h_trace_vars   [B x step_cap]: entry k = the variable eliminated at step k
 *   h_step_clauses [B x step_cap]: entry k = the clause count after completed
 *                 step k; zero-filled (the step that ended an elimination
 *                 completed no list), exact for every step < step_cap
 *   optional record (all three pointers or none; a part of them is an error):
 *   the clause list after every completed step, formula after formula through
 *   rec_clause_off / rec_lits; formula b's list after step k is clauses
 *   rec_step_off[b * (step_cap + 1) + k] .. rec_step_off[b * (step_cap + 1) + k + 1],
 *   in list order.  Every clause's literals are ascending by variable id (+v
 *   before -v) -- NOT satmi_dp_host's set iteration order.  Truncation as
 *   satmi_dp_host's record: a clause needs a free clause offset, literals past
 *   rec_lit_cap are dropped.
 * Arguments are checked before any HIP call (num_instances == 0 returns
 * SATMI_OK).  Thread-safe like satmi_dp_host.
 */
#define SATMI_DP_BATCH_UNFIT (-2)
int satmi_dp_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                        const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                        int64_t step_limit, int64_t clause_limit,
                        int32_t *h_result, int32_t *h_steps,
                        int32_t *h_trace_vars, int64_t *h_step_clauses, int step_cap,
                        int32_t *h_rec_lits, int64_t rec_lit_cap, int64_t *h_rec_clause_off,
                        int64_t rec_clause_cap, int64_t *h_rec_step_off /* [B x (step_cap + 1)] */);

/* Test knob of satmi_dp_batch_host (0 = default): at most `grid` workgroups
 * are launched, and a clause list holds at most `clause_cap` clauses, so a few
 * dozen tiny formulas exercise workgroup reuse and the UNFIT path. */
int satmi_dp_debug_batch(int grid, int clause_cap);

/* The floor of a chain of dependent kernel launches replayed from a HIP graph
 * on this device: `launches` one-block kernels captured in order on one
 * stream, the graph replayed `reps` times; *us_per_launch = the time per
 * launch.  The Davis-Putnam roofline (a solve is a chain of ~280 dependent
 * launches) prices its launches/s against this measured floor. */
int satmi_launch_chain_floor(int launches, int reps, double *us_per_launch);

/* Work of the calling thread's last satmi_dp_host call: elimination steps,
 * subset tests performed by the unique_new filter (REF.py:122-125), new
 * (non-tautological) resolvents, kernel launches enqueued for the steps, key
 * words per clause, and the device time of the step batches (HIP events on its
 * stream), for rooflines. */
int satmi_dp_last_stats(int64_t *steps, int64_t *subset_tests, int64_t *new_clauses, int64_t *launches,
                        int *words, double *device_ms);

/* How often the calling thread's last satmi_dp_host call grew a buffer and ran
 * a step again, per buffer that ran out: out[0] the pair-sized scratch, out[1]
 * the clause-list arrays, out[2] the image arena, out[3] the assembly scratch
 * (a step that ran out of several counts once in each).  All zero for a call
 * whose workspace was already large enough. */
int satmi_dp_last_resumes(int32_t out[4]);

/* Free the idle device workspaces that satmi_dp_host / satmi_resolution_host
 * keep between calls (buffers only grow while kept); calls in flight keep theirs. */
int satmi_dp_trim(void);
int satmi_resolution_trim(void);

/*
 * CDCL, replaces CDCLSolver / cdcl_solve (REF.py:217-384) for a batch of
 * formulas (CSR host arrays as satmi_dpll_batch_host), one wavefront per
 * instance.  The reference's solve loop has no bound of its own (its caller
 * kills it after 60 s): an instance stops after max_iter loop iterations (<= 0:
 * none), at time_limit_s (<= 0: none) or when its arena (sized for learn_cap
 * learned clauses; <= 0: max_iter, else 65536) is full.
 *   h_status[b]   SATMI_CDCL_SAT / _UNSAT (the reference's (True, model) /
 *                 (False, None)), _LIMIT (a bound stopped it), _ERROR (the
 *                 reference raises: KeyError in analyze_conflict), _FULL
 *   h_assign      [B x assign_stride] the assignment dict as signed literals in
 *                 its insertion order (h_assign_len[b] of them): the model for
 *                 _SAT, else the live dict where the run stopped
 *   h_stats       [B x SATMI_CDCL_NSTATS] iterations, conflicts analysed,
 *                 decisions, learned clauses, formula length, watch-list keys,
 *                 decision level, set-table slots used
 *   h_var_inc[b]  the solver's var_inc at the end
 * The arrays are checked first (the count, assign_stride, every pointer of a
 * non-empty batch, both range arrays ascending from >= 0, no literal 0 /
 * INT32_MIN): a malformed call is SATMI_ERR_ARG with the cause in
 * satmi_last_error(), before any HIP call.
 */
#define SATMI_CDCL_UNSAT 0
#define SATMI_CDCL_SAT 1
#define SATMI_CDCL_LIMIT (-1)
#define SATMI_CDCL_ERROR (-2)
#define SATMI_CDCL_FULL (-3)
#define SATMI_CDCL_NSTATS 8
int satmi_cdcl_batch_host(int num_instances, const int32_t *h_inst_clause_begin, const int32_t *h_clause_lit_begin,
                          const int32_t *h_lits, int64_t max_iter, int64_t learn_cap, double time_limit_s,
                          int32_t *h_status, int32_t *h_assign_len, int32_t *h_assign, int assign_stride,
                          int64_t *h_stats, double *h_var_inc);

/* The calling thread's last satmi_cdcl_batch_host launch: its span on the
 * device wall clock (first wave start to last wave end), the busy wave-time
 * (sum over waves of the time spent solving formulas) and the resident waves;
 * busy / (resident x span) is the launch's wave utilisation. */
int satmi_cdcl_last_stats(double *span_s, double *busy_wave_s, int *resident_waves);

/*
 * Batched model check: evaluates assignment rows against their clause sets,
 * one wavefront per instance, every row of an instance in turn (csrc/check.hip).
 * The formulas are CSR arrays as above.  Instance b has `cap` row slots:
 * row r is the first len[b * cap + r] ints of row_lits[(b * cap + r) * stride ..],
 * signed literals -- the layout of satmi_dpll_batch_device's d_sol_len /
 * d_sol_lits with sol_cap / sol_stride, and of satmi_cdcl_batch_host's
 * h_assign_len / h_assign with cap = 1, so a device pipeline checks a solve's
 * models on the same stream right after it, with no copy.
 *   A literal l is TRUE if l is in the row, FALSE if -l is in the row and l is
 *   not, else UNASSIGNED.  A clause is satisfied if some literal is true,
 *   falsified if every literal is false (the empty clause always is), else
 *   undetermined.  The rule is deterministic for malformed rows too: a repeated
 *   literal counts once, and of a contradictory pair +v, -v both literals are
 *   true.
 *   max_vars       the truth table holds variables 1 .. max_vars, two bits each
 *                  in the wavefront's LDS; at most SATMI_CHECK_MAX_VARS (a
 *                  128 KiB table of the CU's 160 KiB), beyond which the call
 *                  returns SATMI_ERR_TOO_LARGE before any launch.  A literal of
 *                  a row with |l| > max_vars (or 0, INT32_MIN) is ignored and
 *                  flagged; such a literal of the formula is unassigned.
 *   max_clause_len longest clause of the batch, 0 = unknown: 1 .. 8 takes the
 *                  lane-per-clause form, anything else the wave-per-clause form
 *                  (same results)
 *   rows           [B] rows to check per instance (clamped to 0 .. cap), NULL =
 *                  cap; the rows from rows[b] on have their four words zeroed
 *   len            [B x cap]; a length is clamped to 0 .. stride
 *   out            [B x cap x SATMI_CHECK_NWORDS]: clauses falsified, clauses
 *                  undetermined, index of the first falsified clause relative
 *                  to the instance's first clause (-1: none), flags.  A row is
 *                  a model iff words 0, 1 and 3 are all 0.
 * The device form is asynchronous on `stream` (NULL = default stream) and owns
 * no device memory.  The host form checks its arguments before any HIP call
 * (num_instances == 0 returns SATMI_OK; a row count outside 0 .. cap or a
 * length outside 0 .. stride is SATMI_ERR_ARG), computes max_vars over the
 * formulas and the rows and max_clause_len itself, and is thread-safe: a call
 * leases a workspace with its own stream, like satmi_resolution_batch_host.
 * UNSAT answers are certified by satmi_check_refutations_* below (SOUND DPLL's
 * own through satmi_dpll_refutations_*).
 */
#define SATMI_CHECK_NWORDS 4          /* per row: falsified, undetermined, first_falsified (-1: none), flags */
#define SATMI_CHECK_CONTRADICTORY 1   /* flags bit: some v with both +v and -v in the row */
#define SATMI_CHECK_BAD_LITERAL 2     /* flags bit: a literal 0, INT32_MIN or |l| > max_vars (ignored) */
#define SATMI_CHECK_MAX_VARS 524287   /* the largest max_vars: (524287 >> 4) + 1 = 32,768 table words */
int satmi_check_models_device(int num_instances, const int32_t *d_inst_clause_begin,
                              const int32_t *d_clause_lit_begin, const int32_t *d_lits, int max_vars,
                              int max_clause_len, const int32_t *d_rows, const int32_t *d_len,
                              const int32_t *d_row_lits, int cap, int stride, int32_t *d_out, void *stream);
int satmi_check_models_host(int num_instances, const int32_t *h_inst_clause_begin,
                            const int32_t *h_clause_lit_begin, const int32_t *h_lits, const int32_t *h_rows,
                            const int32_t *h_len, const int32_t *h_row_lits, int cap, int stride, int32_t *h_out);

/* Test knob of the model check (0 = default): at most `workgroups` workgroups
 * are launched, of `waves_per_wg` (1, 2 or 4) wavefronts each, so a few dozen
 * tiny instances exercise table reuse across instances and every region layout. */
int satmi_check_debug_grid(int workgroups, int waves_per_wg);

/*
 * Batched refutation check: verifies UNSAT answers by forward reverse unit
 * propagation (RUP), one wavefront per instance (csrc/refute.hip).  Instance b
 * has the formula F of the CSR arrays above and the ordered lemma clauses
 * L0 .. Lk-1 of a second CSR triple of the same shape: its lemmas are
 * proof_inst_begin[b] .. proof_inst_begin[b + 1], lemma p's literals
 * proof_clause_begin[p] .. proof_clause_begin[p + 1] of proof_lits.
 *   Lemma Li is VERIFIED if assigning every literal of Li false and running
 *   unit propagation to a fixpoint over F and L0 .. Li-1 reaches a conflict: a
 *   clause whose literals are all false (the empty clause always is), or a
 *   variable needed with both signs.  An earlier lemma is a premise whether or
 *   not it verified: a verdict means "follows by unit propagation from F and
 *   the lemmas before it".  A lemma that holds +v and -v is verified trivially
 *   and sets SATMI_REFUTE_TAUTOLOGY; a repeated literal counts once.  Checking
 *   ends with the instance's first empty lemma, which is checked like any
 *   other; the lemmas behind it are not checked.  Unit propagation is confluent
 *   about reaching a conflict, so every output is independent of scan order.
 *   The record of satmi_resolution_host / satmi_resolution_batch_host (the
 *   clauses each pass added) or of satmi_dp_host / satmi_dp_batch_host (the
 *   clause list after each step), in order, followed by the empty clause when
 *   the result was 0, is such a proof: every recorded clause is a resolvent of
 *   two clauses before it, and the empty one of two opposite unit clauses.
 *   max_vars       the truth table and the trail of assigned variables hold
 *                  variables 1 .. max_vars in the wavefront's LDS; at most
 *                  SATMI_REFUTE_MAX_VARS (8 KiB + 64 KiB), beyond which the call
 *                  returns SATMI_ERR_TOO_LARGE before any launch.  A literal 0,
 *                  INT32_MIN or with |l| > max_vars sets SATMI_REFUTE_BAD_LITERAL:
 *                  a formula clause or an earlier lemma that holds one is
 *                  skipped as a premise (sound), a lemma that holds one fails.
 *   max_clause_len longest clause of formulas and lemmas, 0 = unknown: 1 .. 8
 *                  takes the lane-per-clause form, anything else the
 *                  wave-per-clause form (same results)
 *   out            [B x SATMI_REFUTE_NWORDS]: status, checked lemmas that
 *                  failed, index of the first failed lemma relative to the
 *                  instance's first lemma (-1: none), flags
 *   lemma_ok       [P = proof_inst_begin[B]] or NULL: 1 verified, 0 failed,
 *                  -1 not checked
 * The device form is asynchronous on `stream` (NULL = default stream) and owns
 * no device memory.  The host form checks both triples before any HIP call
 * (num_instances == 0 returns SATMI_OK; a literal 0 / INT32_MIN is
 * SATMI_ERR_ARG), computes max_vars and max_clause_len itself, and is
 * thread-safe: a call leases a workspace with its own stream.
 */
#define SATMI_REFUTE_NWORDS 4         /* per instance: status, failed, first_failed (-1: none), flags */
#define SATMI_REFUTE_FAILED 0         /* status: at least one checked lemma failed */
#define SATMI_REFUTE_PROVEN 1         /* status: no checked lemma failed and an empty lemma was reached */
#define SATMI_REFUTE_OPEN 2           /* status: none failed, no empty lemma reached (an empty proof) */
#define SATMI_REFUTE_TAUTOLOGY 1      /* flags bit: a checked lemma holds both +v and -v */
#define SATMI_REFUTE_BAD_LITERAL 2    /* flags bit: a literal 0, INT32_MIN or |l| > max_vars in the formula or a checked lemma */
#define SATMI_REFUTE_MAX_VARS 32767   /* the largest max_vars: a trail entry is 16 bits */
int satmi_check_refutations_device(int num_instances, const int32_t *d_inst_clause_begin,
                                   const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                   const int32_t *d_proof_inst_begin, const int32_t *d_proof_clause_begin,
                                   const int32_t *d_proof_lits, int max_vars, int max_clause_len, int32_t *d_out,
                                   int32_t *d_lemma_ok, void *stream);
int satmi_check_refutations_host(int num_instances, const int32_t *h_inst_clause_begin,
                                 const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                 const int32_t *h_proof_inst_begin, const int32_t *h_proof_clause_begin,
                                 const int32_t *h_proof_lits, int32_t *h_out, int32_t *h_lemma_ok);

/* Test knob of the refutation check, as satmi_check_debug_grid. */
int satmi_refute_debug_grid(int workgroups, int waves_per_wg);

/*
 * Batched refutation trimming: the backward form of the check above, one
 * wavefront per instance (csrc/trim.hip).  The instances are given as for
 * satmi_check_refutations_*.  Besides a verdict it answers which formula
 * clauses make the formula unsatisfiable (the core) and which lemmas the
 * refutation needs (the trimmed proof).
 *   Let e be the instance's first empty lemma; with none the status is
 *   SATMI_REFUTE_OPEN and nothing is marked.  The lemmas behind e are never
 *   looked at.  Le is marked needed, and i runs e, e-1, .., 0: a lemma that is
 *   not needed is skipped; a needed lemma is checked exactly as the forward
 *   check does it (its literals false, unit propagation over F and L0 .. Li-1,
 *   an earlier lemma a premise whether or not it would verify, a clause with a
 *   bad literal no premise, a needed lemma with a bad literal failed, a
 *   tautological one verified), and every propagated literal remembers the
 *   clause that made it unit.  On a conflict the falsified clause (or the two
 *   clauses that need one variable with both signs) is marked, and,
 *   transitively, the reason of every false literal of a marked clause: a
 *   marked formula clause is in the core, a marked lemma becomes needed.  A
 *   tautological lemma marks nothing.  A needed lemma that reaches no conflict
 *   has failed, marks nothing, and the walk goes on.
 *   The status is SATMI_REFUTE_FAILED if a needed lemma failed, else
 *   SATMI_REFUTE_PROVEN: the core clauses alone, with the needed lemmas in
 *   their order, are a proof that satmi_check_refutations_* accepts with no
 *   failed lemma.  That is weaker than the forward PROVEN: a lemma that does
 *   not verify but that nothing needs does not count.  Where the forward check
 *   reports no failed lemma and reaches an empty lemma, the trim is PROVEN.
 *   Which core is found depends on the propagation order, so the marks are a
 *   function of the inputs and of the clause form (max_clause_len below), and
 *   of nothing else; the two forms may return different, equally valid cores.
 *   max_vars       as above, at most SATMI_TRIM_MAX_VARS: the wavefront's LDS
 *                  holds the truth table, a bitmap of the analysis, the trail
 *                  and a 32-bit reason per trail entry (4 + 2 + 32 + 64 KiB at
 *                  the limit); beyond it the call returns SATMI_ERR_TOO_LARGE
 *                  before any launch
 *   max_clause_len as above: 1 .. 8 the lane-per-clause form, else wave-per-clause
 *   out            [B x SATMI_TRIM_NWORDS]: status, needed lemmas that failed,
 *                  the lowest index of a failed needed lemma (-1: none), flags
 *                  (SATMI_REFUTE_BAD_LITERAL for the formula and the needed
 *                  lemmas, SATMI_REFUTE_TAUTOLOGY for the needed lemmas), the
 *                  number of core clauses (marks that are 1), the number of
 *                  needed lemmas (marks that are not -1)
 *   core           [C = inst_clause_begin[B]]: 1 in the core, 0 not
 *   lemma          [P = proof_inst_begin[B]]: 1 needed and verified, 0 needed
 *                  and failed, -1 not needed
 * The device form is asynchronous on `stream`, owns no device memory and needs
 * no memset: the kernel initialises its instances' ranges of both mark arrays,
 * which are the walk's own state, so neither pointer may be NULL there.  The
 * host form checks both triples before any HIP call, as the forward check's
 * does and with its messages; either of its mark pointers may be NULL; clauses
 * and lemmas before the first instance's ranges read 0 / -1.  It is
 * thread-safe: a call leases a workspace with its own stream.
 */
#define SATMI_TRIM_NWORDS 6           /* per instance: status, failed, first_failed (-1: none), flags, core clauses, kept lemmas */
#define SATMI_TRIM_MAX_VARS 16383     /* the largest max_vars: a 102 KiB region in a CU's 160 KiB */
int satmi_trim_refutations_device(int num_instances, const int32_t *d_inst_clause_begin,
                                  const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                  const int32_t *d_proof_inst_begin, const int32_t *d_proof_clause_begin,
                                  const int32_t *d_proof_lits, int max_vars, int max_clause_len, int32_t *d_out,
                                  int32_t *d_core, int32_t *d_lemma, void *stream);
int satmi_trim_refutations_host(int num_instances, const int32_t *h_inst_clause_begin,
                                const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                const int32_t *h_proof_inst_begin, const int32_t *h_proof_clause_begin,
                                const int32_t *h_proof_lits, int32_t *h_out, int32_t *h_core, int32_t *h_lemma);

/* Test knob of the trim, as satmi_check_debug_grid. */
int satmi_trim_debug_grid(int workgroups, int waves_per_wg);

/*
 * Batched witness models: rebuilds an assignment from the record of a
 * Davis-Putnam elimination or of a resolution saturation that answered True,
 * and evaluates it against the formula, one wavefront per instance
 * (csrc/witness.hip).  Instance b has the formula F (m clauses) of the first
 * CSR triple, the record R (P clauses) of a second triple shaped like the
 * proofs above, and the stages inst_stage_begin[b] .. inst_stage_begin[b + 1].
 * Clause index c < m is formula clause c, index m + j record clause j.
 *   The assignment is total: every variable starts False.  Stage (x, lo, hi),
 *   0 <= lo <= hi <= m + P, reads the clauses lo .. hi - 1 under the assignment
 *   as it stands; the stages are processed in order, and ranges may overlap,
 *   repeat and straddle m.  A clause that holds +x and -x is passed, and with
 *   highest_only = 1 so is a clause whose largest |literal| is not x.  needP
 *   holds if some clause holds +x and every other literal of it is false, needN
 *   likewise with -x; with both the stage is STUCK.  In every case x becomes
 *   needP (a variable may be decided again by a later stage).  After the last
 *   stage every clause of F is evaluated: the status is SATMI_WITNESS_MODEL iff
 *   none is falsified.  The status does not depend on how the stages came
 *   about, so it is sound for any input; the stuck count is diagnostic.  Every
 *   output is a function of the inputs alone (not of lane order, grid or clause
 *   form).
 *   The record of satmi_dp_host / satmi_dp_batch_host with result 1 gives the
 *   stages (var[k], the clause list before step k), last step first; that of
 *   satmi_resolution_host / satmi_resolution_batch_host with result 1 gives one
 *   stage (v, 0, m + P) per variable, ascending, with highest_only = 1
 *   (satmi/witness.py builds both).
 *   max_vars       the table holds a value bit and an "occurs in F" bit for the
 *                  variables 1 .. max_vars in the wavefront's LDS; at most
 *                  SATMI_WITNESS_MAX_VARS (satmi_check_models_*'s limit, so any
 *                  witness can be checked), beyond which the call returns
 *                  SATMI_ERR_TOO_LARGE before any launch.  A literal 0,
 *                  INT32_MIN or with |l| > max_vars counts as false (and as a
 *                  magnitude for highest_only) and sets
 *                  SATMI_WITNESS_BAD_LITERAL when it is in F or in a clause that
 *                  a stage reads.  A stage whose variable is outside
 *                  1 .. max_vars is skipped and sets SATMI_WITNESS_BAD_STAGE.
 *   max_clause_len longest clause of formulas and records, 0 = unknown: 1 .. 8
 *                  takes the lane-per-clause form, anything else the
 *                  wave-per-clause form (same results)
 *   out            [B x SATMI_WITNESS_NWORDS]: status, stuck stages, index of
 *                  the first stuck stage relative to the instance's first stage
 *                  (-1: none), flags, falsified clauses of F, index of the first
 *                  falsified clause (-1: none)
 *   row_len, row_lits, stride   [B], [B x stride]: the assignment as a row of
 *                  satmi_check_models_* (cap = 1): one signed literal per
 *                  distinct variable that occurs in F with a good literal,
 *                  ascending by variable, the sign by its final value.  A row
 *                  longer than stride sets SATMI_WITNESS_ROW_TRUNCATED: its
 *                  first stride literals are written, row_len holds the count.
 * The device form is asynchronous on `stream`, owns no device memory, trusts
 * the CSR ranges and clamps a stage's range to 0 .. m + P.  The host form
 * checks both triples before any HIP call as satmi_check_refutations_host does
 * ("formulas: ", "records: "), and refuses ("stages: ") descending
 * inst_stage_begin, a stage variable outside 1 .. max_vars and a range outside
 * 0 <= lo <= hi <= m + P; it computes max_vars and max_clause_len itself, writes
 * 0 to the words of a row behind its length, and is thread-safe: a call leases
 * a workspace with its own stream.
 */
#define SATMI_WITNESS_NWORDS 6          /* per instance: status, stuck, first_stuck (-1), flags, falsified, first_falsified (-1) */
#define SATMI_WITNESS_NOT_MODEL 0       /* status: the assignment falsifies a clause of F */
#define SATMI_WITNESS_MODEL 1           /* status: the assignment satisfies every clause of F */
#define SATMI_WITNESS_BAD_LITERAL 1     /* flags bit: a literal 0, INT32_MIN or |l| > max_vars was read (false) */
#define SATMI_WITNESS_BAD_STAGE 2       /* flags bit: a stage variable outside 1 .. max_vars (the stage is skipped) */
#define SATMI_WITNESS_ROW_TRUNCATED 4   /* flags bit: the row is longer than stride */
#define SATMI_WITNESS_MAX_VARS 524287   /* the largest max_vars: SATMI_CHECK_MAX_VARS */
int satmi_witness_models_device(int num_instances, const int32_t *d_inst_clause_begin,
                                const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                const int32_t *d_record_inst_begin, const int32_t *d_record_clause_begin,
                                const int32_t *d_record_lits, const int32_t *d_inst_stage_begin,
                                const int32_t *d_stage_var, const int32_t *d_stage_lo, const int32_t *d_stage_hi,
                                int highest_only, int max_vars, int max_clause_len, int32_t *d_out,
                                int32_t *d_row_len, int32_t *d_row_lits, int stride, void *stream);
int satmi_witness_models_host(int num_instances, const int32_t *h_inst_clause_begin,
                              const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                              const int32_t *h_record_inst_begin, const int32_t *h_record_clause_begin,
                              const int32_t *h_record_lits, const int32_t *h_inst_stage_begin,
                              const int32_t *h_stage_var, const int32_t *h_stage_lo, const int32_t *h_stage_hi,
                              int highest_only, int32_t *h_out, int32_t *h_row_len, int32_t *h_row_lits,
                              int stride);

/* Test knob of the witness kernel, as satmi_check_debug_grid. */
int satmi_witness_debug_grid(int workgroups, int waves_per_wg);

/*
 * Refutations of SATMI_MODE_SOUND DPLL: the batched DPLL above, run by the
 * general kernel (its LDS form, or SATMI_KERNEL_WIDE for what that form does
 * not hold; never a clause kernel) in a form that logs why every closed
 * subtree holds no model, followed by a pack of the logs into the proof triple
 * of satmi_check_refutations_* / satmi_trim_refutations_* (csrc/dpll.hip,
 * csrc/dpll_proof.hip).  The search is always SOUND and takes no caller
 * assignment: an assumption is nothing a lemma could discharge.  Statuses,
 * counters, models and root assignments are those of satmi_dpll_batch_device;
 * an instance the general kernel answers SATMI_DPLL_TOO_LARGE stays so.
 *   A node of the search is its decision path, the frames d1 .. dk (a variable
 *   and the phase that runs).  The wave logs one lemma whenever a subtree is
 *   closed without a solution: at a conflict the clause -d1 .. -dk of the path,
 *   and when a frame is popped after its False phase the same clause of the
 *   frames below it.  A search that ends SATMI_DPLL_EXHAUSTED with no solution
 *   logs its tree in post-order and ends with the empty clause, decisions + 1
 *   lemmas in all, conflicts = decisions / 2 + 1.  Every lemma follows by unit
 *   propagation from the formula and the lemmas before it: a leaf's because
 *   what the solver propagated on the path are unit consequences of the
 *   decisions, an inner node's from its two children's lemmas.  Pure-literal
 *   assignments are in no lemma and need not be: a literal p is pure when no
 *   active clause holds -p, so below that point no unit clause and no emptied
 *   clause counts -p among its false literals; the checker, which never
 *   assigns p, only has more clauses active, and unit propagation is monotone
 *   in its premises.
 *   log, log_begin   instance b logs into log[log_begin[b] .. log_begin[b + 1])
 *                  (int64 offsets, ascending), one record `len, lit_1 .. lit_len`
 *                  of signed literals in frame order per lemma.  A record that
 *                  does not fit is counted and not written.
 *   info           [B x SATMI_DPLL_PROOF_NWORDS] int64: lemmas logged, log words
 *                  needed (both exact, whatever the region held), flags
 *                  (SATMI_DPLL_PROOF_TRUNCATED: the region was too small), and
 *                  the offset of the instance's first literal in proof_lits
 *   proof_inst_begin [B + 1], proof_clause_begin [proof_clause_cap + 1],
 *   proof_lits [proof_lit_cap]   the proof triple.  An instance has its lemmas
 *                  there when it ended EXHAUSTED with no solution and its log
 *                  was not truncated, else none (the check reports
 *                  SATMI_REFUTE_OPEN).
 *   totals         [2] int64: lemmas and literals of the whole proof.  When they
 *                  exceed a capacity (or 2^31 - 1), every instance has no lemma,
 *                  nothing is written past a capacity, and the caller calls
 *                  again with arrays of the totals' size.
 * The device form is asynchronous on `stream` and owns no device memory beyond
 * the per-stream state of satmi_dpll_batch_device; its proof triple feeds the
 * check and the trim on the same stream with no copy.  The host form checks its
 * arguments before any HIP call as satmi_dpll_batch_host does (and refuses a
 * capacity below 1), sizes the log itself and runs again with the counted sizes
 * until no refuted instance is truncated; h_info and the solution and root
 * outputs may be NULL.  It is thread-safe: a call leases a workspace with its
 * own stream.
 */
#define SATMI_DPLL_PROOF_NWORDS 4      /* per instance: lemmas, log words needed, flags, first literal offset */
#define SATMI_DPLL_PROOF_TRUNCATED 1   /* flags bit: the instance's log region was too small */
int satmi_dpll_refutations_device(int num_instances, const int32_t *d_inst_clause_begin,
                                  const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                  const int32_t *d_inst_nvars, int max_vars, int max_clauses, int max_lits,
                                  int max_clause_len, int64_t max_solutions, int64_t node_limit,
                                  double time_limit_s, int sol_cap, int sol_stride,
                                  int32_t *d_status, int64_t *d_counters, int32_t *d_sol_len,
                                  int32_t *d_sol_lits, int32_t *d_root_len, int32_t *d_root_lits,
                                  int32_t *d_log, const int64_t *d_log_begin,
                                  int32_t *d_proof_inst_begin, int32_t *d_proof_clause_begin,
                                  int64_t proof_clause_cap, int32_t *d_proof_lits, int64_t proof_lit_cap,
                                  int64_t *d_info, int64_t *d_totals, void *stream);
int satmi_dpll_refutations_host(int num_instances, const int32_t *h_inst_clause_begin,
                                const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                const int32_t *h_inst_nvars, int64_t max_solutions, int64_t node_limit,
                                double time_limit_s, int sol_cap, int sol_stride,
                                int32_t *h_status, int64_t *h_counters, int32_t *h_sol_len,
                                int32_t *h_sol_lits, int32_t *h_root_len, int32_t *h_root_lits,
                                int32_t *h_proof_inst_begin, int32_t *h_proof_clause_begin,
                                int64_t proof_clause_cap, int32_t *h_proof_lits, int64_t proof_lit_cap,
                                int64_t *h_info, int64_t *h_totals);

/* Test knob of satmi_dpll_refutations_host (0 = default): the log words every
 * instance gets in the first run, so a small search takes the run-again path. */
int satmi_dpll_refutations_debug_room(int64_t words);

/*
 * Sound CDCL: a clause-learning search whose learned clauses are its proof, one
 * wavefront per formula, batched over a persistent grid (csrc/cdcl_sound.hip).
 * Unlike satmi_cdcl_batch_host above, which mirrors the reference's CDCLSolver
 * step for step, this is a decision procedure: it answers SAT with a model that
 * is a row of satmi_check_models_*, or UNSAT with a refutation that
 * satmi_check_refutations_* / satmi_trim_refutations_* read.  Every output is a
 * function of the formula and conflict_limit alone (not of the grid, of lane
 * timing or of the clause form), by the rule below; tests/cdcl_sound_rows.py
 * restates it in Python.
 *   Clause indices: formula clauses are 0 .. m-1, learned clause j is m + j.
 *   Evaluating a clause: a repeated literal counts once; a clause is satisfied
 *   if some literal is true, falsified if every literal is false (the empty
 *   clause always is), unit if no literal is true and all its unassigned
 *   literals are one and the same literal.  A clause that holds +v and -v is
 *   therefore never unit or falsified.
 *   Propagation runs in rounds.  Every clause is evaluated under the assignment
 *   as it stood at the round's start.  If any clause is falsified, the conflict
 *   is the lowest-indexed one and the round implies nothing.  Otherwise each
 *   variable implied by some unit clause takes the sign and the reason of the
 *   lowest-indexed clause implying it, at the current decision level, and the
 *   implied variables enter the trail in ascending order of that clause index.
 *   A round that implies nothing is the fixpoint.
 *   Conflicts: a conflict at level 0 gives UNSAT.  Otherwise, if conflict_limit
 *   > 0 and this is conflict number conflict_limit, the instance ends LIMIT.
 *   Otherwise first-UIP analysis runs backwards over the trail: starting from
 *   the conflict clause, the literals of the clause at hand (but the one just
 *   resolved on) whose variables are above level 0 are marked; the clause at
 *   hand becomes the reason of the marked variable nearest the trail's end,
 *   which loses its mark, until that variable is the only marked one of the
 *   current level.  Level-0 literals are dropped.  The learned clause is the
 *   negation of that variable's trail literal (the asserting literal), first,
 *   and the negated trail literals of the other marked variables in descending
 *   trail position.  The search backjumps to the highest level among the
 *   others, or to 0 for a unit clause: every variable above that level is
 *   unassigned and its value saved as its phase.  Each variable of the learned
 *   clause gains 1 activity; after a conflict whose number is a multiple of 256
 *   every activity is halved (integers, rounding down).  Propagation follows;
 *   its first round finds the learned clause unit.
 *   Decisions, at a fixpoint: the candidates are the unassigned variables that
 *   occur in the formula.  SAT holds when none is left.  Otherwise the one of
 *   the highest activity, the lowest id on a tie, opens a new level with its
 *   saved phase, initially False.  There are no restarts.
 *   max_vars       the wavefront's LDS holds, per variable of 0 .. max_vars, a
 *                  32-bit reason, a mark bit, 16 bits each of level, trail and
 *                  activity, and a byte of value, phase and "occurs": 89 KiB at
 *                  SATMI_CDCL_SOUND_MAX_VARS, beyond which the call returns
 *                  SATMI_ERR_TOO_LARGE before any launch.  An instance with
 *                  inst_nvars[b] > max_vars, or a literal 0, INT32_MIN or beyond
 *                  inst_nvars[b], ends SATMI_CDCL_SOUND_TOO_LARGE untouched.
 *   max_clause_len longest clause of the formulas, 0 = unknown: 1 .. 8 takes the
 *                  lane-per-clause form, anything else the wave-per-clause form
 *                  (same results); learned clauses are always read wave-per-clause
 *   time_limit_s   per-instance wall-clock limit (<= 0 = none), looked at once per
 *                  conflict and decision: the instance ends LIMIT
 *   lemmas, lemma_begin   instance b keeps its learned clauses in
 *                  lemmas[lemma_begin[b] .. lemma_begin[b + 1]) (int64 offsets,
 *                  ascending), one record `len, lit_1 .. lit_len` each, in the order
 *                  learned: the clause database and the proof log at once.  On
 *                  UNSAT the record `0`, the empty clause, closes it.  A record
 *                  that does not fit is counted and never written, in part or
 *                  whole, and the instance ends FULL (so does one whose offsets
 *                  m + words would pass 2^31 - 1).
 *   status         [B] SATMI_CDCL_SOUND_*
 *   counters       [B x SATMI_CDCL_SOUND_NCOUNTERS] int64: conflicts, decisions,
 *                  propagated literals, rounds, learned clauses, learned
 *                  literals, highest level, restarts (0)
 *   row_len, row_lits, stride   [B], [B x stride]: for SAT the model as a row of
 *                  satmi_check_models_* (cap = 1): one signed literal per variable
 *                  that occurs in the formula, ascending; row_len holds the count,
 *                  the first stride literals are written.  Else row_len is 0.
 *   info           [B x SATMI_CDCL_SOUND_NWORDS] int64: records (the closing
 *                  empty clause and a record that did not fit included), region
 *                  words needed, flags (SATMI_CDCL_SOUND_TRUNCATED with FULL), and,
 *                  after the pack, the offset of the instance's first literal
 *                  in proof_lits
 * The device form is asynchronous on `stream` and owns no device memory.  The
 * pack, on the same stream, turns the regions into the proof triple (as
 * satmi_dpll_refutations_device's does: an instance has its lemmas there when
 * it ended UNSAT, else none; totals [2] = lemmas and literals of the whole
 * proof, and when they exceed a capacity every instance has no lemma and
 * nothing is written past a capacity), so the solve, the pack, the check and the
 * trim run on one stream with no copy.
 * Why the proof checks: when clause j is learned, assigning its literals false
 * repeats, for the checker, the trail below the asserting level together with
 * the negated UIP; every reason clause the analysis resolved on then becomes
 * unit in reverse resolution order (its other literals are false: they are in
 * the learned clause, or were resolved on later, or hold at level 0, which unit
 * propagation over F and the earlier lemmas reaches as the solver did), and the
 * conflict clause is falsified.  The checker's propagation is a fixpoint, so
 * order does not matter.  The closing empty clause follows from the level-0
 * conflict in the same way.
 * The host form checks its arguments before any HIP call as
 * satmi_dpll_refutations_host does (and refuses stride < the largest inst_nvars),
 * sizes the regions itself and runs again with four times the room while an
 * instance ended FULL, up to room_cap words per instance (0 = as much as the
 * 32-bit offsets allow).  A run-again repeats the whole batch, the instances
 * that had finished included (only the FULL ones get more room; the search is
 * deterministic, so the others end as before): one outlier costs its batch up
 * to a dozen runs, and a caller who expects one gives it a batch of its own or
 * a room_cap.  Likewise a proof that outgrows proof_clause_cap / proof_lit_cap
 * is reported in h_totals with no lemma written, and the call that fetches it
 * with larger arrays solves again.  h_info alone of the outputs may be NULL (an
 * output the caller does not want); a proof capacity beyond the 32-bit offsets
 * of the proof arrays (2^31 - 2 lemmas, 2^31 - 1 literals) is refused.  It is
 * thread-safe: a call leases a workspace with its own stream.
 */
#define SATMI_CDCL_SOUND_UNSAT 0
#define SATMI_CDCL_SOUND_SAT 1
#define SATMI_CDCL_SOUND_LIMIT 2       /* conflict_limit or time_limit_s stopped it */
#define SATMI_CDCL_SOUND_FULL 3        /* a learned clause did not fit the instance's region */
#define SATMI_CDCL_SOUND_TOO_LARGE 4   /* the instance does not fit the launch's layout */
#define SATMI_CDCL_SOUND_NCOUNTERS 8
#define SATMI_CDCL_SOUND_NWORDS 4      /* per instance: records, region words needed, flags, first literal offset */
#define SATMI_CDCL_SOUND_TRUNCATED 1   /* flags bit: the instance's region was too small */
#define SATMI_CDCL_SOUND_MAX_VARS 8191 /* the largest max_vars: an 89 KiB region in a CU's 160 KiB */
int satmi_cdcl_sound_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                  const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                  const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                  int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                  const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                  int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                  void *stream);
int satmi_cdcl_sound_pack_device(int num_instances, const int32_t *d_status, const int32_t *d_lemmas,
                                 const int64_t *d_lemma_begin, int64_t *d_info, int32_t *d_proof_inst_begin,
                                 int32_t *d_proof_clause_begin, int64_t proof_clause_cap, int32_t *d_proof_lits,
                                 int64_t proof_lit_cap, int64_t *d_totals, void *stream);
int satmi_cdcl_sound_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                int64_t room_cap, int32_t *h_status, int64_t *h_counters, int32_t *h_row_len,
                                int32_t *h_row_lits, int stride, int32_t *h_proof_inst_begin,
                                int32_t *h_proof_clause_begin, int64_t proof_clause_cap, int32_t *h_proof_lits,
                                int64_t proof_lit_cap, int64_t *h_info, int64_t *h_totals);

/* Test knobs of the sound CDCL (0 = default): the grid as satmi_check_debug_grid;
 * the region words every instance gets in the host form's first run, so a small
 * search takes the run-again path. */
int satmi_cdcl_sound_debug_grid(int workgroups, int waves_per_wg);
int satmi_cdcl_sound_debug_room(int64_t words);

/* LDS bytes one wavefront needs at this max_vars (0 = beyond the limit). */
uint64_t satmi_cdcl_sound_lds_bytes(int max_vars);

/*
 * Sound CDCL under assumptions: is F satisfiable under the literals a_1 .. a_k,
 * and if not, which of them are to blame?  The assumption-carrying form of the
 * search above (csrc/cdcl_sound.hip, its own kernel instantiations; the ones
 * above keep their machine code).  Instance b assumes
 * assume_lits[assume_begin[b] .. assume_begin[b + 1]) (int32 offsets, ascending),
 * in that order.  Every output is a function of the formula, the assumption
 * list and conflict_limit alone, by the rule above with these additions;
 * tests/cdcl_assume_rows.py restates it in Python.
 *   Occurs: a variable occurs if it is in the formula or in the assumptions.
 *   Decision candidates and the model row are over these variables, so
 *   inst_nvars[b] covers the assumptions' variables too.
 *   Assumption levels: level i <= k belongs to a_i.  At a fixpoint with the
 *   current level cur < k, let a = a_(cur+1).  If a is true, cur becomes cur + 1:
 *   an empty level; nothing is assigned and nothing is counted as a decision.  If
 *   a is unassigned, cur becomes cur + 1 and a is assigned at that level with no
 *   reason, as a decision is, and enters the trail; it is not counted in
 *   `decisions`.  In both cases the highest level is updated and propagation
 *   follows with its own round.  If a is false, the instance ends
 *   SATMI_CDCL_SOUND_ASSUMED, UNSAT under the assumptions, after the final
 *   analysis below.  Free decisions start only once cur >= k; SAT is answered
 *   only there.  Conflicts, analysis, learning, backjumps, activities, phases
 *   and conflict_limit are unchanged: a backjump below level k simply re-opens
 *   the assumption levels in order, and a conflict at level 0 is UNSAT as
 *   before, with an empty core and a refutation of F alone.
 *   Final analysis, when a is false: the core starts as [a], and var(a) is
 *   marked if its level is above 0.  The trail is walked from its end down to
 *   the first level-0 entry: a marked variable with no reason (at these levels
 *   always an assumption) appends its trail literal to the core; a marked
 *   variable with a reason marks the other literals of its reason clause whose
 *   level is above 0.  The core is therefore a first, then assumptions in
 *   descending trail position: a sublist of the assumptions as literals, [a]
 *   alone when -a holds at level 0, [a, -a] when the assumptions contradict
 *   each other.  It need not be minimal (satmi_cdcl_shrink_batch_* below
 *   shrinks it until it is).
 *   Limits: an instance with more than SATMI_CDCL_SOUND_MAX_VARS assumptions, or
 *   with an assumption literal 0, INT32_MIN or beyond inst_nvars[b], ends
 *   TOO_LARGE untouched; levels therefore stay below 2^16.  The assumptions are
 *   read from the caller's arrays where they lie, never copied to LDS.
 *   core_len, core_lits, core_stride   [B], [B x core_stride]: for ASSUMED the
 *                  core; core_len holds the count, the first core_stride
 *                  literals are written (core_stride >= 0; a core has at most
 *                  k literals).  Else core_len is 0.
 * With ASSUMED the region is closed by the empty record, as with UNSAT (and ends
 * FULL, with no core, when that record does not fit).  satmi_cdcl_assume_pack_device
 * is the pack above that also gives ASSUMED instances their lemmas; the pack
 * above is unchanged and gives them none.
 * Why the proof checks: the lemma list, the empty clause last, is a RUP
 * refutation of F together with the core's literals as unit clauses.  Every
 * lemma but the last is RUP from F and the earlier lemmas alone, by the argument
 * above: an assumption is on the trail as a decision is, and the analysis never
 * resolves on it, so no lemma depends on the assumptions but through its own
 * literals.  The empty clause follows because unit propagation over F, the
 * lemmas and the core's units reaches -a as the solver's assumption levels did:
 * the final analysis marked exactly the variables that the derivation of -a
 * rests on above level 0, each of them either a core literal, which is a unit
 * clause, or implied by a reason clause whose other literals are marked or hold
 * at level 0, which propagation reaches as the solver did; and a itself is a
 * unit clause, so -a falsifies it.  The checker's propagation is a fixpoint, so
 * order does not matter.  satmi_check_refutations_* and satmi_trim_refutations_*
 * read that pair as they read any other; neither kernel changes.
 * With no assumptions (assume_begin all equal) every output -- status, counters,
 * model row, region words, info -- equals satmi_cdcl_sound_batch_*'s.
 * The host form checks its arguments before any HIP call as
 * satmi_cdcl_sound_batch_host does, and the assumption arrays as
 * satmi_dpll_batch_host checks its init ranges (NULL or descending
 * assume_begin, an assumption literal 0, INT32_MIN or beyond inst_nvars[b] and a
 * negative core_stride are refused; h_core_lits may be NULL when core_stride is
 * 0); it shares the run-again loop, the workspace pool and the thread safety.
 */
#define SATMI_CDCL_SOUND_ASSUMED 5     /* UNSAT under the assumptions: core_len / core_lits hold the failed ones */
int satmi_cdcl_assume_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                   const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                   const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                   int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                   const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                   int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                   const int32_t *d_assume_begin, const int32_t *d_assume_lits, int32_t *d_core_len,
                                   int32_t *d_core_lits, int core_stride, void *stream);
int satmi_cdcl_assume_pack_device(int num_instances, const int32_t *d_status, const int32_t *d_lemmas,
                                  const int64_t *d_lemma_begin, int64_t *d_info, int32_t *d_proof_inst_begin,
                                  int32_t *d_proof_clause_begin, int64_t proof_clause_cap, int32_t *d_proof_lits,
                                  int64_t proof_lit_cap, int64_t *d_totals, void *stream);
int satmi_cdcl_assume_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                 const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                 const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                 int64_t room_cap, int32_t *h_status, int64_t *h_counters, int32_t *h_row_len,
                                 int32_t *h_row_lits, int stride, int32_t *h_proof_inst_begin,
                                 int32_t *h_proof_clause_begin, int64_t proof_clause_cap, int32_t *h_proof_lits,
                                 int64_t proof_lit_cap, int64_t *h_info, int64_t *h_totals,
                                 const int32_t *h_assume_begin, const int32_t *h_assume_lits, int32_t *h_core_len,
                                 int32_t *h_core_lits, int core_stride);

/*
 * Incremental sound CDCL: the search above, started with lemmas that an earlier
 * query on the same formula learned.  Every lemma of the assumption-carrying
 * search follows from F alone, so it is still valid for the next query on F
 * under other assumptions, and stays valid when clauses are added to F.
 * satmi_cdcl_carry_batch_device (csrc/cdcl_sound.hip, a third instantiation of
 * the search kernel; the ones above keep their machine code) takes and returns
 * them where they lie, in the instance's region.  The assumption rule holds,
 * with these additions; tests/cdcl_carry_rows.py restates them in Python.
 *   Carried lemmas: carry_in[b] = (records, words), int64 [B x 2]: the first
 *   `words` words of instance b's region hold `records` records
 *   `len, lit_1 .. lit_len`, clauses that the caller asserts to follow from F.
 *   They are the learned clauses m+0 .. m+p-1 in the order given, under the
 *   reason codes already in place (m + word offset), and the clauses learned in
 *   this call follow them.  From the first round on they are evaluated, offer
 *   units, become conflicts and serve as reasons exactly as learned clauses do.
 *   Their variables occur: they are decision candidates and are in the model
 *   row.  A NULL carry_in carries nothing anywhere.
 *   What is not carried: activities start at 0 and phases at False.  The
 *   counters conflicts, learned and learned literals, and the conflict number
 *   that conflict_limit and the halving look at, count this call only.  A
 *   search that ended LIMIT and is resumed from its kept lemmas is therefore a
 *   restart from level 0 with those lemmas.  Every output is a function of the
 *   formula, the assumptions, conflict_limit and the carried list alone.
 *   Empty carry: with no carried lemma every output equals
 *   satmi_cdcl_assume_batch_*'s, word for word.
 *   The proof: the region's records, the carried lemmas first and then, with
 *   UNSAT or ASSUMED, the empty clause last, are the refutation of F plus the
 *   core's unit clauses.  info[0] and info[1], the region's records and words,
 *   count the carried ones too, so satmi_cdcl_assume_pack_device turns such a
 *   region into the proof triple unchanged.  A carried list is an earlier
 *   call's lemma sequence: each lemma is RUP from that call's formula and its
 *   predecessors, hence from any formula that contains it and the same
 *   predecessors; the lemmas of this call are RUP from F, the carried ones and
 *   their own predecessors by the arguments above.
 *   Who vouches for the carry: that a carried clause follows from F is the
 *   caller's claim and the checker's verdict, not the solver's.  A carried
 *   clause that does not follow from F can make a satisfiable F UNSAT; the
 *   refutation check then fails at that lemma.
 *   carry_out[b] = (records, words) of the non-empty records in the region at
 *   the end: the carried ones and those learned and written, without the closing
 *   empty record and without a record that did not fit (FULL).  It is what the
 *   next query carries.  Only instance b's wavefront reads or writes entry b, so
 *   carry_in and carry_out may be one array, and a chain of queries runs in
 *   place on one stream with no copy and no pack in between.
 *   Malformed carry: the instance ends SATMI_CDCL_SOUND_TOO_LARGE with the info
 *   flag SATMI_CDCL_SOUND_BAD_CARRY, its region untouched and carry_out[b] =
 *   (0, 0), when records or words is negative; the words exceed the region (or
 *   m + words would pass 2^31 - 1); a record's length is below 1 (an empty
 *   record is refused: the closing record of an earlier answer is never
 *   carried); a record runs past the stated words, or the chain does not end
 *   exactly on them after exactly the stated records; or a literal is 0,
 *   INT32_MIN or beyond inst_nvars[b].  An instance that is TOO_LARGE for
 *   another reason writes its carry_in back.
 * satmi_cdcl_carry_pack_device packs every instance's kept lemmas, whatever its
 * status, from `carry` (a carry_out) as a clause triple: instance b's clauses
 * are kept_clause_begin[kept_inst_begin[b] .. kept_inst_begin[b + 1]]; totals
 * [2] = lemmas and literals, and when they exceed a capacity (>= 0) no instance
 * has a lemma and nothing is written past a capacity.  Counts that no region
 * holds contribute nothing.
 * The host form takes the carried lemmas as such a triple (h_carry_inst_begin
 * [B + 1], h_carry_clause_begin, h_carry_lits; all three NULL: none) and
 * returns the kept ones as one (the three arrays may be NULL with both
 * capacities 0).  h_totals is [4]: proof lemmas, proof literals, kept lemmas,
 * kept literals, the kept ones reported as the proof's are.  It checks all of
 * it before any HIP call as satmi_cdcl_assume_batch_host does: the carry triple
 * as a CSR pair, no empty clause, literals within inst_nvars[b] (a malformed
 * carry is refused here, never launched).  Each region is the carried words
 * plus the usual first room; a run-again starts from the input carry with four
 * times the room, so the answer is the same whatever the first room was.  A
 * room_cap below an instance's carried words refuses its carry (BAD_CARRY).
 */
#define SATMI_CDCL_SOUND_BAD_CARRY 2   /* flags bit: the carried records were malformed (with TOO_LARGE) */
int satmi_cdcl_carry_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                  const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                  const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                  int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                  const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                  int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                  const int32_t *d_assume_begin, const int32_t *d_assume_lits, int32_t *d_core_len,
                                  int32_t *d_core_lits, int core_stride, const int64_t *d_carry_in,
                                  int64_t *d_carry_out, void *stream);
int satmi_cdcl_carry_pack_device(int num_instances, const int32_t *d_lemmas, const int64_t *d_lemma_begin,
                                 const int64_t *d_carry, int32_t *d_kept_inst_begin, int32_t *d_kept_clause_begin,
                                 int64_t kept_clause_cap, int32_t *d_kept_lits, int64_t kept_lit_cap,
                                 int64_t *d_totals, void *stream);
int satmi_cdcl_carry_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                int64_t room_cap, int32_t *h_status, int64_t *h_counters, int32_t *h_row_len,
                                int32_t *h_row_lits, int stride, int32_t *h_proof_inst_begin,
                                int32_t *h_proof_clause_begin, int64_t proof_clause_cap, int32_t *h_proof_lits,
                                int64_t proof_lit_cap, int64_t *h_info, int64_t *h_totals,
                                const int32_t *h_assume_begin, const int32_t *h_assume_lits, int32_t *h_core_len,
                                int32_t *h_core_lits, int core_stride, const int32_t *h_carry_inst_begin,
                                const int32_t *h_carry_clause_begin, const int32_t *h_carry_lits,
                                int32_t *h_kept_inst_begin, int32_t *h_kept_clause_begin, int64_t kept_clause_cap,
                                int32_t *h_kept_lits, int64_t kept_lit_cap);

/*
 * Minimal failed-assumption cores: deletion-based minimisation with core
 * refinement, the whole chain of an instance in one launch.
 * satmi_cdcl_shrink_batch_device (csrc/cdcl_sound.hip, a fourth instantiation
 * of the search kernel; the ones above keep their machine code) takes an
 * instance of satmi_cdcl_carry_batch_device: formula F, assumptions a_1 .. a_k,
 * conflict_limit, carried lemmas.  Its wavefront runs a chain of carrying
 * searches on it; tests/cdcl_shrink_rows.py restates the chain in Python as a
 * composition of the carrying rule.
 *   Query 0 is the carrying search on the assumptions as given.  If it ends
 *   anything but ASSUMED the instance ends there, and every output that the
 *   carrying entry point has is that entry point's, word for word.
 *   Otherwise let W be query 0's core in the order reported and p = 0.  While
 *   p < |W|: the trial list is W without W[p], order kept, and the wavefront
 *   runs the carrying search on F under the trial list.  That search carries
 *   every non-empty record now in the region; the closing empty record of the
 *   query before is dropped first, as carry_out drops it.  Activities, phases
 *   and the conflict number that conflict_limit and the halving look at start
 *   afresh, as the carry rule says of any resumed search, and the variables
 *   that occur are those of F, of the records and of the trial list, as in any
 *   carrying search under that list.  Then, as the trial ends
 *     ASSUMED with core C: W becomes the trial list's members that are in C, in
 *       W's order; p is unchanged.  (C comes out the refuted assumption first
 *       and then by descending level, the trial list's order backwards.)
 *     SAT: W[p] is necessary; p += 1.
 *     LIMIT: W[p] is kept unproven; p += 1; the LIMIT-trial count goes up.
 *     UNSAT (a conflict at level 0): F alone is unsatisfiable.  W becomes empty
 *       and the chain ends: the instance ends UNSAT, its region closed by that
 *       query's empty record.
 *     FULL: the instance ends FULL with core_len 0.
 *   The end: the instance is ASSUMED with core W.  The region holds every lemma
 *   carried and learned by every query of the chain, in order, closed by one
 *   empty record (the last query's when that ended ASSUMED, else one written
 *   now); if that record does not fit the instance ends FULL.
 *   The first p literals survive a refinement: x became necessary because F
 *   with (W_then \ x) was satisfiable, every later W is a subset of W_then, so
 *   x is in every core drawn from a later W.  Every trial removes a literal of
 *   W or passes one, so there are at most |query 0's core| trials.
 *   The proof: every lemma of every query follows from F alone (the argument
 *   of the sound search).  The last ASSUMED query, whose core is W as a set,
 *   left a lemma list from which unit propagation over F, the lemmas and W's
 *   units reaches the empty clause, and lemmas added after it only help.  So
 *   (F + W's unit clauses, the region's records) is a RUP refutation that
 *   satmi_cdcl_assume_pack_device and the refutation check and trim read
 *   unchanged.
 *   Minimal: when no trial ended LIMIT, F with W less any one literal is
 *   satisfiable; the SAT trials found those models, which are not returned.
 *   Outputs: status; row_len / row_lits (only query 0's SAT writes a row);
 *   core_len / core_lits (the final W; the words behind it, up to query 0's
 *   core length and core_stride, are 0; core_stride may be 0: the refinement
 *   does not read core_lits); carry_out (the non-empty records at the end).
 *   counters are summed over the chain's queries, the highest level being their
 *   maximum.  info is the final region's records and words, the closing record
 *   or the record that did not fit included, and the flags.  shrink_info,
 *   int64 [B x SATMI_CDCL_SHRINK_NWORDS]: the queries run (query 0 included),
 *   the SAT trials, the ASSUMED trials, the LIMIT trials (non-zero: minimality
 *   is not proven), the length of query 0's core (0 unless it ended ASSUMED), 0.
 *   time_limit_s bounds the instance's whole chain from its first query: every
 *   trial reached late ends LIMIT.
 *   d_work_lits, int32, two words per assumption: instance b owns
 *   [2 * assume_begin[b], 2 * assume_begin[b + 1]), only its wavefront touches
 *   them, and their contents on return are unspecified.
 * The host form is satmi_cdcl_carry_batch_host's with h_shrink_info [B x 6]
 * (not NULL): the same checks before any HIP call, the same workspace, the same
 * run-again from the input carry for the instances that ended FULL, the same
 * packs for the proof and the kept lemmas.
 */
#define SATMI_CDCL_SHRINK_NWORDS 6
int satmi_cdcl_shrink_batch_device(int num_instances, const int32_t *d_inst_clause_begin,
                                   const int32_t *d_clause_lit_begin, const int32_t *d_lits,
                                   const int32_t *d_inst_nvars, int max_vars, int max_clause_len,
                                   int64_t conflict_limit, double time_limit_s, int32_t *d_lemmas,
                                   const int64_t *d_lemma_begin, int32_t *d_status, int64_t *d_counters,
                                   int32_t *d_row_len, int32_t *d_row_lits, int stride, int64_t *d_info,
                                   const int32_t *d_assume_begin, const int32_t *d_assume_lits, int32_t *d_core_len,
                                   int32_t *d_core_lits, int core_stride, const int64_t *d_carry_in,
                                   int64_t *d_carry_out, int32_t *d_work_lits, int64_t *d_shrink_info, void *stream);
int satmi_cdcl_shrink_batch_host(int num_instances, const int32_t *h_inst_clause_begin,
                                 const int32_t *h_clause_lit_begin, const int32_t *h_lits,
                                 const int32_t *h_inst_nvars, int64_t conflict_limit, double time_limit_s,
                                 int64_t room_cap, int32_t *h_status, int64_t *h_counters, int32_t *h_row_len,
                                 int32_t *h_row_lits, int stride, int32_t *h_proof_inst_begin,
                                 int32_t *h_proof_clause_begin, int64_t proof_clause_cap, int32_t *h_proof_lits,
                                 int64_t proof_lit_cap, int64_t *h_info, int64_t *h_totals,
                                 const int32_t *h_assume_begin, const int32_t *h_assume_lits, int32_t *h_core_len,
                                 int32_t *h_core_lits, int core_stride, const int32_t *h_carry_inst_begin,
                                 const int32_t *h_carry_clause_begin, const int32_t *h_carry_lits,
                                 int32_t *h_kept_inst_begin, int32_t *h_kept_clause_begin, int64_t kept_clause_cap,
                                 int32_t *h_kept_lits, int64_t kept_lit_cap, int64_t *h_shrink_info);

/* Device-side span of the last DPLL launch on `stream`: enqueues (on that
 * stream, after the launch) a copy of two uint64 s_memrealtime ticks into
 * d_span: [0] = ~(first wave's start), [1] = last wave's end, so the launch
 * took (d_span[1] - ~d_span[0]) / satmi_wallclock_hz() seconds -- the kernel's
 * own duration even when launches on two streams overlap. */
int satmi_dpll_launch_span(void *stream, uint64_t *d_span);
int satmi_wallclock_hz(double *hz);

/* LDS bytes one wavefront needs for an instance of this size (0 = unsupported). */
uint64_t satmi_dpll_lds_bytes(int max_vars, int max_clauses, int max_lits);

/* Same for the clause-scan kernel (0 = the shape is not eligible for it). */
uint64_t satmi_dpll_scan_lds_bytes(int max_vars, int max_clauses, int max_lits, int max_clause_len);

/* Which DPLL kernel satmi_dpll_batch_* use (process-wide; default AUTO):
 *   AUTO     the incremental clause kernel where eligible, else the general kernel
 *            (its wide HBM-arena form when the batch exceeds the LDS layout)
 *   GENERAL  always the general (occurrence-list, clause-counter) kernel
 *   SCAN     the clause-scan kernel, every propagation round a full clause scan;
 *            an ineligible call fails with SATMI_ERR_ARG
 *   INC      the clause kernel with incremental rounds (only the clauses that lost
 *            a literal are read); an ineligible call fails with SATMI_ERR_ARG
 *   WIDE     the general kernel in its wide form (see SATMI_KERNEL_WIDE)
 * All give identical statuses, counters and models, but for one status: the
 * LDS form of the general kernel holds clauses of at most 255 literals, so under
 * a pinned GENERAL (or with max_clause_len = 0, unknown) an instance with a
 * longer clause whose batch fits the LDS layout gets SATMI_DPLL_TOO_LARGE, where
 * AUTO and WIDE solve it. */
#define SATMI_KERNEL_AUTO 0
#define SATMI_KERNEL_GENERAL 1
#define SATMI_KERNEL_SCAN 2
#define SATMI_KERNEL_INC 3
#define SATMI_KERNEL_WIDE 4   /* the general kernel with its image in a per-wave HBM arena (32-bit
                                 indices; clauses of at most 65,535 literals); AUTO takes it for batches
                                 beyond the LDS layout or with a clause of more than 255 literals */
int satmi_dpll_set_kernel(int policy);

/* Branch splitting in the clause kernels (process-wide; default on): once a
 * launch's instance queue drains, idle wavefronts take over the False branches
 * of open decisions of the searches still running (a search checks for idle
 * wavefronts every 16 nodes); the donor takes the helper's result when its
 * backtracking reaches the branch.  Statuses, counters and models are those of
 * the unsplit search (branches a sequential search would not have visited are
 * cancelled and count nothing).  Applies to SOUND-mode launches with
 * max_solutions == 1, no node limit and no time limit.
 *   enable          0 off; 1 auto (default): launches with at least one and
 *                   at most 8 instances per resident wavefront; 2 every
 *                   eligible launch
 *   helpers_per_cu  wavefronts per CU that stay as helpers once the queue
 *                   drains (0 = default 1); the others exit, freeing their CU
 *                   slots for a launch queued on another stream */
int satmi_dpll_set_split(int enable, int helpers_per_cu);

/* Nodes (recursive calls) a search visits before it may donate a branch
 * (process-wide; < 0 = default 256, 0 = from its first donation check).  Short
 * searches never split: their subtrees cost a helper more to restage than to
 * search. */
int satmi_dpll_set_split_warmup(int nodes);

/* Branch-splitting statistics of the last DPLL launch on `stream` (waits for
 * the stream): out[0..6] = donations, helper tickets, subtrees run by helpers,
 * donations taken back by their donors, waves that registered as helpers,
 * searches handed to a helper (a donor that reaches a branch its helper is
 * still searching passes it the rest of its search instead of waiting; until
 * r06 this entry was the donors' waiting ticks), root instances finished.  All zero
 * (out[6] = 0) when that launch did not split. */
int satmi_dpll_split_stats(void *stream, int64_t *out);

/* Wave ticks (satmi_wallclock_hz) that the waves of the last DPLL launch on
 * `stream` spent inside searches, summed over the launch's waves, if that
 * launch split (else 0; waits for the stream).  Divided by the launch's waves
 * and its span (satmi_dpll_launch_span) it is the launch's wave utilisation,
 * measured per wave -- independent of how a split search's rows collect their
 * helpers' ticks. */
int satmi_dpll_split_busy(void *stream, int64_t *busy_ticks);

/* The launch satmi_dpll_batch_device would make for this batch shape under the
 * current policy: *kernel = SATMI_KERNEL_SCAN, _INC, _GENERAL or _WIDE, LDS
 * bytes per wavefront, and wavefronts resident per CU (LDS and registers). */
int satmi_dpll_plan(int max_vars, int max_clauses, int max_lits, int max_clause_len, int mode, int has_init,
                    int *kernel, uint64_t *lds_bytes_per_wave, int *waves_per_cu);

/* Which compiled form of the clause kernels a launch of this batch shape takes
 * (inc != 0: incremental rounds, the AUTO / INC policies; 0: the SCAN policy).
 * Launches nothing.  *K = literal slots of a clause word (3 or 5: 3-literal
 * formulas with more than 511 variables are promoted to 5); *lv_class = bytes
 * of the static literal-state array of the one-wave workgroup form (256, 512,
 * 1024 for K = 3; 512, 4096 for K = 5), 0 = the literal states lie in each
 * wave's dynamic LDS image (the 2- and 4-wave workgroup forms, and the fixed
 * form); *waves_per_wg = 1, 2 or 4; *fixed = 1 for the static-layout kernel of
 * the bench class (K = 3, <= 127 variables, <= 448 clauses, incremental).
 * SATMI_ERR_ARG when the clause kernels do not take the shape.  The choice
 * depends on the device's occupancy answer for each form, so it is a property
 * of the shape and the device. */
int satmi_dpll_scan_shape(int max_vars, int max_clauses, int max_clause_len, int inc, int *K, int *lv_class,
                          int *waves_per_wg, int *fixed);

#ifdef __cplusplus
}
#endif
#endif
