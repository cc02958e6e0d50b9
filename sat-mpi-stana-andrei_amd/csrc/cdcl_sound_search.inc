// cdcl_sound_search.inc -- the two kernels of cdcl_sound.hip that have an
// assumption-carrying form: the search and the pack's scan.  cdcl_sound.hip
// includes this text three times, with
//   CS_ASSUME            0: satmi_cdcl_sound_*'s kernels; 1: satmi_cdcl_assume_*'s
//   CS_CARRY             1 (with CS_ASSUME 1): satmi_cdcl_carry_batch_device's search
//                        kernel, whose instances start with carried lemmas in their
//                        regions (CsCarryArgs); it has a pack of its own, so the
//                        third inclusion defines no scan kernel
//   CS_SEARCH_KERNEL     the search kernel's name, CS_SEARCH_ARGS its argument struct
//   CS_PACK_SCAN_KERNEL  the pack scan kernel's name
// Kernel bodies, not functions inlined into two wrappers: with CS_ASSUME 0 the
// compiler sees the kernels as they were before the assumption-carrying form
// existed, token for token, and their machine code stays what it was
// (tools/isa_compare.py).  The lines of the other form are under #if CS_ASSUME:
// the instance carries an ordered list of assumption literals (CsAssumeArgs),
// read from the caller's arrays where they lie; level i <= k belongs to
// assumption i.  The lines of the carrying form are under #if CS_CARRY.
// A fourth inclusion with CS_SHRINK 1 (and CS_ASSUME, CS_CARRY 1; CsShrinkArgs)
// is satmi_cdcl_shrink_batch_device's kernel: the wave runs the instance's body
// as a chain of queries, query 0 as the carrying form does and then one trial
// per literal of the core, each under the core less that literal and carrying
// every lemma in the region.  Its lines are under #if CS_SHRINK, which is 0 in
// the three inclusions before it.
template <bool LONG>
__global__ void __launch_bounds__(256) CS_SEARCH_KERNEL(CS_SEARCH_ARGS A) {
    extern __shared__ __attribute__((aligned(16))) uint32_t cs_lds[];
    const int ln = lane_id(), wv = (int)threadIdx.x >> 6, wpg = (int)blockDim.x >> 6;
    const uint64_t lt = lanemask_lt();
    CsWave w;
    {
        uint32_t *base = cs_lds + (size_t)wv * A.region_words;
        w.reason = (int32_t *)base;
        w.seen = base + cs_reason_words(A.max_vars);
        w.level = (uint16_t *)(w.seen + cs_seen_words(A.max_vars));
        w.trail = w.level + 2u * cs_half_words(A.max_vars);
        w.act = w.trail + 2u * cs_half_words(A.max_vars);
        w.flags = (uint8_t *)(w.act + 2u * cs_half_words(A.max_vars));
    }
    w.lits = A.lits;
    const int64_t W = (int64_t)gridDim.x * wpg;
    for (int64_t b = (int64_t)blockIdx.x * wpg + wv; b < A.num_instances; b += W) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        const int c0 = A.icb[b];
        w.m = A.icb[b + 1] - c0;
        w.fclb = A.clb + c0;
        w.nv = A.nvars[b];
        const int64_t lb = A.lemma_begin[b];
        w.rec = A.lemmas + lb;
        w.room = max((int64_t)0, A.lemma_begin[b + 1] - lb);
        w.used = 0;
        w.trail_len = w.ncand = w.cur = 0;
        int status = CS_RUNNING;
        int64_t conflicts = 0, decisions = 0, props = 0, rounds = 0, learned = 0, learned_lits = 0, top = 0;
        int64_t records = 0, words = 0;   // what the search needed of its region, exact
        int row = 0;
        const int ls = w.fclb[0], le = w.fclb[w.m];
        // ---- the instance must fit the layout: no LDS index beyond the region
        {
            bool bad = false;
            for (int j = ls + ln; j < le; j += 64) bad |= cs_var(A.lits[j]) - 1u >= (uint32_t)max(w.nv, 0);
            if (w.nv < 0 || (uint32_t)w.nv > A.max_vars || __ballot(bad) != 0ull) status = SATMI_CDCL_SOUND_TOO_LARGE;
        }
#if CS_ASSUME
        // ---- the assumptions: at most MAX_VARS of them (levels stay below 2^16), over the instance's variables
        const int32_t *assume = A.assume_lits + A.assume_begin[b];
        int na = A.assume_begin[b + 1] - A.assume_begin[b], core = 0;
        {
            if (na < 0 || na > SATMI_CDCL_SOUND_MAX_VARS) {
                na = 0;
                status = SATMI_CDCL_SOUND_TOO_LARGE;
            }
            bool bad = false;
            for (int i = ln; i < na; i += 64) bad |= cs_var(assume[i]) - 1u >= (uint32_t)max(w.nv, 0);
            if (__ballot(bad) != 0ull) status = SATMI_CDCL_SOUND_TOO_LARGE;
        }
#endif
#if CS_CARRY
        // ---- the carried lemmas: carry_in[b] = (records, words) that lie in the region already
        int64_t cin_r = 0, cin_w = 0;
        bool bad_carry = false;
        if (A.carry_in) {
            cin_r = A.carry_in[2 * b];
            cin_w = A.carry_in[2 * b + 1];
        }
#endif
#if CS_SHRINK
        // ---- the chain: query 0 under the assumptions as given, then trials under W less W[p].
        // The instance's scratch: W in its first na0 words; behind them the trial list while a
        // trial searches, and the core of a final analysis as it is collected (the list is
        // dead by then).  Every query but the first re-walks the region as its carry.
        const int na0 = na;
        int32_t *const wl = A.work_lits + 2 * (int64_t)A.assume_begin[b], *const tl = wl + na0;
        int nw = 0, wp = 0, core0 = 0, nq = 0, n_sat = 0, n_assumed = 0, n_limit = 0;
        int64_t s_conflicts = 0, s_decisions = 0, s_props = 0, s_rounds = 0, s_learned = 0, s_learned_lits = 0, s_top = 0;
        for (int q = 0; q <= na0; ++q) {   // (a trial drops a literal of W or passes one: at most |W| <= na0 of them)
        if (q > 0) {
            // the trial list; the carry is what lies in the region without its closing record
            for (int j = ln; j < nw - 1; j += 64) tl[j] = wl[j + (j >= wp ? 1 : 0)];
            assume = tl;
            na = nw - 1;
            cin_r += learned;
            cin_w = w.used - (status == SATMI_CDCL_SOUND_ASSUMED ? 1 : 0);
            status = CS_RUNNING;
            conflicts = decisions = props = rounds = learned = learned_lits = top = 0;
            w.trail_len = w.ncand = w.cur = 0;
            core = 0;
            wave_sync();
        }
#endif
        if (status == CS_RUNNING) {
            for (int v = ln; v <= w.nv; v += 64) {
                w.reason[v] = CS_NONE;
                w.level[v] = 0;
                w.act[v] = 0;
                w.flags[v] = 0;
            }
            for (int t = ln; t < (int)cs_seen_words((uint32_t)w.nv); t += 64) w.seen[t] = 0u;
            wave_sync();
            for (int j = ls + ln; j < le; j += 64) w.flags[cs_var(A.lits[j])] = 8u;   // occurs (every lane the same byte value)
#if CS_ASSUME
            for (int i = ln; i < na; i += 64) w.flags[cs_var(assume[i])] = 8u;   // a variable of the assumptions occurs too
#endif
            wave_sync();
        }
#if CS_CARRY
        if (status == CS_RUNNING) {
            // The chain must hold `cin_r` records of at least one literal each, over the
            // instance's variables, and end on word `cin_w` exactly; codes m + offset stay
            // below 2^31.  One header per step, the lanes over its literals, which occur.
            bad_carry = cin_r < 0 || cin_w < 0 || cin_w > w.room || (int64_t)w.m + cin_w > (int64_t)INT32_MAX;
            int64_t p = 0, k = 0;
            bool lbad = false;
            for (; !bad_carry && k < cin_r && p < cin_w; ++k) {
                const int len = uniform_i32(w.rec[p]);
                if (len < 1 || (int64_t)len > cin_w - p - 1) {
                    bad_carry = true;
                    break;
                }
                for (int j = ln; j < len; j += 64) {
                    const uint32_t v = cs_var(w.rec[p + 1 + j]);
                    if (v - 1u >= (uint32_t)w.nv) lbad = true;
                    else w.flags[v] = 8u;
                }
                p += 1 + (int64_t)len;
            }
            bad_carry = bad_carry || k != cin_r || p != cin_w || __ballot(lbad) != 0ull;
            wave_sync();
            if (bad_carry) {
                status = SATMI_CDCL_SOUND_TOO_LARGE;
            } else {
                w.used = cin_w;
                records = cin_r;
                words = cin_w;
            }
        }
#endif
        // Every pass of the loop ends the instance, learns a clause (two words of
        // the region at least) or decides (at most nv decisions between conflicts).
#if CS_ASSUME   // (or opens an assumption's level: at most na between conflicts)
        const uint64_t pass_cap = ((uint64_t)w.room / 2u + 2u) * ((uint64_t)max(w.nv, 0) + 2u + (uint64_t)na);
#else
        const uint64_t pass_cap = ((uint64_t)w.room / 2u + 2u) * ((uint64_t)max(w.nv, 0) + 2u);
#endif
        for (uint64_t pass = 0; status == CS_RUNNING && pass < pass_cap; ++pass) {
            // ---- unit propagation in rounds, to a conflict or the fixpoint
            int confl = -1;
            for (int r = 0; r <= w.nv && confl < 0; ++r) {
                ++rounds;
                w.ncand = 0;
                confl = LONG ? cs_scan_long(w) : cs_scan_short(w);
                if (confl < 0) confl = cs_scan_learned(w);
                if (confl >= 0) {   // nothing is implied in this round
                    for (int i = ln; i < w.ncand; i += 64) w.reason[w.trail[w.trail_len + i] & 0x7FFFu] = CS_NONE;
                    w.ncand = 0;
                    wave_sync();
                    break;
                }
                if (w.ncand == 0) break;   // the fixpoint
                for (int i = ln; i < w.ncand; i += 64) {
                    const uint16_t e = w.trail[w.trail_len + i];
                    const uint32_t v = e & 0x7FFFu;
                    w.flags[v] = (uint8_t)((w.flags[v] & 12u) | ((e & 0x8000u) ? 2u : 1u));
                    w.level[v] = (uint16_t)w.cur;
                }
                w.trail_len += w.ncand;
                props += w.ncand;
                wave_sync();
            }
            const bool late = A.time_limit_ticks && __builtin_amdgcn_s_memrealtime() - t0 > A.time_limit_ticks;
            if (confl >= 0) {
                ++conflicts;
                if (w.cur == 0) {   // UNSAT: the empty clause closes the proof
                    ++records;
                    ++words;
                    if (w.used + 1 <= w.room) {
                        if (ln == 0) w.rec[w.used] = 0;
                        ++w.used;
                        status = SATMI_CDCL_SOUND_UNSAT;
                    } else {
                        status = SATMI_CDCL_SOUND_FULL;
                    }
                    break;
                }
                if ((A.conflict_limit > 0 && conflicts >= A.conflict_limit) || late) {
                    status = SATMI_CDCL_SOUND_LIMIT;
                    break;
                }
                // ---- first-UIP analysis, backwards over the trail
                int counter = 0, nlow = 0, idx = w.trail_len - 1;
                uint32_t pvar = 0;
                uint16_t pe = 0;
                int code = confl;
                bool broken = false;
                for (int step = 0; step <= w.trail_len; ++step) {
                    int len;
                    const int32_t *p = cs_clause(w, code, &len);
                    for (int j0 = 0; j0 < len; j0 += 64) {
                        const int j = j0 + ln;
                        bool at_cur = false, low = false;
                        if (j < len) {
                            const uint32_t v = cs_var(p[j]);
                            const int lv = w.level[v];
                            if (v != pvar && lv > 0) {
                                const uint32_t bit = 1u << (v & 31u);
                                if (!(atomicOr(&w.seen[v >> 5], bit) & bit)) {   // this lane marked it
                                    at_cur = lv == w.cur;
                                    low = !at_cur;
                                }
                            }
                        }
                        counter += __popcll(__ballot(at_cur));
                        nlow += __popcll(__ballot(low));
                    }
                    wave_sync();
                    // the next marked literal down the trail
                    bool found = false;
                    for (; idx >= 0 && !found;) {
                        const int i = idx - ln;
                        const uint64_t sm = __ballot(i >= 0 && cs_seen(w, w.trail[i] & 0x7FFFu));
                        if (sm) {
                            idx -= (int)__builtin_ctzll(sm);
                            found = true;
                        } else {
                            idx -= 64;
                        }
                    }
                    if (!found) {
                        broken = true;
                        break;
                    }
                    pe = (uint16_t)uniform_i32(w.trail[idx]);
                    pvar = pe & 0x7FFFu;
                    if (ln == 0) atomicAnd(&w.seen[pvar >> 5], ~(1u << (pvar & 31u)));
                    wave_sync();
                    --idx;
                    --counter;
                    if (counter <= 0) break;
                    code = uniform_i32(w.reason[pvar]);
                    if (code < 0 || code == CS_NONE) {   // a decision with marks above it: never by the rule
                        broken = true;
                        break;
                    }
                }
                if (broken || counter != 0) {
                    status = SATMI_CDCL_SOUND_LIMIT;
                    break;
                }
                // ---- the learned clause: the asserting literal, then the others down the trail
                const int len = 1 + nlow;
                const int64_t need = 1 + (int64_t)len;
                ++records;
                words += need;
                if (w.used + need > w.room || (int64_t)w.m + w.used + need > (int64_t)INT32_MAX) {
                    status = SATMI_CDCL_SOUND_FULL;   // nothing of the record is written
                    break;
                }
                int32_t *rp = w.rec + w.used;
                if (ln == 0) {
                    rp[0] = len;
                    rp[1] = -cs_dec(pe);
                    ++w.act[pvar];
                }
                int k = 0, bj = 0;
                for (; idx >= 0 && k < nlow; idx -= 64) {
                    const int i = idx - ln;
                    bool s = false;
                    uint16_t e = 0;
                    int lv = 0;
                    if (i >= 0) {
                        e = w.trail[i];
                        const uint32_t v = e & 0x7FFFu;
                        s = cs_seen(w, v);
                        lv = w.level[v];
                    }
                    const uint64_t sm = __ballot(s);
                    if (sm && k == 0) bj = __builtin_amdgcn_readlane(lv, (int)__builtin_ctzll(sm));
                    if (s) {
                        const uint32_t v = e & 0x7FFFu;
                        const int at = k + __popcll(sm & lt);
                        atomicAnd(&w.seen[v >> 5], ~(1u << (v & 31u)));
                        if (at < nlow) rp[2 + at] = -cs_dec(e);   // (every mark is on the trail once: always so)
                        ++w.act[v];
                    }
                    k += __popcll(sm);
                }
                w.used += need;
                ++learned;
                learned_lits += len;
                // ---- backjump: the trail's levels ascend, so what stays is a prefix
                int keep_n = 0;
                for (int i0 = 0; i0 < w.trail_len; i0 += 64) {
                    const int i = i0 + ln;
                    bool keep = false;
                    if (i < w.trail_len) {
                        const uint32_t v = w.trail[i] & 0x7FFFu;
                        keep = w.level[v] <= bj;
                        if (!keep) {
                            const uint32_t f = w.flags[v];
                            w.flags[v] = (uint8_t)((f & 8u) | ((f & 3u) == 1u ? 4u : 0u));   // unassigned, its phase saved
                            w.reason[v] = CS_NONE;
                        }
                    }
                    keep_n += __popcll(__ballot(keep));
                }
                w.trail_len = keep_n;
                w.cur = bj;
                if ((conflicts & 255) == 0)
                    for (int v = 1 + ln; v <= w.nv; v += 64) w.act[v] >>= 1;
                wave_sync();
                continue;
            }
#if CS_ASSUME
            {
                if (w.cur < na) {   // ---- the next assumption's level
                    const int32_t a = uniform_i32(assume[w.cur]);
                    const uint32_t av = cs_var(a);
                    const uint32_t st = uniform_u32(cs_val(w, a));
                    if (st == 2u) {   // false: UNSAT under the assumptions; the empty clause closes the proof
                        ++records;
                        ++words;
                        if (w.used + 1 > w.room) {
                            status = SATMI_CDCL_SOUND_FULL;
                            break;
                        }
                        if (ln == 0) w.rec[w.used] = 0;
                        ++w.used;
                        // the final analysis: the assumptions `a` was refuted from, down the trail
                        int32_t *cp = A.core_lits + b * (int64_t)A.core_stride;
                        if (ln == 0) {
                            if (A.core_stride > 0) cp[0] = a;
#if CS_SHRINK
                            tl[0] = a;   // (na0 >= 1 here: an assumption was read)
#endif
                            if (w.level[av] > 0) atomicOr(&w.seen[av >> 5], 1u << (av & 31u));
                        }
                        core = 1;
                        wave_sync();
                        int idx = w.trail_len - 1;
                        for (int step = 0; step < w.trail_len && idx >= 0; ++step) {
                            bool found = false;   // the next marked literal down the trail
                            for (; idx >= 0 && !found;) {
                                const int i = idx - ln;
                                const uint64_t sm = __ballot(i >= 0 && cs_seen(w, w.trail[i] & 0x7FFFu));
                                if (sm) {
                                    idx -= (int)__builtin_ctzll(sm);
                                    found = true;
                                } else {
                                    idx -= 64;
                                }
                            }
                            if (!found) break;
                            const uint16_t pe = (uint16_t)uniform_i32(w.trail[idx]);
                            const uint32_t pvar = pe & 0x7FFFu;
                            const int code = uniform_i32(w.reason[pvar]);
                            if (ln == 0) atomicAnd(&w.seen[pvar >> 5], ~(1u << (pvar & 31u)));
                            --idx;
                            if (code < 0) {   // no reason: at these levels an assumption
                                if (ln == 0 && core < A.core_stride) cp[core] = cs_dec(pe);
#if CS_SHRINK
                                if (ln == 0 && core < na) tl[core] = cs_dec(pe);   // (one per level below this one: always so)
#endif
                                ++core;
                            } else if (code != CS_NONE) {   // the others of its reason, above level 0
                                int len;
                                const int32_t *p = cs_clause(w, code, &len);
                                for (int j = ln; j < len; j += 64) {
                                    const uint32_t v = cs_var(p[j]);
                                    if (v != pvar && w.level[v] > 0) atomicOr(&w.seen[v >> 5], 1u << (v & 31u));
                                }
                            }
                            wave_sync();
                        }
                        status = SATMI_CDCL_SOUND_ASSUMED;
                        break;
                    }
                    if (late) {
                        status = SATMI_CDCL_SOUND_LIMIT;
                        break;
                    }
                    ++w.cur;   // its level: empty if it holds already, and never a decision
                    top = max(top, (int64_t)w.cur);
                    if (st == 0u) {
                        if (ln == 0) {
                            w.flags[av] = (uint8_t)((w.flags[av] & 12u) | (a > 0 ? 1u : 2u));
                            w.level[av] = (uint16_t)w.cur;
                            w.reason[av] = -1;
                            w.trail[w.trail_len] = cs_enc(a);
                        }
                        ++w.trail_len;
                        wave_sync();
                    }
                    continue;   // propagation follows, with its own round
                }
            }
#endif
            // ---- decide: the unassigned variable of the formula with the highest activity, the lowest id on a tie
            uint32_t best = 0;
            for (int v0 = 1; v0 <= w.nv; v0 += 64) {
                const int v = v0 + ln;
                if (v <= w.nv) {
                    const uint32_t f = w.flags[v];
                    if ((f & 8u) && !(f & 3u)) best = max(best, ((uint32_t)w.act[v] << 15) | (uint32_t)(32767 - v));
                }
            }
            best = wave_max_u32(best);
            if (best == 0u) {   // SAT: every variable of the formula is assigned
#if CS_SHRINK
                if (q > 0) {   // a trial's model is not returned
                    status = SATMI_CDCL_SOUND_SAT;
                    break;
                }
#endif
                int k = 0;
                for (int v0 = 1; v0 <= w.nv; v0 += 64) {
                    const int v = v0 + ln;
                    const uint32_t f = v <= w.nv ? w.flags[v] : 0u;
                    const bool occ = (f & 8u) != 0u;
                    const uint64_t om = __ballot(occ);
                    const int at = k + __popcll(om & lt);
                    if (occ && at < A.stride) A.row_lits[b * A.stride + at] = (f & 3u) == 1u ? v : -v;
                    k += __popcll(om);
                }
                row = k;
                status = SATMI_CDCL_SOUND_SAT;
                break;
            }
            if (late) {
                status = SATMI_CDCL_SOUND_LIMIT;
                break;
            }
            {
                const uint32_t v = 32767u - (best & 32767u);
                ++w.cur;
                ++decisions;
                top = max(top, (int64_t)w.cur);
                if (ln == 0) {
                    const uint32_t f = w.flags[v];
                    w.flags[v] = (uint8_t)(f | ((f & 4u) ? 1u : 2u));
                    w.level[v] = (uint16_t)w.cur;
                    w.reason[v] = -1;
                    w.trail[w.trail_len] = (uint16_t)(v | ((f & 4u) ? 0u : 0x8000u));
                }
                ++w.trail_len;
                wave_sync();
            }
        }
        if (status == CS_RUNNING) status = SATMI_CDCL_SOUND_LIMIT;   // the pass bound (never by the rule)
#if CS_SHRINK
        ++nq;
        s_conflicts += conflicts;
        s_decisions += decisions;
        s_props += props;
        s_rounds += rounds;
        s_learned += learned;
        s_learned_lits += learned_lits;
        s_top = max(s_top, top);
        wave_sync();   // lane 0's core words, before the lanes read them
        if (status == SATMI_CDCL_SOUND_ASSUMED) {
            // Query 0's core is W in the order reported.  A trial's core comes out the
            // refuted assumption first and then by descending level, which is the trial
            // list's order backwards: W is those literals turned round, still in W's order.
            core = min(core, na);   // (na0 at query 0, nw - 1 after: the words collected)
            for (int j = ln; j < core; j += 64) wl[j] = tl[q == 0 ? j : core - 1 - j];
            nw = core;
            if (q == 0) core0 = core;
            else ++n_assumed;
            wave_sync();
        } else if (q > 0 && status == SATMI_CDCL_SOUND_SAT) {
            ++n_sat;
            ++wp;
        } else if (q > 0 && status == SATMI_CDCL_SOUND_LIMIT) {
            ++n_limit;
            ++wp;
        } else {   // query 0 ended otherwise; a trial refuted F alone or filled the region
            break;
        }
        if (wp >= nw) break;
        }
        if (nq > 1 && (status == SATMI_CDCL_SOUND_SAT || status == SATMI_CDCL_SOUND_LIMIT || status == SATMI_CDCL_SOUND_ASSUMED)) {
            // ---- the end: ASSUMED with core W, the region closed by one empty record
            if (status != SATMI_CDCL_SOUND_ASSUMED) {
                ++records;
                ++words;
                if (w.used + 1 <= w.room) {
                    if (ln == 0) w.rec[w.used] = 0;
                    ++w.used;
                    status = SATMI_CDCL_SOUND_ASSUMED;
                } else {
                    status = SATMI_CDCL_SOUND_FULL;
                }
            }
            core = nw;
            int32_t *cp = A.core_lits + b * (int64_t)A.core_stride;
            for (int j = ln; j < min(core0, A.core_stride); j += 64) cp[j] = j < nw ? wl[j] : 0;   // (0 behind W, over query 0's core)
        }
#endif
        const bool trunc = status == SATMI_CDCL_SOUND_FULL;
        if (ln == 0) {
            A.status[b] = status;
            A.row_len[b] = row;
#if CS_ASSUME
            A.core_len[b] = status == SATMI_CDCL_SOUND_ASSUMED ? core : 0;
#endif
#if CS_CARRY
            // the non-empty records in the region: the carried ones and those learned and
            // written, without the closing record; a refused instance's input, or none of a bad carry
            const bool ran = status != SATMI_CDCL_SOUND_TOO_LARGE;
            const bool closed = status == SATMI_CDCL_SOUND_UNSAT || status == SATMI_CDCL_SOUND_ASSUMED;
            A.carry_out[2 * b] = bad_carry ? 0 : ran ? cin_r + learned : cin_r;
            A.carry_out[2 * b + 1] = bad_carry ? 0 : ran ? w.used - (closed ? 1 : 0) : cin_w;
#endif
        }
#if CS_SHRINK
        if (ln < SATMI_CDCL_SHRINK_NWORDS)
            A.shrink_info[b * SATMI_CDCL_SHRINK_NWORDS + ln] = ln == 0   ? nq
                                                               : ln == 1 ? n_sat
                                                               : ln == 2 ? n_assumed
                                                               : ln == 3 ? n_limit
                                                               : ln == 4 ? core0
                                                                         : 0;
        conflicts = s_conflicts;   // the counters of the chain
        decisions = s_decisions;
        props = s_props;
        rounds = s_rounds;
        learned = s_learned;
        learned_lits = s_learned_lits;
        top = s_top;
#endif
        if (ln < SATMI_CDCL_SOUND_NCOUNTERS)
            A.counters[b * SATMI_CDCL_SOUND_NCOUNTERS + ln] = ln == 0   ? conflicts
                                                              : ln == 1 ? decisions
                                                              : ln == 2 ? props
                                                              : ln == 3 ? rounds
                                                              : ln == 4 ? learned
                                                              : ln == 5 ? learned_lits
                                                              : ln == 6 ? top
                                                                        : 0;
        if (ln < SATMI_CDCL_SOUND_NWORDS)
            A.info[b * SATMI_CDCL_SOUND_NWORDS + ln] = ln == 0   ? records
                                                       : ln == 1 ? words
#if CS_CARRY
                                                       : ln == 2 ? (trunc ? SATMI_CDCL_SOUND_TRUNCATED : 0) |
                                                                       (bad_carry ? SATMI_CDCL_SOUND_BAD_CARRY : 0)
#else
                                                       : ln == 2 ? (trunc ? SATMI_CDCL_SOUND_TRUNCATED : 0)
#endif
                                                                 : 0;
        wave_sync();
    }
}

#if !CS_CARRY
// One wavefront: the totals, whether they fit, and the offsets by an exclusive
// scan, 64 instances at a time.  Totals that do not fit leave every instance
// with no lemma, as dpll_proof.hip's pack does.
__global__ void __launch_bounds__(64) CS_PACK_SCAN_KERNEL(CsPack P) {
    constexpr bool ASSUMED = CS_ASSUME;
    const int ln = lane_id(), B = P.num_instances;
    int64_t sn = 0, sl = 0;
    for (int b = ln; b < B; b += 64) {
        int64_t n, l;
        cs_contribution<ASSUMED>(P, b, &n, &l);
        sn += n;
        sl += l;
    }
    const int64_t tn = __shfl(cs_incl_scan64(sn), 63, 64), tl = __shfl(cs_incl_scan64(sl), 63, 64);
    const bool fits = tn <= P.clause_cap && tl <= P.lit_cap && tn <= INT32_MAX - 1 && tl <= INT32_MAX;
    if (ln == 0) {
        P.totals[0] = tn;
        P.totals[1] = tl;
        P.pib[B] = fits ? (int32_t)tn : 0;
        P.pcb[fits ? tn : 0] = fits ? (int32_t)tl : 0;
    }
    int64_t cn = 0, cl = 0;
    for (int b0 = 0; b0 < B; b0 += 64) {
        const int b = b0 + ln;
        int64_t n = 0, l = 0;
        if (b < B) cs_contribution<ASSUMED>(P, b, &n, &l);
        const int64_t in = cs_incl_scan64(n), il = cs_incl_scan64(l);
        if (b < B) {
            P.pib[b] = fits ? (int32_t)(cn + in - n) : 0;
            P.info[(int64_t)b * SATMI_CDCL_SOUND_NWORDS + 3] = fits ? cl + il - l : 0;
        }
        cn += __shfl(in, 63, 64);
        cl += __shfl(il, 63, 64);
    }
}
#endif
