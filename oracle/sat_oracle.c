/*
 * sat_oracle.c -- CPU restatement of the reference's clause-set solvers.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the product path (sat-mpi-stana-andrei_amd/)
 * links, loads or calls this file.  It is used by tests/ as the checker, by
 * __graft_entry__.smoke() as the checker and by bench.py's cpu_baseline leg.
 *
 * Reference: /root/reference/"comparatie intre algoritmii de rezolvare a seturilor
 * de clauze.py" (called REF.py below).  Each function cites the lines it restates.
 *
 * This is a deliberately *literal* restatement: formulas are explicit clause
 * lists that are copied/filtered exactly like the Python lists in REF.py, the
 * recursion is real recursion, unit clauses are processed one at a time in the
 * order the reference processes them.  The GPU kernels use a very different
 * formulation (assignment-state bitmaps, time-stamped conflict detection, an
 * explicit trail stack), so agreement between the two is meaningful.
 *
 * oracle_dpll_paths runs the same search and also counts, in the terms of the
 * general DPLL kernel (csrc/dpll.hip), which of its code paths the formula
 * drives (DP_* below, named in oracle.py DPLL_PATHS): tests/dpll_paths.py holds
 * the formulas that reach each path, tests/test_dpll_paths.py proves they do.
 * The counters only read the search (clause ids, the assignment at a snapshot's
 * start); with c->P == NULL none of that code runs.
 *
 * Pinning: the JSON files in tests/golden hold outputs of the reference functions themselves
 * (run here by tests/golden/make_golden.py, with per-call counters observed via
 * sys.settrace); tests/test_oracle_golden.py checks this file against them.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ */
/* formula = list of clauses, clause = list of ints (REF.py:11-13)     */
/* ------------------------------------------------------------------ */
typedef struct {
    int nc;        /* number of clauses                 */
    int *len;      /* len[i]                            */
    int **cl;      /* cl[i] -> literals                 */
    int *pool;     /* owned literal storage             */
    int *id;       /* id[i] = index of the input clause cl[i] descends from (-1: a decision's
                      unit clause); read by the path counters only, never by the search */
} formula;

static formula *f_alloc(int nc, long nlits) {
    formula *f = (formula *)calloc(1, sizeof(formula));
    f->nc = 0;
    f->len = (int *)malloc(sizeof(int) * (size_t)(nc > 0 ? nc : 1));
    f->cl = (int **)malloc(sizeof(int *) * (size_t)(nc > 0 ? nc : 1));
    f->pool = (int *)malloc(sizeof(int) * (size_t)(nlits > 0 ? nlits : 1));
    f->id = (int *)malloc(sizeof(int) * (size_t)(nc > 0 ? nc : 1));
    return f;
}
static void f_free(formula *f) {
    if (!f) return;
    free(f->len); free(f->cl); free(f->pool); free(f->id); free(f);
}
static long f_nlits(const formula *f) {
    long s = 0;
    for (int i = 0; i < f->nc; i++) s += f->len[i];
    return s;
}
static formula *f_copy_append_unit(const formula *f, int unit_lit) {
    long nl = f_nlits(f);
    formula *g = f_alloc(f->nc + 1, nl + 1);
    int *p = g->pool;
    for (int i = 0; i < f->nc; i++) {
        memcpy(p, f->cl[i], sizeof(int) * (size_t)f->len[i]);
        g->cl[g->nc] = p; g->len[g->nc] = f->len[i]; g->id[g->nc] = f->id[i]; g->nc++;
        p += f->len[i];
    }
    p[0] = unit_lit;
    g->cl[g->nc] = p; g->len[g->nc] = 1; g->id[g->nc] = -1; g->nc++;
    return g;
}

/* ------------------------------------------------------------------ */
/* ordered assignment: Dict[int,bool] with insertion order (REF.py:14) */
/* ------------------------------------------------------------------ */
typedef struct {
    int n;               /* entries                          */
    int *order;          /* signed literal per entry, in insertion order */
    signed char *val;    /* val[var] = 0 unassigned, +1 True, -1 False   */
} assign_t;

typedef struct {
    int nvars;
    int mode;            /* 0 = REF semantics, 1 = SOUND (decisions as unit clauses) */
    int64_t max_solutions, node_limit;
    int stop;            /* 1 = max_solutions reached, 2 = node limit */
    int64_t nodes, decisions, unit_props, pure_assigns, conflicts, solutions;
    /* solution output */
    int32_t *sol_lits; int64_t sol_cap_lits, sol_used_lits;
    int64_t *sol_off; int64_t sol_cap, sol_stored;
    /* root assignment after the root's unit_propagate (dict mutated in place) */
    int32_t *root_assign; int *root_len; int root_done;
    struct dpaths *P;    /* path counters (oracle_dpll_paths), else NULL */
} dctx;

/* ------------------------------------------------------------------ */
/* Path counters: what csrc/dpll.hip does with this search.            */
/*                                                                     */
/* The kernel runs unit_propagate on *snapshots* of unit literals, 64  */
/* per wave step: the root's is the input's unit clauses, a SOUND      */
/* decision's is the decision literal alone, a later one the clauses   */
/* the last batch made unit (collect_units).  The reference's own      */
/* snapshot (REF.py:143) also holds the unit clauses it met before and */
/* could not drop -- their variable is assigned, with the same value,  */
/* by a caller's dict or a REF-mode decision, neither of which reduces */
/* the formula -- so an index here is the index in the kernel's list:  */
/* the reference's entries less those stale ones.  The kernel runs no  */
/* propagation for a REF-mode decision's child nor a pure literals'    */
/* child (nothing can become unit there); `model_mismatch` counts any  */
/* event that contradicts this account.                                */
/* ------------------------------------------------------------------ */
enum {
    DP_SNAPSHOT_LEN_MAX,          /* entries of a snapshot (propagate's k0 chunks)                     */
    DP_COLLECTED_SNAPSHOT_LEN_MAX,/* ... of one made by collect_units                                  */
    DP_STAMP_DROP_LEN_MAX,        /* ... of one that ends without an emptied clause (nu > 64: trail walk) */
    DP_MISMATCH_INDEX_MAX,        /* k of the unit that returns at REF.py:150 (-1: never)              */
    DP_EMPTIED_INDEX_MAX,         /* k of the unit whose reduction emptied a clause (-1: never)        */
    DP_UNDONE_AFTER_STOP_MAX,     /* variables assigned after that unit in its chunk: the cut's undo   */
    DP_CUT_ROUND_LEN_MAX,         /* assignments of the round when it is cut (the `keep` scan)         */
    DP_SAME_VAR_SAME_SIGN,        /* a claim loser: its variable is claimed earlier in the chunk       */
    DP_SAME_VAR_OPPOSITE_SIGN,    /* ... with the other sign: the clause is emptied at the winner's time */
    DP_SAME_VAR_EARLIER_CHUNK,    /* its variable was assigned by an earlier chunk of the snapshot     */
    DP_SKIP_ASSIGNED_EQUAL,       /* REF.py:152 `continue`: assigned before the snapshot, same value   */
    DP_EMPTY_CLAUSE_WITH_UNITS,   /* the input holds [] and a batch assigns: has_empty && mk           */
    DP_EMPTY_CLAUSE_NO_UNITS,     /* ... and a propagation assigns nothing                             */
    DP_EMPTY_CLAUSE_FIRST_INDEX_MAX, /* first_k of has_empty && mk (-1: never)                         */
    DP_OCC_SINGLE_LEN_MAX,        /* apply_lanes with one literal: its list + its negation's           */
    DP_FLAT_TOTAL_MAX,            /* apply_lanes with several: the flattened total                     */
    DP_FLAT_LIST_STRADDLES_WINDOW,/* a list that crosses a 64-slot window of the flattening (`carry`)  */
    DP_UNIT_CLAUSE_INDEX_MAX,     /* clause index of a collected unit (-1: never)                      */
    DP_CONFLICT_CLAUSES_MAX,      /* clauses of an instance whose propagation conflicts (clear_ubits)  */
    DP_PURE_COUNT_MAX,            /* pure literals of one node                                         */
    DP_PURE_FIRST_POS_MAX,        /* first position of a pure variable (posbits word / 64; -1: never)  */
    DP_BRANCH_VAR_MAX,            /* the largest decision variable                                     */
    DP_BRANCH_TIE_ACROSS_GROUPS,  /* maximal counts in two 64-variable groups of analyze               */
    DP_UNDO_LEN_MAX,              /* trail entries of one unassign_to                                  */
    DP_UNDO_NON_EFFECTIVE,        /* ... that are not effective (a REF-mode decision)                  */
    DP_INIT_OVERWRITE,            /* caller's dict: a key given twice                                  */
    DP_INIT_VAR_BEYOND_FORMULA,   /* ... a key above every variable of the formula                     */
    DP_INIT_MISMATCH,             /* a unit contradicts the caller's dict                              */
    DP_DECISION_MISMATCH,         /* ... a REF-mode decision                                           */
    DP_SOLS_PAST_CAP,             /* solutions counted beyond sol_cap                                  */
    DP_CLAUSE_LEN_MAX,            /* the longest input clause (Narrow::MAX_LEN = 255)                  */
    DP_MODEL_MISMATCH,            /* the search contradicts the account above                          */
    DP_NPATHS
};

typedef struct dpaths {
    int64_t v[DP_NPATHS];
    int nv, m, mode, has_empty;
    const int32_t *coff, *lits;   /* the input as the kernel stages it                          */
    int *occ;                     /* [2nv+2] occurrences of var*2 + negative in the input: the  */
                                  /* lengths of the kernel's static occurrence lists            */
    unsigned char *isinit;        /* [nv+1] variable of the caller's dict                       */
    int *claim;                   /* [nv+1] 1 + snapshot index that claimed the variable        */
    signed char *pre;             /* [nv+1] the assignment at the snapshot's start              */
    int *idstamp; int serial;     /* [m] serial of the last snapshot that held the clause       */
    int *ft; int depth;           /* [nv+2] trail length before each open decision              */
    int *klit, *kcl;              /* [m+2] the kernel's snapshot: literals, clause indices      */
    int *firstcl;                 /* [nv+1] reduced clause of a variable's first occurrence     */
} dpaths;

static void p_max(dpaths *P, int i, int64_t x) { if (x > P->v[i]) P->v[i] = x; }

/* apply_lanes: the effective literals of up to 64 lanes, in lane order */
static void p_apply(dpaths *P, const int *lits, int n) {
    int nz = 0, one = 0, straddle = 0;
    long total = 0;
    for (int i = 0; i < n; i++) {
        int v = lits[i] > 0 ? lits[i] : -lits[i];
        int len = P->occ[2 * v] + P->occ[2 * v + 1];
        if (len == 0) continue;
        nz++; one = len;
        if (total / 64 != (total + len - 1) / 64) straddle = 1;
        total += len;
    }
    if (nz == 1) p_max(P, DP_OCC_SINGLE_LEN_MAX, one);
    if (nz >= 2) {
        p_max(P, DP_FLAT_TOTAL_MAX, total);
        if (straddle) P->v[DP_FLAT_LIST_STRADDLES_WINDOW]++;
    }
}

/* unassign_to(lo, hi): apply_trail<UNDO> in 64-entry steps from lo, effective entries only.
 * In REF mode the entry at an open decision's trail length is that decision. */
static void p_undo(dpaths *P, const int *order, int lo, int hi) {
    int buf[64];
    if (hi <= lo) return;
    p_max(P, DP_UNDO_LEN_MAX, hi - lo);
    for (int w0 = lo; w0 < hi; w0 += 64) {
        int n = 0;
        for (int e = w0; e < hi && e < w0 + 64; e++) {
            int noneff = 0;
            if (P->mode == 0)
                for (int j = 0; j < P->depth; j++) if (P->ft[j] == e) noneff = 1;
            if (noneff) P->v[DP_UNDO_NON_EFFECTIVE]++;
            else buf[n++] = order[e];
        }
        p_apply(P, buf, n);
    }
}

/* a conflict or a leaf below an open decision: the kernel pops back to it */
static void p_backtrack(dpaths *P, const int *order, int n) {
    if (P->depth > 0) p_undo(P, order, P->ft[P->depth - 1], n);
}

/* One snapshot as propagate runs it.  stop_kind 0: processed to its end, 1: the
 * unit at stop_k emptied a clause, 2: the unit at stop_k mismatched. */
static void p_snapshot(dpaths *P, int nk, int collected, int stop_kind, int stop_k) {
    const int *K = P->klit;
    int buf[64], after[64];
    p_max(P, DP_SNAPSHOT_LEN_MAX, nk);
    if (collected) {
        p_max(P, DP_COLLECTED_SNAPSHOT_LEN_MAX, nk);
        for (int k = 0; k < nk; k++) p_max(P, DP_UNIT_CLAUSE_INDEX_MAX, P->kcl[k]);
    }
    if (stop_kind != 1) p_max(P, DP_STAMP_DROP_LEN_MAX, nk);
    if (stop_kind) p_max(P, DP_CONFLICT_CLAUSES_MAX, P->m);
    if (stop_kind == 1) {
        p_max(P, DP_EMPTIED_INDEX_MAX, stop_k);
        if (P->has_empty) { P->v[DP_EMPTY_CLAUSE_WITH_UNITS]++; p_max(P, DP_EMPTY_CLAUSE_FIRST_INDEX_MAX, stop_k); }
    }
    if (stop_kind == 2) {
        int v = K[stop_k] > 0 ? K[stop_k] : -K[stop_k];
        p_max(P, DP_MISMATCH_INDEX_MAX, stop_k);
        P->v[P->isinit[v] ? DP_INIT_MISMATCH : DP_DECISION_MISMATCH]++;
    }
    int assigned = 0, done = 0;
    for (int k0 = 0; k0 < nk && !done; k0 += 64) {
        const int ke = k0 + 64 < nk ? k0 + 64 : nk;
        int kmis = 0x7fffffff, n = 0, nafter = 0;
        for (int k = k0; k < ke; k++) {
            int v = K[k] > 0 ? K[k] : -K[k], val = K[k] > 0 ? 1 : -1;
            if (P->pre[v] && P->pre[v] != val) { kmis = k; break; }
        }
        for (int k = k0; k < ke; k++) {
            int v = K[k] > 0 ? K[k] : -K[k], val = K[k] > 0 ? 1 : -1;
            if (P->pre[v]) { if (P->pre[v] == val) P->v[DP_SKIP_ASSIGNED_EQUAL]++; continue; }
            const int j = P->claim[v] - 1;
            if (j >= 0 && j < k0) {      /* time-stamped by an earlier chunk: a different sign had stopped there */
                P->v[(K[j] > 0) == (K[k] > 0) ? DP_SAME_VAR_EARLIER_CHUNK : DP_MODEL_MISMATCH]++;
                continue;
            }
            if (k >= kmis) continue;     /* not claimable */
            if (j >= 0) { P->v[(K[j] > 0) == (K[k] > 0) ? DP_SAME_VAR_SAME_SIGN : DP_SAME_VAR_OPPOSITE_SIGN]++; continue; }
            P->claim[v] = k + 1;
            buf[n++] = K[k];
            if (stop_kind == 1 && k > stop_k) after[nafter++] = K[k];
        }
        p_apply(P, buf, n);
        assigned += n;
        if (stop_kind && stop_k >= k0 && stop_k < ke) {
            if (stop_kind == 1) {
                p_max(P, DP_UNDONE_AFTER_STOP_MAX, nafter);
                p_max(P, DP_CUT_ROUND_LEN_MAX, assigned);
                p_apply(P, after, nafter);            /* apply_trail<UNDO>(cut, trail_len): < 64 entries */
            } else if (kmis != stop_k) {
                P->v[DP_MODEL_MISMATCH]++;
            }
            done = 1;
        } else if (kmis != 0x7fffffff) {
            P->v[DP_MODEL_MISMATCH]++;                /* the kernel stops here, the reference went on */
            done = 1;
        }
    }
    if (stop_kind && !done) P->v[DP_MODEL_MISMATCH]++;
    for (int k = 0; k < nk; k++) P->claim[K[k] > 0 ? K[k] : -K[k]] = 0;
}

static assign_t *a_new(int nvars) {
    assign_t *a = (assign_t *)calloc(1, sizeof(assign_t));
    a->order = (int *)malloc(sizeof(int) * (size_t)(nvars + 1));
    a->val = (signed char *)calloc((size_t)nvars + 1, 1);
    return a;
}
static assign_t *a_copy(const assign_t *a, int nvars) {
    assign_t *b = a_new(nvars);
    b->n = a->n;
    memcpy(b->order, a->order, sizeof(int) * (size_t)a->n);
    memcpy(b->val, a->val, (size_t)nvars + 1);
    return b;
}
static void a_free(assign_t *a) {
    if (!a) return;
    free(a->order); free(a->val); free(a);
}
static void a_set(assign_t *a, int lit) {
    int v = lit > 0 ? lit : -lit;
    a->val[v] = lit > 0 ? 1 : -1;
    a->order[a->n++] = lit;
}

static void emit_solution(dctx *c, const assign_t *a) {
    c->solutions++;
    if (c->sol_off && c->sol_stored < c->sol_cap &&
        c->sol_used_lits + a->n <= c->sol_cap_lits) {
        memcpy(c->sol_lits + c->sol_used_lits, a->order, sizeof(int32_t) * (size_t)a->n);
        c->sol_used_lits += a->n;
        c->sol_stored++;
        c->sol_off[c->sol_stored] = c->sol_used_lits;
    }
    if (c->max_solutions > 0 && c->solutions >= c->max_solutions) c->stop = 1;
}

/* unit_propagate, REF.py:139-165.  Returns the (possibly new) formula, or NULL
 * on conflict.  `f_in` is never freed here; a returned formula != f_in is owned
 * by the caller.  `skip_first_count`: SOUND decision children do not count the
 * propagation of the decision literal itself as a unit propagation.
 * `kernel_runs` (path counters only): how the kernel runs this call -- 1: from
 * the input's unit clauses (the root), 2: from the decision literal alone (a
 * SOUND decision's child), 0: not at all. */
static formula *unit_propagate(dctx *c, const formula *f_in, assign_t *a, int skip_first_count, int kernel_runs) {
    const formula *f = f_in;
    formula *owned = NULL;
    int changed = 1;
    int *units = NULL; int ucap = 0;
    dpaths *P = c->P;
    int *kidx = NULL;        /* index of the reference's entry in the kernel's snapshot, -1: a stale entry */
    int round = 0, prev_serial = 0;
    while (changed) {
        changed = 0;
        /* unit_clauses = [c for c in f if len(c) == 1]   (REF.py:143) */
        int nu = 0, nk = 0;
        if (ucap < f->nc) {
            ucap = f->nc + 1; units = (int *)realloc(units, sizeof(int) * (size_t)ucap);
            if (P) kidx = (int *)realloc(kidx, sizeof(int) * (size_t)ucap);
        }
        for (int i = 0; i < f->nc; i++)
            if (f->len[i] == 1) {
                if (P) {
                    const int id = f->id[i];
                    const int in_kernel = !kernel_runs ? 0 : round == 0 ? (kernel_runs == 1 || id < 0)
                                                                        : (id >= 0 && P->idstamp[id] != prev_serial);
                    kidx[nu] = in_kernel ? nk : -1;
                    if (in_kernel) { P->klit[nk] = f->cl[i][0]; P->kcl[nk] = id; nk++; }
                }
                units[nu++] = f->cl[i][0];
            }
        if (P) {
            prev_serial = ++P->serial;
            for (int i = 0; i < f->nc; i++) if (f->len[i] == 1 && f->id[i] >= 0) P->idstamp[f->id[i]] = prev_serial;
            memcpy(P->pre, a->val, (size_t)P->nv + 1);
        }
        for (int k = 0; k < nu; k++) {
            int lit = units[k];
            int var = lit > 0 ? lit : -lit;
            int val = lit > 0 ? 1 : -1;
            if (a->val[var] != 0) {                      /* REF.py:149-152 */
                if (a->val[var] != val) {
                    if (P && kidx[k] < 0) P->v[DP_MODEL_MISMATCH]++;
                    else if (P) p_snapshot(P, nk, round > 0, 2, kidx[k]);
                    free(units); free(kidx); f_free(owned); return NULL;
                }
                continue;
            }
            if (P && kidx[k] < 0) P->v[DP_MODEL_MISMATCH]++;   /* a stale entry never assigns */
            a_set(a, lit);                               /* REF.py:154 */
            if (skip_first_count) skip_first_count = 0; else c->unit_props++;
            changed = 1;
            /* new_f (REF.py:156-164) */
            formula *g = f_alloc(f->nc, f_nlits(f));
            int *p = g->pool;
            for (int i = 0; i < f->nc; i++) {
                const int *ci = f->cl[i];
                int li = f->len[i], has = 0;
                for (int j = 0; j < li; j++) if (ci[j] == lit) { has = 1; break; }
                if (has) continue;
                int n = 0;
                for (int j = 0; j < li; j++) if (ci[j] != -lit) p[n++] = ci[j];
                if (n == 0) {
                    if (P && kidx[k] >= 0) p_snapshot(P, nk, round > 0, 1, kidx[k]);
                    f_free(g); free(units); free(kidx); f_free(owned); return NULL;
                }
                g->cl[g->nc] = p; g->len[g->nc] = n; g->id[g->nc] = f->id[i]; g->nc++;
                p += n;
            }
            f_free(owned);
            owned = g; f = g;
        }
        if (P && kernel_runs) p_snapshot(P, nk, round > 0, 0, 0);
        round++;
    }
    free(units); free(kidx);
    if (P && kernel_runs && P->has_empty) P->v[DP_EMPTY_CLAUSE_NO_UNITS]++;
    if (!owned) {   /* unchanged: hand back a private copy to keep ownership simple */
        formula *g = f_alloc(f->nc, f_nlits(f));
        int *p = g->pool;
        for (int i = 0; i < f->nc; i++) {
            memcpy(p, f->cl[i], sizeof(int) * (size_t)f->len[i]);
            g->cl[g->nc] = p; g->len[g->nc] = f->len[i]; g->id[g->nc] = f->id[i]; g->nc++; p += f->len[i];
        }
        owned = g;
    }
    return owned;
}

/* first_position: where the variable of `lit` first occurs in the reduced formula,
 * as a literal index of the input (the key of the kernel's posbits). */
static int64_t p_first_position(const dpaths *P, const formula *f, int lit) {
    const int var = lit > 0 ? lit : -lit, id = f->id[P->firstcl[var]];
    if (id < 0) return -1;
    for (int j = P->coff[id]; j < P->coff[id + 1]; j++)
        if (P->lits[j] == var || P->lits[j] == -var) return j;
    return -1;
}

/* dpll_optimized, REF.py:133-214 (mode 0).  Mode 1 (SOUND) replaces the branch
 * of REF.py:210-213 by a recursion on `formula + [[lit]]` with the assignment
 * copied *without* var, i.e. the decision is applied to the formula as a unit
 * clause and is propagated by REF.py's own unit_propagate. */
static void dpll_node(dctx *c, const formula *F, assign_t *a, int is_decision_child, int is_root) {
    if (c->stop) return;
    c->nodes++;
    if (c->node_limit > 0 && c->nodes > c->node_limit) { c->stop = 2; return; }

    dpaths *P = c->P;
    formula *f = unit_propagate(c, F, a, is_decision_child && c->mode == 1,
                                is_root ? 1 : (is_decision_child && c->mode == 1) ? 2 : 0);
    if (is_root && c->root_assign) {
        memcpy(c->root_assign, a->order, sizeof(int32_t) * (size_t)a->n);
        *c->root_len = a->n;
    }
    if (!f) { c->conflicts++; if (P) p_backtrack(P, a->order, a->n); return; }   /* REF.py:168-169 */
    if (f->nc == 0) {                                    /* REF.py:170-171 */
        emit_solution(c, a);
        if (P && !c->stop) p_backtrack(P, a->order, a->n);
        f_free(f);
        return;
    }

    int nv = c->nvars;
    /* literal_sign = defaultdict(set), REF.py:174-179 (dict order = first occurrence) */
    int *order = (int *)malloc(sizeof(int) * (size_t)(nv + 1));
    unsigned char *signs = (unsigned char *)calloc((size_t)nv + 1, 1);   /* bit0 True, bit1 False */
    int *cnt = (int *)calloc((size_t)nv + 1, sizeof(int));
    int norder = 0;
    for (int i = 0; i < f->nc; i++)
        for (int j = 0; j < f->len[i]; j++) {
            int lit = f->cl[i][j], var = lit > 0 ? lit : -lit;
            if (a->val[var] == 0) {
                if (signs[var] == 0) { order[norder++] = var; if (P) P->firstcl[var] = i; }
                signs[var] |= (lit > 0) ? 1 : 2;
                cnt[var]++;
            }
        }
    /* pure_literals, REF.py:181-184 */
    int *pure = (int *)malloc(sizeof(int) * (size_t)(nv + 1));
    int npure = 0;
    for (int k = 0; k < norder; k++) {
        int var = order[k];
        if (signs[var] == 1) pure[npure++] = var;
        else if (signs[var] == 2) pure[npure++] = -var;
    }
    if (npure > 0) {                                     /* REF.py:186-195 */
        assign_t *na = a_copy(a, nv);
        for (int k = 0; k < npure; k++) a_set(na, pure[k]);
        c->pure_assigns += npure;
        if (P) {   /* assign_pures + apply_trail over the new entries, 64 at a time */
            p_max(P, DP_PURE_COUNT_MAX, npure);
            for (int k = 0; k < npure; k++) p_max(P, DP_PURE_FIRST_POS_MAX, p_first_position(P, f, pure[k]));
            for (int k0 = 0; k0 < npure; k0 += 64) p_apply(P, pure + k0, npure - k0 < 64 ? npure - k0 : 64);
        }
        /* membership tests against the pure list */
        signed char *ispure = (signed char *)calloc((size_t)nv + 1, 1);
        for (int k = 0; k < npure; k++) ispure[pure[k] > 0 ? pure[k] : -pure[k]] = pure[k] > 0 ? 1 : -1;
        formula *g = f_alloc(f->nc, f_nlits(f));
        int *p = g->pool;
        for (int i = 0; i < f->nc; i++) {
            int drop = 0;
            for (int j = 0; j < f->len[i] && !drop; j++) {
                int lit = f->cl[i][j], var = lit > 0 ? lit : -lit;
                if (ispure[var] == (lit > 0 ? 1 : -1)) drop = 1;      /* lit in pure_literals */
            }
            if (drop) continue;
            int n = 0;
            for (int j = 0; j < f->len[i]; j++) {
                int lit = f->cl[i][j], var = lit > 0 ? lit : -lit;
                if (ispure[var] == (lit > 0 ? -1 : 1)) continue;       /* -lit in pure_literals */
                p[n++] = lit;
            }
            g->cl[g->nc] = p; g->len[g->nc] = n; g->id[g->nc] = f->id[i]; g->nc++; p += n;
        }
        free(ispure);
        free(order); free(signs); free(cnt); free(pure);
        f_free(f);
        dpll_node(c, g, na, 0, 0);
        f_free(g); a_free(na);
        return;
    }
    free(pure);
    /* var_counts + max(... key=count), REF.py:198-208: first maximal in dict order */
    if (norder == 0) {                                   /* REF.py:205-206 */
        emit_solution(c, a);
        if (P && !c->stop) p_backtrack(P, a->order, a->n);
        free(order); free(signs); free(cnt); f_free(f);
        return;
    }
    int best = order[0];
    for (int k = 1; k < norder; k++)
        if (cnt[order[k]] > cnt[best]) best = order[k];
    if (P) {
        int tie = 0;
        for (int k = 0; k < norder; k++)
            if (cnt[order[k]] == cnt[best] && (order[k] - 1) / 64 != (best - 1) / 64) tie = 1;
        P->v[DP_BRANCH_TIE_ACROSS_GROUPS] += tie;
        p_max(P, DP_BRANCH_VAR_MAX, best);
        P->ft[P->depth++] = a->n;                        /* the frame both branches run under */
    }
    free(order); free(signs); free(cnt);
    for (int t = 0; t < 2 && !c->stop; t++) {            /* for val in [True, False] */
        int lit = t == 0 ? best : -best;
        assign_t *na = a_copy(a, nv);
        c->decisions++;
        if (c->mode == 0) {
            a_set(na, lit);                               /* new_assignment[var] = val */
            dpll_node(c, f, na, 1, 0);
        } else {
            formula *g = f_copy_append_unit(f, lit);
            dpll_node(c, g, na, 1, 0);
            f_free(g);
        }
        a_free(na);
    }
    if (P) {   /* both branches done: the frame is popped, and the kernel unwinds to the one below */
        P->depth--;
        if (!c->stop) p_backtrack(P, a->order, a->n);
    }
    f_free(f);
}

typedef struct {
    int64_t nodes, decisions, unit_props, pure_assigns, conflicts, solutions;
} oracle_counters;

static int dpll_run(int nvars, int nclauses, const int32_t *clause_off, const int32_t *lits,
                int mode, int64_t max_solutions, int64_t node_limit,
                const int32_t *init_assign, int n_init,
                int32_t *sol_lits, int64_t sol_cap_lits, int64_t *sol_off, int64_t sol_cap,
                int32_t *root_assign, int *root_len, oracle_counters *ctr, int64_t *paths) {
    int nv = nvars;
    for (int i = 0; i < n_init; i++) { int v = init_assign[i] > 0 ? init_assign[i] : -init_assign[i]; if (v > nv) nv = v; }
    for (long i = 0; i < clause_off[nclauses]; i++) { int v = lits[i] > 0 ? lits[i] : -lits[i]; if (v > nv) nv = v; }
    dctx c; memset(&c, 0, sizeof(c));
    c.nvars = nv; c.mode = mode; c.max_solutions = max_solutions; c.node_limit = node_limit;
    c.sol_lits = sol_lits; c.sol_cap_lits = sol_cap_lits; c.sol_off = sol_off; c.sol_cap = sol_cap;
    if (sol_off) sol_off[0] = 0;
    c.root_assign = root_assign; c.root_len = root_len;
    if (root_len) *root_len = 0;
    dpaths PP;
    if (paths) {
        dpaths *P = &PP;
        memset(P, 0, sizeof(*P));
        P->v[DP_MISMATCH_INDEX_MAX] = P->v[DP_EMPTIED_INDEX_MAX] = P->v[DP_EMPTY_CLAUSE_FIRST_INDEX_MAX] = -1;
        P->v[DP_UNIT_CLAUSE_INDEX_MAX] = P->v[DP_PURE_FIRST_POS_MAX] = -1;
        P->nv = nv; P->m = nclauses; P->mode = mode; P->coff = clause_off; P->lits = lits;
        P->occ = (int *)calloc(2 * (size_t)nv + 2, sizeof(int));
        P->isinit = (unsigned char *)calloc((size_t)nv + 1, 1);
        P->claim = (int *)calloc((size_t)nv + 1, sizeof(int));
        P->pre = (signed char *)calloc((size_t)nv + 1, 1);
        P->idstamp = (int *)calloc((size_t)nclauses + 1, sizeof(int));
        P->ft = (int *)calloc((size_t)nv + 2, sizeof(int));
        P->klit = (int *)calloc((size_t)nclauses + 2, sizeof(int));
        P->kcl = (int *)calloc((size_t)nclauses + 2, sizeof(int));
        P->firstcl = (int *)calloc((size_t)nv + 1, sizeof(int));
        int fmax = 0;
        for (long i = 0; i < clause_off[nclauses]; i++) {
            int v = lits[i] > 0 ? lits[i] : -lits[i];
            P->occ[2 * v + (lits[i] < 0)]++;
            if (v > fmax) fmax = v;
        }
        for (int i = 0; i < nclauses; i++) {
            const int len = clause_off[i + 1] - clause_off[i];
            if (len == 0) P->has_empty = 1;
            p_max(P, DP_CLAUSE_LEN_MAX, len);
        }
        for (int i = 0; i < n_init; i++) {
            int v = init_assign[i] > 0 ? init_assign[i] : -init_assign[i];
            if (P->isinit[v]) P->v[DP_INIT_OVERWRITE]++;
            if (v > fmax) P->v[DP_INIT_VAR_BEYOND_FORMULA]++;
            P->isinit[v] = 1;
        }
        c.P = P;
    }

    formula *F = f_alloc(nclauses, clause_off[nclauses]);
    memcpy(F->pool, lits, sizeof(int) * (size_t)clause_off[nclauses]);
    for (int i = 0; i < nclauses; i++) { F->cl[i] = F->pool + clause_off[i]; F->len[i] = clause_off[i + 1] - clause_off[i]; F->id[i] = i; }
    F->nc = nclauses;
    assign_t *a = a_new(nv);
    for (int i = 0; i < n_init; i++) {   /* a caller-supplied dict: later keys overwrite, order kept */
        int lit = init_assign[i], v = lit > 0 ? lit : -lit;
        if (a->val[v] != 0) { a->val[v] = lit > 0 ? 1 : -1;
            for (int k = 0; k < a->n; k++) if ((a->order[k] > 0 ? a->order[k] : -a->order[k]) == v) a->order[k] = lit;
        } else a_set(a, lit);
    }
    dpll_node(&c, F, a, 0, 1);
    a_free(a); f_free(F);
    if (ctr) {
        ctr->nodes = c.nodes; ctr->decisions = c.decisions; ctr->unit_props = c.unit_props;
        ctr->pure_assigns = c.pure_assigns; ctr->conflicts = c.conflicts; ctr->solutions = c.solutions;
    }
    if (paths) {
        dpaths *P = &PP;
        if (c.solutions > sol_cap) P->v[DP_SOLS_PAST_CAP] = c.solutions - sol_cap;
        memcpy(paths, P->v, sizeof(P->v));
        free(P->occ); free(P->isinit); free(P->claim); free(P->pre); free(P->idstamp); free(P->ft);
        free(P->klit); free(P->kcl); free(P->firstcl);
    }
    return c.stop;
}

/* Returns 0 = search complete, 1 = stopped after max_solutions, 2 = node limit. */
int oracle_dpll(int nvars, int nclauses, const int32_t *clause_off, const int32_t *lits,
                int mode, int64_t max_solutions, int64_t node_limit,
                const int32_t *init_assign, int n_init,
                int32_t *sol_lits, int64_t sol_cap_lits, int64_t *sol_off, int64_t sol_cap,
                int32_t *root_assign, int *root_len, oracle_counters *ctr) {
    return dpll_run(nvars, nclauses, clause_off, lits, mode, max_solutions, node_limit, init_assign, n_init,
                    sol_lits, sol_cap_lits, sol_off, sol_cap, root_assign, root_len, ctr, NULL);
}

/* The same search; paths[0 .. npaths) receives the path counters (DP_*).
 * Returns -3 if npaths is not this library's count (a stale caller or library). */
int oracle_dpll_paths(int nvars, int nclauses, const int32_t *clause_off, const int32_t *lits,
                      int mode, int64_t max_solutions, int64_t node_limit,
                      const int32_t *init_assign, int n_init,
                      int32_t *sol_lits, int64_t sol_cap_lits, int64_t *sol_off, int64_t sol_cap,
                      int32_t *root_assign, int *root_len, oracle_counters *ctr, int64_t *paths, int npaths) {
    if (npaths != DP_NPATHS || !paths) return -3;
    return dpll_run(nvars, nclauses, clause_off, lits, mode, max_solutions, node_limit, init_assign, n_init,
                    sol_lits, sol_cap_lits, sol_off, sol_cap, root_assign, root_len, ctr, paths);
}
