// rfx_meta.hip -- reads to contigs with the dynamic-k ("meta") assembler in ONE resident call: the orchestrator of
// the reference, Pipelines.reflexivDSDynamicAssemblyStepsPipe (Pipelines.java:840-1291), over the stages this library has -- the
// reduction from reads (rfx_reduce.hip), the first-four passes and the iterations (rfx_dynamic.hip), 04Fixing (rfx_fixing.hip),
// 05FixingAgain / 06ContigEnds (rfx_fixing2.hip), the end mapping (rfx_endmap.hip), 07EndExtend (rfx_endext.hip), 08Extend and
// 09ExtendAgain (rfx_ctgext.hip, rfx_fixing2.hip) and the de-duplication (rfx_dedup.hip).  Nothing here is a stage: the driver owns the
// SCHEDULE, the PARTITION RULE and the SEAMS.
//
// THE SCHEDULE (:877-980).  00firstFour: the random reflection and four passes.  Then EIGHT iteration jobs, each a run of its own whose
// passes read the job's START: 5-9, 10-14, 15-19 (`for i = 5; i < 20; i += 5`, :886), then 21-30, 31-40, 41-50, 51-60, 61-70 (`for i =
// 21; i < 71; i += 10`, :925) -- the reference never runs an iteration 20 --, so only the job 61-70 drops the shorter forward records
// (the pass's rule from iteration 61 on).  Between two jobs the reference writes and reads a file; here the set stays, and what the
// file would have done to it is done in place: marker through its decimal text, left / right through theirs and clamped (k_mt_as_rows).
//
// THE PARTITION RULE (:877-883, :914-921, :954-974, repeated ahead of every later stage).  O = the caller's P; one P stands for
// `partitions` and `shufflePartition` alike, as everywhere in this library.  All divisions are integer divisions:
//     first four                                                   O
//     iterations 5-19                                              O >= 10 ? O * 80 / 100 : O
//     iterations 21-70                                             O >= 10 ? O * 60 / 100 : O
//     fixing, fixing again, mapping, extend, extend again          O >= 10 ? O * 40 / 100 : O
// The reference's 20 % (O >= 100) and 10 % (O >= 1000) tiers of the last line are out of reach: the stages take P <= 63.  The end
// mapping and the de-duplication take no P here (the stated deviations of sections 26 and 13).
//
// THE SEAMS are the library's own sets (DynDev, CtgDev, EeSetDev, MpHitsDev); no text is made between two stages and nothing goes to the
// caller's arrays but the final set.  At most one stage's input, output and scratch are live beside the read store.  The last stage runs
// through the public entry points on a view of the library's set: the de-duplication keeps its set type to itself.
//
// RFX_META_TRACE (set to anything): one line per stage on stderr with its host time (every stage returns after the stream has drained).
#include <algorithm>
#include <string>
#include <vector>
#include "rfx_internal.h"
#include "rfx_packed_words.h"

using namespace rfx;

namespace {

// the iteration jobs: (start, end, tier of the partition rule)
const int MT_JOBS[8][3] = {{5, 9, 1}, {10, 14, 1}, {15, 19, 1}, {21, 30, 2}, {31, 40, 2}, {41, 50, 2}, {51, 60, 2}, {61, 70, 2}};

// tier 0: first four, 1: iterations 5-19, 2: iterations 21-70, 3: everything behind them
int mt_p(int O, int tier) {
    static const int PERCENT[4] = {100, 80, 60, 40};
    return O >= 10 ? O * PERCENT[tier] / 100 : O;
}

// what the file between two jobs does to a record: rfx_dev_dyn_to_text prints marker, left and right in decimal and form 1 of the
// binarizer reads them back (nine digits of ten, left / right clamped); keys and extensions hold their bases and nothing else already
__global__ __launch_bounds__(256) void k_mt_as_rows(int64_t n, int32_t *__restrict__ marker, int32_t *__restrict__ left, int32_t *__restrict__ right) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    marker[i] = pk_int_as_text(marker[i]); left[i] = pk_clamp(pk_int_as_text(left[i])); right[i] = pk_clamp(pk_int_as_text(right[i]));
}

double mt_now_ms() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e3 + t.tv_nsec * 1e-6; }

int mt_params(rfx_ctx *ctx, const rfx_meta_params *p, int max_k) {
    if (!p) return RFX_E_ARG;
    if (!parts_ok(p->P)) { ctx->last_error = "meta: P outside 1..63"; return RFX_E_ARG; }
    if (max_k < 31 || max_k > 124) { ctx->last_error = "meta: max_k (the last k of the list) must be 31..124"; return RFX_E_ARG; }
    if (p->max_iteration < -1) { ctx->last_error = "meta: max_iteration below -1"; return RFX_E_ARG; }
    if (p->min_contig < 0) { ctx->last_error = "meta: a negative min_contig"; return RFX_E_ARG; }
    if (p->stop_after < RFX_META_FIRST_FOUR || p->stop_after > RFX_META_ASSEMBLY) { ctx->last_error = "meta: stop_after names no stage"; return RFX_E_ARG; }
    const rfx_map_params mp{p->map_seed, p->map_min_overlap, p->map_max_mismatch};
    return mp_params_ok(ctx, &mp) ? RFX_OK : RFX_E_ARG;
}

// what is live when the driver stops: the stage's own set, by kind
struct MtSets {
    DynDev dyn;                 // 00firstFour .. 04Fixing, 08Extend
    CtgDev ctg;                 // 05FixingAgain / 06ContigEnds (with the mapper's rows: the contigs they name), 09ExtendAgain
    MpHitsDev hits;             // the mapper's rows
    EeSetDev ee;                // 07EndExtend
};

struct MtTrace {
    bool on = getenv("RFX_META_TRACE") != nullptr;
    double t = mt_now_ms();
    void stage(const char *name, int P, int64_t n) {
        if (!on) return;
        const double now = mt_now_ms();
        fprintf(stderr, "meta: %-18s P %2d: %9.1f ms, %lld left\n", name, P, now - t, (long long)n);
        t = now;
    }
};

int mt_contigs(rfx_ctx *ctx, const DynDev &in, int max_k, CtgDev &c) {
    Fx2Plan plan;
    RFX_TRY(fx2_contigs_plan(ctx, in, max_k, plan));
    RFX_TRY(ctg_alloc(ctx, c, plan.m, plan.words));
    RFX_TRY(fx2_contigs_fill(ctx, in, plan, c.w.as<uint64_t>(), c.woff.as<int64_t>(), c.len.as<int64_t>(), c.left.as<int32_t>(), c.right.as<int32_t>()));
    return sync_checked(ctx);                                           // (the plan's scratch is read until here)
}

// every stage behind the reduction up to `stop`; a = the reduced set (taken over).  The result of the stage `stop` is left in `s`
int mt_run(rfx_ctx *ctx, DynDev &a, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, int max_k, const rfx_meta_params &p,
           int stop, rfx_meta_report *rep, MtSets &s) {
    const int O = p.P, P3 = mt_p(O, 3);
    const rfx_fix_params fp{max_k, p.scramble, p.max_iteration};
    const rfx_map_params mp{p.map_seed, p.map_min_overlap, p.map_max_mismatch};
    MtTrace tr;
    rep->n_reduced = a.n;
    // 00firstFour
    RFX_TRY(dyn_run_set(ctx, a, mt_p(O, 0), 1, 4, 1, 0));
    rep->n[RFX_META_FIRST_FOUR] = a.n;
    tr.stage("00firstFour", mt_p(O, 0), a.n);
    // 01Iteration*
    for (int j = 0; j < 8 && stop > RFX_META_FIRST_FOUR + j; j++) {
        const int P = mt_p(O, MT_JOBS[j][2]);
        if (a.n > 0) RFX_LAUNCH_N(k_mt_as_rows, a.n, a.n, a.marker.as<int32_t>(), a.left.as<int32_t>(), a.right.as<int32_t>());
        RFX_TRY(dyn_run_set(ctx, a, P, 0, 0, MT_JOBS[j][0], MT_JOBS[j][1]));
        rep->n[RFX_META_ITERATION_5_9 + j] = a.n;
        tr.stage(("01Iteration" + std::to_string(MT_JOBS[j][0]) + "_" + std::to_string(MT_JOBS[j][1])).c_str(), P, a.n);
    }
    if (stop <= RFX_META_ITERATION_61_70) { s.dyn = std::move(a); return RFX_OK; }
    // 04Fixing, through the packed seam
    RFX_TRY(fx_run_set(ctx, a, P3, fp, s.dyn));
    RFX_TRY(sync_checked(ctx));
    a = DynDev();
    rep->n[RFX_META_FIXING] = s.dyn.n;
    tr.stage("04Fixing", P3, s.dyn.n);
    if (stop == RFX_META_FIXING) return RFX_OK;
    // 05FixingAgain / 06ContigEnds
    {
        DynDev b;
        RFX_TRY(fx2_run(ctx, s.dyn, P3, fp.scramble, fp.max_iteration, b));
        RFX_TRY(sync_checked(ctx));
        s.dyn = DynDev();
        RFX_TRY(mt_contigs(ctx, b, max_k, s.ctg));
    }
    rep->n[RFX_META_FIXING_AGAIN] = rep->n[RFX_META_CONTIG_ENDS] = s.ctg.n;
    tr.stage("05FixingAgain", P3, s.ctg.n);
    if (stop <= RFX_META_CONTIG_ENDS) return RFX_OK;
    // the end mapping on the read store
    const Fx2View v = fx2_view(s.ctg);
    {
        MpPlan plan;
        RFX_TRY(mp_plan(ctx, v, d_words, d_read_len, n_reads, wpr, mp, plan));
        RFX_TRY(mp_hits_alloc(ctx, s.hits, plan.hits));
        RFX_TRY(mp_fill(ctx, v, d_words, d_read_len, n_reads, wpr, mp, plan, mp_hits(s.hits)));
        RFX_TRY(sync_checked(ctx));
    }
    rep->hits = rep->n[RFX_META_MAPPING] = s.hits.n;
    tr.stage("Mapping", 0, s.hits.n);
    if (stop == RFX_META_MAPPING) return RFX_OK;
    // 07EndExtend: the consensus through the packed seam, then the splice
    {
        EeConsDev cons;
        EeConsPlan cp;
        RFX_TRY(ee_consensus_plan_hits(ctx, v, d_words, d_read_len, wpr, mp_hits(s.hits), s.hits.n, mp.seed, cp));
        RFX_TRY(ee_cons_alloc(ctx, cons, s.ctg.n, cp.lwords, cp.rwords));
        RFX_TRY(ee_consensus_fill(ctx, cp, ee_cons_out(cons)));
        s.hits = MpHitsDev();
        EePlan plan;
        RFX_TRY(ee_contigs_plan(ctx, v, ee_cons_in(cons), max_k, plan));
        RFX_TRY(ee_set_alloc(ctx, s.ee, plan.m, plan.words));
        RFX_TRY(ee_contigs_fill(ctx, v, ee_cons_in(cons), plan, ee_set_out(s.ee)));
        RFX_TRY(sync_checked(ctx));
    }
    s.ctg = CtgDev();
    rep->n[RFX_META_END_EXTEND] = s.ee.n;
    tr.stage("07EndExtend", 0, s.ee.n);
    if (stop == RFX_META_END_EXTEND) return RFX_OK;
    // 08Extend
    {
        DynDev lng;
        DevBuf kmers;
        int64_t n31 = 0;
        RFX_TRY(ex_contig_ends(ctx, ee_set_in(s.ee), max_k, lng, kmers, &n31));
        RFX_TRY(fx_from_ends(ctx, kmers.as<uint64_t>(), n31, lng, P3, fp.scramble, fp.max_iteration, s.dyn));
        RFX_TRY(sync_checked(ctx));
    }
    s.ee = EeSetDev();
    rep->n[RFX_META_EXTEND] = s.dyn.n;
    tr.stage("08Extend", P3, s.dyn.n);
    if (stop == RFX_META_EXTEND) return RFX_OK;
    // 09ExtendAgain
    {
        DynDev b;
        RFX_TRY(fx2_run(ctx, s.dyn, P3, fp.scramble, fp.max_iteration, b));
        RFX_TRY(sync_checked(ctx));
        s.dyn = DynDev();
        RFX_TRY(mt_contigs(ctx, b, max_k, s.ctg));
    }
    rep->n[RFX_META_EXTEND_AGAIN] = s.ctg.n;
    tr.stage("09ExtendAgain", P3, s.ctg.n);
    return RFX_OK;
}

// a set of the library's as the public entry points of the de-duplication take one
rfx_contigs_packed mt_public(const CtgDev &c) {
    rfx_contigs_packed p{};
    p.n = c.n; p.words = c.w.as<uint64_t>(); p.word_off = c.woff.as<int64_t>(); p.len = c.len.as<int64_t>();
    p.cap_n = c.n; p.cap_words = c.words;
    return p;
}

// the file of the stage `stop` out of what mt_run left, written by that stage's own writer into a buffer of the library's
int mt_text(rfx_ctx *ctx, MtSets &s, int stop, const uint64_t *d_words, const uint32_t *d_read_len, int wpr, const rfx_meta_params &p, rfx_meta_report *rep,
            DevBuf &text, int64_t *total) {
    *total = 0;
    if (stop <= RFX_META_FIXING || stop == RFX_META_EXTEND) return dyn_to_text(ctx, s.dyn, nullptr, 0, total, &text);
    if (stop == RFX_META_FIXING_AGAIN || stop == RFX_META_CONTIG_ENDS || stop == RFX_META_EXTEND_AGAIN)
        return fx2_text(ctx, fx2_view(s.ctg), stop == RFX_META_FIXING_AGAIN ? 0 : stop == RFX_META_CONTIG_ENDS ? 1 : 2, nullptr, 0, total, &text);
    if (stop == RFX_META_MAPPING)
        return mp_text(ctx, fx2_view(s.ctg), d_words, d_read_len, wpr, mp_hits(s.hits), s.hits.n, p.map_seed, nullptr, 0, total, nullptr, &text);
    if (stop == RFX_META_END_EXTEND) return ee_text(ctx, ee_set_in(s.ee), nullptr, 0, total, &text);
    // Assembly: the de-duplication, then its text with min_contig
    CtgDev d;
    RFX_TRY(ctg_alloc(ctx, d, s.ctg.n, s.ctg.words));                   // (a merge takes no more words than its two parts)
    const rfx_contigs_packed in = mt_public(s.ctg);
    rfx_contigs_packed out = mt_public(d);
    RFX_TRY(rfx_dev_dedup_contigs(ctx, &in, &out, nullptr));
    rep->n[RFX_META_ASSEMBLY] = out.n;
    int64_t len = 0;
    const int st = rfx_dev_contigs_to_text(ctx, &out, p.min_contig, nullptr, 0, &len, nullptr);
    if (st != RFX_E_CAP) RFX_TRY(st);
    RFX_HIP(text.alloc((size_t)std::max<int64_t>(len, 1), ctx->stream));
    if (len > 0) RFX_TRY(rfx_dev_contigs_to_text(ctx, &out, p.min_contig, text.as<char>(), len, &len, nullptr));
    *total = len;
    return RFX_OK;
}

}  // namespace

extern "C" {

void rfx_meta_default_params(rfx_meta_params *p) try {
    if (!p) return;
    p->P = 8; p->scramble = 2; p->max_iteration = 150; p->min_contig = 500;
    p->map_seed = 21; p->map_min_overlap = 31; p->map_max_mismatch = 2;
    p->stop_after = RFX_META_ASSEMBLY;
} RFX_API_CATCH_VOID(nullptr)

int rfx_dev_meta_from_reduced(rfx_ctx *ctx, const rfx_dyn_packed *d_reduced, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads,
                              int words_per_read, int max_k, const rfx_meta_params *params, rfx_meta_report *report, rfx_contigs_packed *d_out) try {
    if (!ctx || !dyn_packed_ok(d_reduced) || n_reads < 0 || (n_reads > 0 && (!d_words || !d_read_len)) || words_per_read < 1 || !report ||
        !fx2_contigs_ok(d_out))
        return RFX_E_ARG;
    RFX_TRY(mt_params(ctx, params, max_k));
    if (params->stop_after != RFX_META_ASSEMBLY) { ctx->last_error = "meta: the device form runs to the end (stop_after = RFX_META_ASSEMBLY)"; return RFX_E_ARG; }
    RFX_HIP(hipSetDevice(ctx->device));
    *report = rfx_meta_report{};
    DynDev a;
    MtSets s;
    RFX_TRY(dyn_borrow(ctx, d_reduced, a));
    RFX_TRY(mt_run(ctx, a, d_words, d_read_len, n_reads, words_per_read, max_k, *params, RFX_META_ASSEMBLY, report, s));
    const rfx_contigs_packed in = mt_public(s.ctg);
    RFX_TRY(rfx_dev_dedup_contigs(ctx, &in, d_out, nullptr));           // (RFX_E_CAP: need_n / need_words set, nothing written)
    report->n[RFX_META_ASSEMBLY] = d_out->n;
    return RFX_OK;
} RFX_API_CATCH(ctx)

int rfx_dev_meta_reads(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int words_per_read, int max_read_len,
                       const int *klist, int n_k, const rfx_reduce_reads_params *reduce_params, const rfx_meta_params *params, rfx_meta_report *report,
                       rfx_contigs_packed *d_out) try {
    if (!ctx || !report || !fx2_contigs_ok(d_out)) return RFX_E_ARG;
    RFX_TRY(rr_check_args(ctx, d_words, d_read_len, n_reads, words_per_read, max_read_len, klist, n_k, reduce_params));
    RFX_TRY(mt_params(ctx, params, klist[n_k - 1]));
    if (params->stop_after != RFX_META_ASSEMBLY) { ctx->last_error = "meta: the device form runs to the end (stop_after = RFX_META_ASSEMBLY)"; return RFX_E_ARG; }
    RFX_HIP(hipSetDevice(ctx->device));
    *report = rfx_meta_report{};
    DynDev a;
    MtSets s;
    const double t0 = mt_now_ms();
    RFX_TRY(rr_reduce_set(ctx, d_words, d_read_len, n_reads, words_per_read, max_read_len, klist, n_k, *reduce_params, a, nullptr));
    if (getenv("RFX_META_TRACE")) fprintf(stderr, "meta: %-18s P %2d: %9.1f ms, %lld left\n", "reduce", reduce_params->P, mt_now_ms() - t0, (long long)a.n);
    RFX_TRY(mt_run(ctx, a, d_words, d_read_len, n_reads, words_per_read, klist[n_k - 1], *params, RFX_META_ASSEMBLY, report, s));
    const rfx_contigs_packed in = mt_public(s.ctg);
    RFX_TRY(rfx_dev_dedup_contigs(ctx, &in, d_out, nullptr));
    report->n[RFX_META_ASSEMBLY] = d_out->n;
    return RFX_OK;
} RFX_API_CATCH(ctx)

// host form: ASCII reads in, ONE text out -- the file of the stage params->stop_after names, written by that stage's own writer; one
// upload, one encode, one copy back.  A short buffer: *out_len set and nothing written (rfx_reduce_text's rule)
int rfx_meta_reads(rfx_ctx *ctx, const uint8_t *bases, const int64_t *read_off, int64_t n_reads, const int *klist, int n_k,
                   const rfx_reduce_reads_params *reduce_params, const rfx_meta_params *params, rfx_meta_report *report, char *out, int64_t cap,
                   int64_t *out_len) try {
    if (!ctx || !text_rows_ok((const char *)bases, read_off, n_reads) || !text_out_ok(out, cap, out_len)) return RFX_E_ARG;
    if (n_reads >= ((int64_t)1 << 31)) { ctx->last_error = "meta: 2^31 reads or more"; return RFX_E_LIMIT; }
    int64_t longest = 1;
    for (int64_t i = 0; i < n_reads; i++) {
        if (read_off[i + 1] < read_off[i]) return RFX_E_ARG;
        longest = std::max(longest, read_off[i + 1] - read_off[i]);
    }
    if (longest > 32 * (int64_t)30000) { ctx->last_error = "meta: a read of more than 960000 bases"; return RFX_E_LIMIT; }
    const int wpr = (int)((longest + 31) >> 5);
    // (a device pointer is not needed to check the arguments: any non-null stands in for the read store)
    RFX_TRY(rr_check_args(ctx, (const uint64_t *)read_off, (const uint32_t *)read_off, n_reads, wpr, (int)longest, klist, n_k, reduce_params));
    RFX_TRY(mt_params(ctx, params, klist[n_k - 1]));
    RFX_HIP(hipSetDevice(ctx->device));
    rfx_meta_report own{};
    rfx_meta_report *rep = report ? report : &own;
    *rep = rfx_meta_report{};
    DevBuf d_b, d_ro, d_words, d_len, text;
    const int64_t r1 = std::max<int64_t>(n_reads, 1);
    RFX_ALLOC(d_words, uint64_t, r1 * wpr); RFX_ALLOC(d_len, uint32_t, r1);
    if (n_reads > 0) {
        RFX_TRY(dyn_upload_text(ctx, (const char *)bases, read_off, n_reads, d_b, d_ro));
        RFX_TRY(encode_reads(ctx, d_b.as<uint8_t>(), d_ro.as<int64_t>(), n_reads, wpr, d_words.as<uint64_t>(), d_len.as<uint32_t>()));
        RFX_TRY(sync_checked(ctx));
        d_b.release(); d_ro.release();
    }
    DynDev a;
    MtSets s;
    int64_t total = 0;
    RFX_TRY(rr_reduce_set(ctx, d_words.as<uint64_t>(), d_len.as<uint32_t>(), n_reads, wpr, (int)longest, klist, n_k, *reduce_params, a, nullptr));
    RFX_TRY(mt_run(ctx, a, d_words.as<uint64_t>(), d_len.as<uint32_t>(), n_reads, wpr, klist[n_k - 1], *params, params->stop_after, rep, s));
    RFX_TRY(mt_text(ctx, s, params->stop_after, d_words.as<uint64_t>(), d_len.as<uint32_t>(), wpr, *params, rep, text, &total));
    return text_to_host(ctx, {{text, total, out, cap, out_len}}, false);
} RFX_API_CATCH(ctx)

}  // extern "C"
