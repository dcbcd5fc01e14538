// ReflexivMain.cpp -- see ReflexivMain.h.  Every call() forwards to one C-ABI entry point.
#include <thread>
#include "ReflexivMain.h"

#include <algorithm>
#include <cstring>

#include <hip/hip_runtime_api.h>

namespace reflexiv {

rfx_records ReflexivSubKmerRDD::view() {
    rfx_records r{};
    r.n = size();
    r.key = key.data(); r.marker = marker.data(); r.ext_off = extOff.data(); r.ext = ext.data();
    r.left = left.data(); r.right = right.data();
    r.cap_n = (int64_t)key.size(); r.cap_words = (int64_t)ext.size();
    return r;
}
void ReflexivSubKmerRDD::reserve(int64_t n, int64_t words) {
    n = std::max<int64_t>(n, 1); words = std::max<int64_t>(words, 1);
    key.resize(n); marker.resize(n); left.resize(n); right.resize(n); extOff.resize(n + 1); ext.resize(words);
}
void ReflexivSubKmerRDD::shrink(const rfx_records &r) {
    key.resize(r.n); marker.resize(r.n); left.resize(r.n); right.resize(r.n); extOff.resize(r.n + 1);
    ext.resize(r.n ? extOff[r.n] : 0);
}

ReflexivMain::ReflexivMain(int device) {
    int st = rfx_ctx_create(device, &ctx);
    if (st != RFX_OK) throw RfxException(st, "rfx_ctx_create", "an MI355X (gfx950) is required; there is no CPU path");
}
ReflexivMain::~ReflexivMain() { rfx_ctx_destroy(ctx); }

void ReflexivMain::check(int st, const char *where) const {
    if (st != RFX_OK) throw RfxException(st, where, rfx_last_error(ctx));
}

void ReflexivMain::FastqFilterWithQual::call(const std::string &text, std::vector<uint8_t> &bases, std::vector<int64_t> &readOff) const {
    fastqFilterWithQual(text, bases, readOff);
}
void ReflexivMain::DSFastqFilterOnlySeq::call(const std::string &text, std::vector<uint8_t> &bases, std::vector<int64_t> &readOff) const {
    dsFastqFilterOnlySeq(text, bases, readOff);
}

std::vector<uint64_t> ReflexivMain::ReverseComplementKmerBinaryExtraction::call(
    const std::vector<uint8_t> &bases, const std::vector<int64_t> &readOff) const {
    int64_t n = 0;
    const int64_t nr = (int64_t)readOff.size() - 1;
    int st = rfx_extract_canon(m.ctx, bases.data(), readOff.data(), nr, m.param.kmerSize, m.param.frontClip,
                               m.param.endClip, nullptr, 0, &n);
    if (st != RFX_OK && st != RFX_E_CAP) m.check(st, "rfx_extract_canon");
    std::vector<uint64_t> out((size_t)std::max<int64_t>(n, 1));
    m.check(rfx_extract_canon(m.ctx, bases.data(), readOff.data(), nr, m.param.kmerSize, m.param.frontClip,
                              m.param.endClip, out.data(), n, &n), "rfx_extract_canon");
    out.resize((size_t)n);
    return out;
}

KmerBinaryRDD ReflexivMain::KmerCounting_KmerCoverageFilter::call(const std::vector<uint64_t> &kmers) const {
    KmerBinaryRDD o;
    const int64_t n = (int64_t)kmers.size();
    o.kmer.resize((size_t)std::max<int64_t>(n, 1)); o.count.resize(o.kmer.size());
    int64_t mm = 0, d = 0;
    m.check(rfx_count_filter(m.ctx, kmers.data(), n, m.param.minKmerCoverage, m.param.maxKmerCoverage, m.param.twin,
                             o.kmer.data(), o.count.data(), n, &mm, &d), "rfx_count_filter");
    o.kmer.resize((size_t)mm); o.count.resize((size_t)mm);
    return o;
}

std::vector<uint64_t> ReflexivMain::ReverseComplementKmerBinaryExtractionFromDataset64::call(
    const std::vector<uint8_t> &bases, const std::vector<int64_t> &readOff) const {
    int64_t n = 0;
    const int64_t nr = (int64_t)readOff.size() - 1;
    const int W = m.param.kmerSize / 32 + 1;                     // kmerBinarySlots, U/DefaultParam.java:81
    int st = rfx_extract_canon_w(m.ctx, bases.data(), readOff.data(), nr, m.param.kmerSize, m.param.frontClip,
                                 m.param.endClip, nullptr, 0, &n);
    if (st != RFX_OK && st != RFX_E_CAP) m.check(st, "rfx_extract_canon_w");
    std::vector<uint64_t> out((size_t)std::max<int64_t>(n, 1) * W);
    m.check(rfx_extract_canon_w(m.ctx, bases.data(), readOff.data(), nr, m.param.kmerSize, m.param.frontClip,
                                m.param.endClip, out.data(), n, &n), "rfx_extract_canon_w");
    out.resize((size_t)n * W);
    return out;
}

void ReflexivMain::KmerBlocksCount::call(const std::vector<uint64_t> &kmers, std::vector<uint64_t> &keys,
                                         std::vector<int64_t> &counts) const {
    const int W = m.param.kmerSize / 32 + 1;
    const int64_t n = (int64_t)kmers.size() / W;
    keys.resize((size_t)std::max<int64_t>(n, 1) * W); counts.resize((size_t)std::max<int64_t>(n, 1));
    int64_t mm = 0, d = 0;
    m.check(rfx_count_filter_w(m.ctx, kmers.data(), n, m.param.kmerSize, m.param.minKmerCoverage, m.param.maxKmerCoverage,
                               keys.data(), counts.data(), n, &mm, &d), "rfx_count_filter_w");
    keys.resize((size_t)mm * W); counts.resize((size_t)mm);
}

std::string ReflexivMain::DSBinaryKmerToString::call(const uint64_t *b) const {
    static const char NUC[4] = {'A', 'C', 'G', 'T'};
    const int k = m.param.kmerSize, res = k % 32;                // kmerSizeResidue
    std::string sb;
    sb.reserve((size_t)k);
    for (int i = 0; i < (k / 32) * 32; i++) sb.push_back(NUC[(b[i / 32] >> (2 * (31 - i % 32))) & 3]);       // :346-352
    for (int i = (k / 32) * 32; i < k; i++) sb.push_back(NUC[(b[i / 32] >> (2 * (res - 1 - i % 32))) & 3]);  // :354-360
    return sb;
}

ReflexivSubKmerRDD ReflexivMain::KmerReverseComplement_ForwardSubKmerExtraction::call(const KmerBinaryRDD &in) const {
    ReflexivSubKmerRDD o;
    const int64_t n = (int64_t)in.kmer.size();
    o.reserve(2 * n, 2 * n);
    rfx_records r = o.view();
    m.check(rfx_rc_expand_subkmer(m.ctx, in.kmer.data(), in.count.data(), n, m.param.kmerSize, &r), "rfx_rc_expand_subkmer");
    o.shrink(r);
    return o;
}

ReflexivSubKmerRDD ReflexivMain::SortByKey::call(ReflexivSubKmerRDD &in, int P) const {
    ReflexivSubKmerRDD o;
    o.reserve(in.size(), (int64_t)in.ext.size());
    o.partStart.resize((size_t)P + 1);
    rfx_records ri = in.view(), ro = o.view();
    m.check(rfx_sort_records(m.ctx, &ri, P, &ro, o.partStart.data()), "rfx_sort_records");
    o.shrink(ro);
    return o;
}

static ReflexivSubKmerRDD fork_call(const ReflexivMain &m, bool reflected, ReflexivSubKmerRDD &in) {
    ReflexivSubKmerRDD o;
    const int P = (int)in.partStart.size() - 1;
    o.reserve(in.size(), in.size());
    o.partStart.resize(in.partStart.size());
    rfx_records ri = in.view(), ro = o.view();
    int st = reflected
        ? rfx_fork_filter_reflected(m.ctx, &ri, in.partStart.data(), P, m.param.kmerSize, m.param.minErrorCoverage,
                                    m.param.twin, &ro, o.partStart.data())
        : rfx_fork_filter_forward(m.ctx, &ri, in.partStart.data(), P, m.param.kmerSize, m.param.minErrorCoverage,
                                  m.param.twin, &ro, o.partStart.data());
    m.check(st, reflected ? "rfx_fork_filter_reflected" : "rfx_fork_filter_forward");
    o.shrink(ro);
    return o;
}
ReflexivSubKmerRDD ReflexivMain::FilterForkSubKmer::call(ReflexivSubKmerRDD &in) const { return fork_call(m, false, in); }
ReflexivSubKmerRDD ReflexivMain::FilterForkReflectedSubKmer::call(ReflexivSubKmerRDD &in) const { return fork_call(m, true, in); }

ReflexivSubKmerRDD ReflexivMain::ReflectedSubKmerExtractionFromForward::call(ReflexivSubKmerRDD &in) const {
    ReflexivSubKmerRDD o;
    o.reserve(in.size(), in.size());
    rfx_records ri = in.view(), ro = o.view();
    m.check(rfx_reflect_from_forward(m.ctx, &ri, m.param.kmerSize, &ro), "rfx_reflect_from_forward");
    o.shrink(ro);
    o.partStart = in.partStart;
    return o;
}

ReflexivSubKmerRDD ReflexivMain::kmerRandomReflection::call(ReflexivSubKmerRDD &in) const {
    ReflexivSubKmerRDD o;
    o.reserve(in.size(), in.size());
    rfx_records ri = in.view(), ro = o.view();
    m.check(rfx_random_reflection(m.ctx, &ri, in.partStart.data(), (int)in.partStart.size() - 1, m.param.kmerSize, &ro),
            "rfx_random_reflection");
    o.shrink(ro);
    o.partStart = in.partStart;
    return o;
}

ReflexivSubKmerRDD ReflexivMain::ExtendReflexivKmer::call(ReflexivSubKmerRDD &in) const {
    ReflexivSubKmerRDD o;
    const int P = (int)in.partStart.size() - 1;
    o.reserve(in.size(), (int64_t)in.ext.size());
    o.partStart.resize(in.partStart.size());
    rfx_records ri = in.view(), ro = o.view();
    m.check(rfx_extend_pass(m.ctx, &ri, in.partStart.data(), P, m.param.kmerSize, m.param.twin, stage, &ro,
                            o.partStart.data()), "rfx_extend_pass");
    o.shrink(ro);
    return o;
}

std::string ReflexivMain::KmerToContig::call(ReflexivSubKmerRDD &in, int64_t *nContigs) const {
    rfx_records ri = in.view();
    int64_t len = 0, nc = 0;
    int st = rfx_contigs_text(m.ctx, &ri, m.param.kmerSize, m.param.minContig, m.param.twin, nullptr, 0, &len, &nc);
    if (st != RFX_OK && st != RFX_E_CAP) m.check(st, "rfx_contigs_text");
    std::string out((size_t)len, '\0');
    m.check(rfx_contigs_text(m.ctx, &ri, m.param.kmerSize, m.param.minContig, m.param.twin, out.data(), len, &len, &nc),
            "rfx_contigs_text");
    if (nContigs) *nContigs = nc;
    return out;
}

// P/ReflexivMain.java:168-316
std::string ReflexivMain::assemblyFromCounts(const KmerBinaryRDD &counts, std::vector<int64_t> *trace) {
    if (!param.bubble)
        throw std::runtime_error("-bubble (no fork filtering) is unusable in the reference too (SURVEY.md C.6)");
    const int P0 = std::max(1, param.logicalPartitions);
    int P = P0;
    SortByKey sortByKey{*this};
    // Step: generate reverse complement k-mers, extract forward sub k-mers  :168-176
    ReflexivSubKmerRDD rdd = KmerReverseComplement_ForwardSubKmerExtraction{*this}.call(counts);
    // filter forks  :178-199
    rdd = sortByKey.call(rdd, P);
    rdd = FilterForkSubKmer{*this}.call(rdd);
    rdd = ReflectedSubKmerExtractionFromForward{*this}.call(rdd);
    rdd = sortByKey.call(rdd, P);
    rdd = FilterForkReflectedSubKmer{*this}.call(rdd);
    // Step 6  :204-205
    rdd = kmerRandomReflection{*this}.call(rdd);
    auto pass = [&](int stage) {
        rdd = sortByKey.call(rdd, P);                       // Step 7  :211
        rdd = ExtendReflexivKmer{*this, stage}.call(rdd);   // Step 8  :221-222
        if (trace) trace->push_back(rdd.size());
    };
    pass(0);
    int iterations = 0;
    for (int i = 1; i < 4; i++) { iterations++; pass(0); }  // :233-241
    iterations++;
    pass(1);                                                // :247-254
    int partitionNumber = P;                                // :263
    int64_t contigNumber = 0;
    while (iterations <= param.maximumIteration) {          // :265-296
        iterations++;
        if (iterations >= param.minimumIteration && iterations % 3 == 0) {
            int64_t currentContigNumber = rdd.size();       // count()  :270
            if (contigNumber == currentContigNumber) break;
            contigNumber = currentContigNumber;
            (void)partitionNumber;                          // coalesce (:277-281) is outside the order contract
        }
        pass(2);
    }
    int64_t nc = 0;
    return KmerToContig{*this}.call(rdd, &nc);              // Step 11  :302-316
}

std::string ReflexivMain::assembly(const std::string &fastqText, std::vector<int64_t> *trace) {
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    FastqFilterWithQual{*this}.call(fastqText, bases, readOff);                          // Steps 1-2  :126-134
    std::vector<uint64_t> kmers = ReverseComplementKmerBinaryExtraction{*this}.call(bases, readOff);   // Step 3  :147-148
    KmerBinaryRDD counts = KmerCounting_KmerCoverageFilter{*this}.call(kmers);            // Steps 4-5  :154-163
    return assemblyFromCounts(counts, trace);
}

namespace {
static_assert(GROW_OK == RFX_OK && GROW_E_CAP == RFX_E_CAP, "HostText.h's retry reads the library's statuses");

// the retry of HostText.h; a failure is `name: detail`
template <class Call> void growOrThrow(rfx_ctx *ctx, const char *name, std::initializer_list<GrowBuf> bufs, Call &&call) {
    if (growCall(bufs, call) != RFX_OK) throw std::runtime_error(std::string(name) + ": " + rfx_last_error(ctx));
}
}  // namespace

rfx_params ReflexivMain::assembleParams() const {
    rfx_params prm;
    rfx_default_params(&prm);
    prm.k = param.kmerSize; prm.min_cov = param.minKmerCoverage; prm.max_cov = param.maxKmerCoverage;
    prm.min_error_cov = param.minErrorCoverage; prm.min_contig = param.minContig;
    prm.min_iter = param.minimumIteration; prm.max_iter = param.maximumIteration;
    prm.front_clip = param.frontClip; prm.end_clip = param.endClip;
    prm.partitions = std::max(1, param.logicalPartitions); prm.twin = param.twin;
    return prm;
}

rfx_reduce_reads_params ReflexivMain::reduceReadsParams(int partitions) const {
    rfx_reduce_reads_params prm;
    rfx_reduce_reads_default_params(&prm);
    prm.min_cov = param.minKmerCoverage; prm.max_cov = param.maxKmerCoverage; prm.min_error_cov = param.minErrorCoverage;
    prm.min_repeat_fold = param.minRepeatFold; prm.bubble = param.bubble ? 1 : 0; prm.sensitive = param.sensitive ? 1 : 0;
    prm.front_clip = param.frontClip; prm.end_clip = param.endClip; prm.P = partitions;
    return prm;
}

rfx_fix_params ReflexivMain::fixParams() const {
    rfx_fix_params prm;
    rfx_fix_default_params(&prm, lastKmerOfList());
    prm.scramble = param.scramble; prm.max_iteration = param.maximumIteration;
    return prm;
}

// the reads of the resident drivers.  k > 31: as `counter` takes them (ReflexivDataFrameCounter64), the first step of the two-step route
void ReflexivMain::residentReads(const std::string &fastqText, std::vector<uint8_t> &bases, std::vector<int64_t> &readOff) {
    if (!param.bubble)
        throw std::runtime_error("-bubble (no fork filtering) is unusable in the reference too (SURVEY.md C.6)");
    if (param.kmerSize > 31) DSFastqFilterOnlySeq{*this}.call(fastqText, bases, readOff);
    else FastqFilterWithQual{*this}.call(fastqText, bases, readOff);
}

std::string ReflexivMain::assemblyResident(const std::string &fastqText, std::vector<int64_t> *trace) {
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    residentReads(fastqText, bases, readOff);
    const rfx_params prm = assembleParams();
    const int64_t nr = (int64_t)readOff.size() - 1;
    std::vector<int64_t> tr((size_t)param.maximumIteration + 8);
    int64_t len = 0, nc = 0, nt = 0, kept = 0;
    std::string out((size_t)1 << 20, '\0');
    check(growCall({{out, len}}, [&] {
        return rfx_assemble_reads(ctx, bases.data(), readOff.data(), nr, &prm, out.data(), (int64_t)out.size(), &len, &nc,
                                  tr.data(), (int64_t)tr.size(), &nt, &kept);
    }), "rfx_assemble_reads");
    if (trace) trace->assign(tr.begin(), tr.begin() + nt);
    return out;
}

namespace {
// What the host keeps of the dynamic-k drivers: the line scan (row_off over the non-empty lines, a trailing '\r' left to the
// device parser) and the refusal of a row with too few fields, before anything is uploaded.  The binarizer
// (DynamicKmerBinarizerFromReducedToSubKmer), the passes and DSBinarySubKmerWith{Short,Long}ExtensionToString run on the
// device behind rfx_dyn_run_text, on the packed record set.
std::string dynRunText(rfx_ctx *ctx, const std::string &csv, bool kmers, int P, int reflect, int four, int start, int end,
                       std::vector<int64_t> *trace) {
    const Rows rows = rowsOf(csv, kmers ? 1 : 2, "dynamic-k");
    std::string out(rows.text.size() + 32 * (size_t)rows.n() + 64, '\0');
    std::vector<int64_t> tr(256);
    int64_t nt = 0, len = 0;
    growOrThrow(ctx, "rfx_dyn_run_text", {{out, len}}, [&] {
        return rfx_dyn_run_text(ctx, rows.text.data(), rows.off.data(), rows.n(), kmers ? 0 : 1, P, reflect, four, start, end, out.data(),
                                (int64_t)out.size(), &len, tr.data(), (int64_t)tr.size(), &nt);
    });
    if (trace) trace->assign(tr.begin(), tr.begin() + std::min<int64_t>(nt, (int64_t)tr.size()));
    return out;
}
}  // namespace

std::string ReflexivMain::assemblyDynamicFirstFour(const std::string &csvText, std::vector<int64_t> *trace) {
    return dynRunText(ctx, csvText, true, std::max(1, param.logicalPartitions), 1, 4, 1, 0, trace);
}

std::string ReflexivMain::assemblyDynamicIteration(const std::string &csvText, int startIteration, int endIteration, std::vector<int64_t> *trace) {
    // (the reference's loop runs while (iterations <= endIteration) { iterations++; ... }: endIteration - startIteration + 1 passes,
    // every one of them under param.startIteration's rules)
    return dynRunText(ctx, csvText, false, std::max(1, param.logicalPartitions), 0, 0, startIteration, endIteration, trace);
}

std::string ReflexivMain::kmerSorting(const std::string &csvText) {
    const Rows rows = rowsOf(csvText);
    rfx_ksort_params prm;
    rfx_ksort_default_params(&prm, param.kmerSize);
    prm.max_k = lastKmerOfList();                                  // maxKmerSize = kmerListInt[length - 1]
    prm.min_error_cov = param.minErrorCoverage; prm.max_cov = param.maxKmerCoverage; prm.bubble = param.bubble ? 1 : 0;
    prm.min_repeat_fold = param.minRepeatFold;
    std::string out(2 * (rows.text.size() + 24 * (size_t)rows.n()) + 64, '\0');
    int64_t len = 0;
    growOrThrow(ctx, "rfx_ksort_text", {{out, len}}, [&] {
        return rfx_ksort_text(ctx, rows.text.data(), rows.off.data(), rows.n(), &prm, out.data(), (int64_t)out.size(), &len);
    });
    return out;
}

int ReflexivMain::lastKmerOfList() const { return lastKmerOf(param.kmerList); }

void ReflexivMain::kmerReduction(const std::string &shortText, const std::string &longText, int k1, int k2, int partitions, std::string *reducedShort,
                                 std::string *rewrittenLong) {
    const Rows s = rowsOf(shortText), l = rowsOf(longText);
    rfx_reduce_params prm;
    rfx_reduce_default_params(&prm, k1, k2);
    prm.max_k = std::max(k2, lastKmerOfList());
    // (a row comes back with its newline, and an edited marker may be one character longer)
    std::string o1(s.text.size() + 2 * (size_t)s.n() + 64, '\0'), o2(l.text.size() + 2 * (size_t)l.n() + 64, '\0');
    int64_t l1 = 0, l2 = 0;
    growOrThrow(ctx, "rfx_reduce_text", {{o1, l1}, {o2, l2}}, [&] {
        return rfx_reduce_text(ctx, s.text.data(), s.off.data(), s.n(), l.text.data(), l.off.data(), l.n(), partitions, &prm, o1.data(),
                               (int64_t)o1.size(), &l1, o2.data(), (int64_t)o2.size(), &l2);
    });
    *reducedShort = std::move(o1); *rewrittenLong = std::move(o2);
}

std::vector<std::string> ReflexivMain::kmerReductionFromReads(const std::string &fastqText, const std::vector<int> &klist, int partitions) {
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    DSFastqFilterOnlySeq{*this}.call(fastqText, bases, readOff);      // as counter()
    const int64_t nr = (int64_t)readOff.size() - 1;
    const rfx_reduce_reads_params prm = reduceReadsParams(partitions);
    if (bases.empty()) bases.push_back(0);
    std::string out(std::max<size_t>(4 * bases.size(), 1 << 16), '\0');
    std::vector<int64_t> off(klist.size() + 1, 0);
    int64_t len = 0;
    growOrThrow(ctx, "rfx_reduce_reads", {{out, len}}, [&] {
        return rfx_reduce_reads(ctx, bases.data(), readOff.data(), nr, klist.data(), (int)klist.size(), &prm, out.data(), (int64_t)out.size(), &len,
                                off.data());
    });
    std::vector<std::string> texts;
    for (size_t i = 0; i < klist.size(); i++) texts.push_back(out.substr((size_t)off[i], (size_t)(off[i + 1] - off[i])));
    return texts;
}

std::string ReflexivMain::metaAssemblyFromReads(const std::string &fastqText, const std::vector<int> &klist, int partitions, int stopAfter) {
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    DSFastqFilterOnlySeq{*this}.call(fastqText, bases, readOff);      // as counter()
    const int64_t nr = (int64_t)readOff.size() - 1;
    const rfx_reduce_reads_params rp = reduceReadsParams(partitions);
    rfx_meta_params mp;
    rfx_meta_default_params(&mp);
    mp.P = partitions; mp.scramble = param.scramble; mp.max_iteration = param.maximumIteration; mp.min_contig = param.minContig;
    mp.stop_after = stopAfter;
    if (bases.empty()) bases.push_back(0);
    std::string out(std::max<size_t>(2 * bases.size(), 1 << 16), '\0');
    int64_t len = 0;
    growOrThrow(ctx, "rfx_meta_reads", {{out, len}}, [&] {
        return rfx_meta_reads(ctx, bases.data(), readOff.data(), nr, klist.data(), (int)klist.size(), &rp, &mp, nullptr, out.data(), (int64_t)out.size(),
                              &len);
    });
    return out;
}

std::string ReflexivMain::dedupContigRows(const std::string &csvText) {
    const Rows rows = rowsOf(csvText);
    const int64_t n = rows.n();
    std::vector<uint8_t> bases;
    std::vector<int64_t> coff(1, 0);
    for (int64_t i = 0; i < n; i++) {
        const std::string row = rows.row(i);
        const size_t c = row.find(',');
        if (c == std::string::npos || row.compare(0, 8, ">Contig-") != 0) throw std::runtime_error("dedup row: " + row);
        size_t e = row.size();
        while (e > c + 1 && (row[e - 1] == '\n' || row[e - 1] == '\r')) e--;
        bases.insert(bases.end(), row.begin() + (long)c + 1, row.begin() + (long)e);
        coff.push_back((int64_t)bases.size());
    }
    if (bases.empty()) bases.push_back(0);
    std::string out(2 * bases.size() + 64 * (size_t)(n + 2) + 4096, '\0');
    int64_t len = 0;
    growOrThrow(ctx, "rfx_dedup_contigs", {{out, len}}, [&] {
        return rfx_dedup_contigs(ctx, bases.data(), coff.data(), n, param.minContig, nullptr, 0, nullptr, 0, nullptr, out.data(), (int64_t)out.size(), &len,
                                 nullptr);
    });
    return out;
}

// the host forms that take rows and rfx_fix_params and give one text (rfx_fix_text, rfx_ext_text, rfx_ext2_text).  min_commas: what a
// row must hold to be one of the stage's; stage: the word that a refused row's message begins with
std::string ReflexivMain::fixParamsText(FixTextFn fn, const char *name, const char *stage, const std::string &csvText, int partitions, int min_commas) {
    const Rows rows = rowsOf(csvText, min_commas, stage);
    const rfx_fix_params prm = fixParams();
    std::string out(rows.text.size() + 64 * (size_t)rows.n() + 64, '\0');
    int64_t len = 0;
    growOrThrow(ctx, name, {{out, len}}, [&] {
        return fn(ctx, rows.text.data(), rows.off.data(), rows.n(), partitions, &prm, out.data(), (int64_t)out.size(), &len);
    });
    return out;
}

std::string ReflexivMain::contigFixing(const std::string &csvText, int partitions) {
    return fixParamsText(rfx_fix_text, "rfx_fix_text", "fixing", csvText, partitions, 2);
}

std::string ReflexivMain::contigExtend(const std::string &csvText, int partitions) {
    return fixParamsText(rfx_ext_text, "rfx_ext_text", "extend", csvText, partitions, 1);
}

std::string ReflexivMain::contigExtendAgain(const std::string &csvText, int partitions) {
    return fixParamsText(rfx_ext2_text, "rfx_ext2_text", "extend2", csvText, partitions, 2);
}

void ReflexivMain::contigFixingRoundTwo(const std::string &csvText, int partitions, std::string *contigRows, std::string *contigEnds) {
    const Rows rows = rowsOf(csvText, 2, "fixing2");
    const rfx_fix_params prm = fixParams();
    std::string o1(rows.text.size() + 64 * (size_t)rows.n() + 64, '\0'), o2(o1.size(), '\0');
    int64_t l1 = 0, l2 = 0;
    growOrThrow(ctx, "rfx_fix2_text", {{o1, l1}, {o2, l2}}, [&] {
        return rfx_fix2_text(ctx, rows.text.data(), rows.off.data(), rows.n(), partitions, &prm, o1.data(), (int64_t)o1.size(), &l1, o2.data(),
                             (int64_t)o2.size(), &l2);
    });
    *contigRows = std::move(o1); *contigEnds = std::move(o2);
}

std::string ReflexivMain::contigEndExtend(const std::string &contigText, const std::string &samText) {
    const Rows contigs = rowsOf(contigText), rows = samRows(samText);
    std::string out(contigs.text.size() + 700 * (size_t)contigs.n() + 64, '\0');
    int64_t len = 0;
    growOrThrow(ctx, "rfx_endext_text", {{out, len}}, [&] {
        return rfx_endext_text(ctx, contigs.text.data(), contigs.off.data(), contigs.n(), rows.text.data(), rows.off.data(), rows.n(), lastKmerOfList(),
                               out.data(), (int64_t)out.size(), &len);
    });
    return out;
}

std::string ReflexivMain::contigMapping(const std::string &contigText, const std::string &fastqText, std::string *rows) {
    const Rows contigs = rowsOf(contigText);
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    DSFastqFilterOnlySeq{*this}.call(fastqText, bases, readOff);
    const int64_t nr = (int64_t)readOff.size() - 1;
    rfx_map_params prm;
    rfx_map_default_params(&prm);
    std::string out(bases.size() + 256 * (size_t)nr + 64, '\0');
    int64_t len = 0;
    growOrThrow(ctx, "rfx_map_text", {{out, len}}, [&] {
        return rfx_map_text(ctx, contigs.text.data(), contigs.off.data(), contigs.n(), bases.data(), readOff.data(), nr, &prm, out.data(),
                            (int64_t)out.size(), &len);
    });
    std::string ext = contigEndExtend(contigText, out);
    if (rows) *rows = std::move(out);
    return ext;
}

std::string ReflexivMain::mercyKmers(const std::string &countText, const std::string &fastqText) {
    const Rows counts = rowsOf(countText);
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    DSFastqFilterOnlySeq{*this}.call(fastqText, bases, readOff);
    const int64_t nr = (int64_t)readOff.size() - 1;
    std::string out((size_t)(param.kmerSize + 3) * (size_t)(nr + 64), '\0');
    int64_t len = 0;
    growOrThrow(ctx, "rfx_mercy_text", {{out, len}}, [&] {
        return rfx_mercy_text(ctx, counts.text.data(), counts.off.data(), counts.n(), bases.data(), readOff.data(), nr, param.kmerSize, param.frontClip,
                              param.endClip, out.data(), (int64_t)out.size(), &len);
    });
    return out;
}

std::string ReflexivMain::dedupContigText(const std::string &contigText) {
    std::string out(contigText.size() + 4096, '\0');
    int64_t len = 0, nc = 0;
    check(rfx_dedup_contig_text(ctx, contigText.data(), (int64_t)contigText.size(), param.minContig, out.data(), (int64_t)out.size(), &len, &nc,
                                nullptr), "rfx_dedup_contig_text");
    out.resize((size_t)len);
    return out;
}

std::string ReflexivMain::assemblyResidentSharded(const std::string &fastqText, int nGpus, std::vector<int64_t> *trace, int64_t gatherBelow) {
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    residentReads(fastqText, bases, readOff);
    const rfx_params prm = assembleParams();
    const int64_t nr = (int64_t)readOff.size() - 1;
    uint8_t id[128];
    check(rfx_comm_unique_id(id), "rfx_comm_unique_id");
    std::vector<std::string> outs((size_t)nGpus), errs((size_t)nGpus);
    std::vector<int64_t> tr((size_t)param.maximumIteration + 8);
    int64_t nt = 0;
    std::vector<std::thread> th;
    for (int r = 0; r < nGpus; r++)
        th.emplace_back([&, r] {
            rfx_ctx *c = nullptr; rfx_comm *comm = nullptr;
            try {
                if (rfx_ctx_create(r, &c) != RFX_OK) throw std::runtime_error("rfx_ctx_create(" + std::to_string(r) + ")");
                if (rfx_comm_init(c, id, r, nGpus, &comm) != RFX_OK) throw std::runtime_error(std::string("rfx_comm_init: ") + rfx_last_error(c));
                const int64_t a = nr * r / nGpus, b = nr * (r + 1) / nGpus;            // contiguous shares of the reads
                std::string out(r == 0 ? (size_t)3 * (size_t)(readOff[nr] - readOff[0]) + ((size_t)1 << 20) : (size_t)1 << 12, '\0');
                int64_t len = 0, nc = 0, n_tr = 0, tot[3];
                growOrThrow(c, "rfx_sharded_assemble_reads", {{out, len}}, [&] {      // (on every rank at once: the retry is collective)
                    return rfx_sharded_assemble_reads(c, comm, bases.data(), readOff.data() + a, b - a, &prm, 4, gatherBelow, out.data(),
                                                      (int64_t)out.size(), &len, &nc, r == 0 ? tr.data() : nullptr,
                                                      r == 0 ? (int64_t)tr.size() : 0, &n_tr, tot);
                });
                outs[(size_t)r] = out;
                if (r == 0) nt = n_tr;
            } catch (const std::exception &e) { errs[(size_t)r] = e.what(); }
            if (comm) rfx_comm_destroy(comm);
            if (c) rfx_ctx_destroy(c);
        });
    for (auto &t : th) t.join();
    for (auto &e : errs) if (!e.empty()) throw std::runtime_error(e);
    if (trace) trace->assign(tr.begin(), tr.begin() + nt);
    return outs[0];
}

// KmerBinarizer.call  P/ReflexivDSMain.java:3883-3931: the rows of countRow(); bases A0 C1 G2, anything else 3, 32 to the word
KmerBinaryRDD ReflexivMain::KmerBinarizer::call(const std::string &csvText) const {
    KmerBinaryRDD o;
    const int k = m.param.kmerSize;
    const Rows rows = rowsOf(csvText);
    for (int64_t r = 0; r < rows.n(); r++) {
        const KmerCount row = countRow(rows.row(r), k);
        uint64_t b = 0;
        for (int i = 0; i < k; i++) b = (b << 2) | baseCode(row.kmer[(size_t)i]);      // :3912-3919
        o.kmer.push_back(b); o.count.push_back(row.count);
    }
    return o;
}

// `run -kmerc`: load -> filter(min <= count <= max) (P/ReflexivDSMain.java:458-478) -> the same driver.
// The order contract wants the (kmer,count) list ascending, whatever order the files came in.
std::string ReflexivMain::assemblyFromKmer(const std::string &csvText, std::vector<int64_t> *trace) {
    KmerBinaryRDD in = KmerBinarizer{*this}.call(csvText);
    std::vector<size_t> idx;
    for (size_t i = 0; i < in.kmer.size(); i++)
        if (in.count[i] >= param.minKmerCoverage && in.count[i] <= param.maxKmerCoverage) idx.push_back(i);
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return in.kmer[a] < in.kmer[b]; });
    KmerBinaryRDD f;
    for (size_t i : idx) { f.kmer.push_back(in.kmer[i]); f.count.push_back(in.count[i]); }
    return assemblyFromCounts(f, trace);
}

// KmerBinarizer.call  P/ReflexivDSMain64.java:10772-10836: the same row rules as above, the k-mer into words of 31 bases
void ReflexivMain::KmerBinarizer64::call(const std::string &csvText, std::vector<uint64_t> &kmers, std::vector<int32_t> &counts) const {
    const int k = m.param.kmerSize, W = (k - 1) / 31 + 1;                                 // kmerBinarySlotsAssemble
    const Rows rows = rowsOf(csvText);
    for (int64_t r = 0; r < rows.n(); r++) {
        const KmerCount row = countRow(rows.row(r), k);
        const size_t at = kmers.size();
        kmers.resize(at + (size_t)W, 0);
        for (int i = 0; i < k; i++)                                                       // :10811-10819
            kmers[at + (size_t)(i / 31)] = (kmers[at + (size_t)(i / 31)] << 2) | baseCode(row.kmer[(size_t)i]);
        counts.push_back(row.count);
    }
}

// `run -kmerc COUNTS -kmer 63`: load -> filter(min <= count <= max) (:458-478) -> the k > 31 driver in one call.
// The order contract wants the list ascending by base string, whatever order the files came in.
std::string ReflexivMain::assemblyFromKmer64(const std::string &csvText, std::vector<int64_t> *trace) {
    const int W = (param.kmerSize - 1) / 31 + 1;
    std::vector<uint64_t> km; std::vector<int32_t> cn;
    KmerBinarizer64{*this}.call(csvText, km, cn);
    std::vector<size_t> idx;
    for (size_t i = 0; i < cn.size(); i++)
        if (cn[i] >= param.minKmerCoverage && cn[i] <= param.maxKmerCoverage) idx.push_back(i);
    std::sort(idx.begin(), idx.end(), [&](size_t a, size_t b) {
        return std::lexicographical_compare(km.begin() + a * W, km.begin() + (a + 1) * W, km.begin() + b * W, km.begin() + (b + 1) * W);
    });
    std::vector<uint64_t> fk; std::vector<int32_t> fc;
    for (size_t i : idx) { fk.insert(fk.end(), km.begin() + i * W, km.begin() + (i + 1) * W); fc.push_back(cn[i]); }
    rfx_params prm = assembleParams();
    // this route's own: the partition count as given (no floor of 1), and the twin at the library's default (the k > 31 passes ignore it)
    prm.partitions = param.logicalPartitions; prm.twin = RFX_TWIN_DS;
    std::vector<int64_t> tr((size_t)param.maximumIteration + 8);
    int64_t nt = 0, nc = 0, len = 0;
    std::string out((size_t)(4 * (fc.size() + 16) * (size_t)(param.kmerSize + 8) + 1024), '\0');
    check(growCall({{out, len}}, [&] {
        return rfx_assemble_counts_w(ctx, fk.data(), fc.data(), (int64_t)fc.size(), &prm, out.data(), (int64_t)out.size(), &len, &nc,
                                     tr.data(), (int64_t)tr.size(), &nt);
    }), "rfx_assemble_counts_w");
    if (trace) trace->assign(tr.begin(), tr.begin() + nt);
    return out;
}

// the k > 31 counter's rows "KMER,count" (P/ReflexivDataFrameCounter64.java:222-233), ascending k-mers
std::string ReflexivMain::countRows64(const std::vector<uint64_t> &keys, const std::vector<int64_t> &cnt) {
    const int W = param.kmerSize / 32 + 1;
    std::string out;
    DSBinaryKmerToString toString{*this};
    for (size_t i = 0; i < cnt.size(); i++) {
        out += toString.call(keys.data() + i * W);
        out.push_back(',');
        out += std::to_string(cnt[i]);
        out.push_back('\n');
    }
    return out;
}

// `counter --resident` at k = 33..100 (not a multiple of 32): the same rows as counter(), the reads packed and counted in HBM
// (rfx_dev_count_reads_w for reads of one length, rfx_dev_count_reads_ragged_w otherwise)
std::string ReflexivMain::counterResident(const std::string &fastqText) {
    const int k = param.kmerSize, W = k / 32 + 1;
    if (k < 33 || k > 100 || k % 32 == 0) throw std::runtime_error("counter --resident: -kmer 33..100, not 64 or 96");
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    DSFastqFilterOnlySeq{*this}.call(fastqText, bases, readOff);      // as counter()
    const int64_t nr = (int64_t)readOff.size() - 1;
    if (nr <= 0) return std::string();
    int64_t maxlen = 1, minlen = INT64_MAX;
    for (int64_t r = 0; r < nr; r++) {
        const int64_t l = readOff[r + 1] - readOff[r];
        maxlen = std::max(maxlen, l); minlen = std::min(minlen, l);
    }
    const int wpr = (int)((maxlen + 31) / 32);
    struct Dev {                                                       // device buffers of this call
        std::vector<void *> ps;
        void *get(size_t bytes) {
            void *p = nullptr;
            if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) throw std::runtime_error("counter --resident: hipMalloc failed");
            ps.push_back(p);
            return p;
        }
        ~Dev() { for (void *p : ps) (void)hipFree(p); }
    } dev;
    auto up = [](void *d, const void *h, size_t bytes) {
        if (bytes && hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("counter --resident: upload failed");
    };
    auto down = [](void *h, const void *d, size_t bytes) {
        if (bytes && hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("counter --resident: download failed");
    };
    check(rfx_ctx_sync(ctx), "rfx_ctx_sync");
    auto *d_bases = (uint8_t *)dev.get(bases.size());
    auto *d_off = (int64_t *)dev.get((size_t)(nr + 1) * 8);
    auto *d_words = (uint64_t *)dev.get((size_t)nr * wpr * 8);
    auto *d_len = (uint32_t *)dev.get((size_t)nr * 4);
    up(d_bases, bases.data(), bases.size());
    up(d_off, readOff.data(), (size_t)(nr + 1) * 8);
    check(rfx_dev_encode_reads(ctx, d_bases, d_off, nr, wpr, d_words, d_len), "rfx_dev_encode_reads");
    const bool uniform = minlen == maxlen;
    int64_t cap = std::max<int64_t>(1 << 16, (int64_t)bases.size() / 8), m = 0, dist = 0, inst = 0;
    uint64_t *d_keys = nullptr; int64_t *d_counts = nullptr;
    for (;;) {                                                         // grow on RFX_E_CAP (*out_n = the need)
        d_keys = (uint64_t *)dev.get((size_t)cap * 8 * W);
        d_counts = (int64_t *)dev.get((size_t)cap * 8);
        const int st = uniform
            ? rfx_dev_count_reads_w(ctx, d_words, nr, wpr, (int)maxlen, k, param.frontClip, param.endClip, param.minKmerCoverage,
                                    param.maxKmerCoverage, d_keys, d_counts, cap, &m, &dist, &inst)
            : rfx_dev_count_reads_ragged_w(ctx, d_words, d_len, nr, wpr, (int)maxlen, k, param.frontClip, param.endClip,
                                           param.minKmerCoverage, param.maxKmerCoverage, d_keys, d_counts, cap, &m, &dist, &inst);
        if (st == RFX_E_CAP && m > cap) { cap = m; continue; }
        check(st, uniform ? "rfx_dev_count_reads_w" : "rfx_dev_count_reads_ragged_w");
        break;
    }
    check(rfx_ctx_sync(ctx), "rfx_ctx_sync");
    std::vector<uint64_t> keys((size_t)m * W); std::vector<int64_t> cnt((size_t)m);
    down(keys.data(), d_keys, (size_t)m * 8 * W);
    down(cnt.data(), d_counts, (size_t)m * 8);
    return countRows64(keys, cnt);
}

// P/ReflexivCounter.java:109-191: k-mer, count text lines
std::string ReflexivMain::counter(const std::string &fastqText) {
    static const char NUC[4] = {'A', 'C', 'G', 'T'};
    std::vector<uint8_t> bases; std::vector<int64_t> readOff;
    DSFastqFilterOnlySeq{*this}.call(fastqText, bases, readOff);      // P/ReflexivDataFrameCounter.java:170-173
    if (param.kmerSize > 31) {                       // P/ReflexivDataFrameCounter64.java:133-232
        std::vector<uint64_t> kmers = ReverseComplementKmerBinaryExtractionFromDataset64{*this}.call(bases, readOff);
        std::vector<uint64_t> keys; std::vector<int64_t> cnt;
        KmerBlocksCount{*this}.call(kmers, keys, cnt);
        return countRows64(keys, cnt);
    }
    std::vector<uint64_t> kmers = ReverseComplementKmerBinaryExtraction{*this}.call(bases, readOff);
    KmerBinaryRDD counts = KmerCounting_KmerCoverageFilter{*this}.call(kmers);
    std::string out;
    const int k = param.kmerSize;
    for (size_t i = 0; i < counts.kmer.size(); i++) {
        for (int j = 0; j < k; j++) out.push_back(NUC[(counts.kmer[i] >> (2 * (k - 1 - j))) & 3]);
        out.push_back(',');
        out += std::to_string(counts.count[i]);
        out.push_back('\n');
    }
    return out;
}

}  // namespace reflexiv
