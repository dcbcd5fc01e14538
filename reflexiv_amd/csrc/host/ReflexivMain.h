// ReflexivMain.h -- C++ host mirror of P/ReflexivMain.java (the RDD-surface twin) and
// P/ReflexivCounter.java over the C ABI of libreflexiv_hip.so.
//
// The reference is Java on Spark; no JVM exists in the build or test environment, so the host
// side above the C ABI is written here in C++ with the reference's class and method names: one
// nested class per Spark operator, each with a call() that takes the partition's records and
// returns the operator's output, and a driver assembly() that applies them in the order of
// P/ReflexivMain.java:147-316.  Errors surface as exceptions (Java: unchecked exceptions ->
// task failure); there is no CPU path.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/reflexiv_hip.h"
#include "DefaultParam.h"
#include "HostText.h"

namespace reflexiv {

struct RfxException : std::runtime_error {
    int status;
    RfxException(int st, const std::string &where, const std::string &detail)
        : std::runtime_error(where + ": status " + std::to_string(st) + (detail.empty() ? "" : " -- " + detail)),
          status(st) {}
};

// JavaPairRDD<Long, Integer> KmerBinaryRDD  (P/ReflexivMain.java:105)
struct KmerBinaryRDD {
    std::vector<uint64_t> kmer;
    std::vector<int32_t> count;
};

// JavaPairRDD<Long, Tuple4<Integer, Long[], Integer, Integer>> (P/ReflexivMain.java:108-109);
// a single-word extension is a one-word array.  partStart = logical partition offsets.
struct ReflexivSubKmerRDD {
    std::vector<uint64_t> key, ext;
    std::vector<int32_t> marker, left, right;
    std::vector<int64_t> extOff, partStart;
    int64_t size() const { return (int64_t)key.size(); }
    rfx_records view();
    void reserve(int64_t n, int64_t words);
    void shrink(const rfx_records &r);
};

class ReflexivMain {
public:
    explicit ReflexivMain(int device = -1);
    ~ReflexivMain();
    void setParam(const DefaultParam &p) { param = p; }          // P/ReflexivMain.java:3126-3128

    // ---- operators (one per inner class; names kept)
    struct FastqFilterWithQual {            // :3089-3113 (+ FastqUnitFilter :3080-3084)
        ReflexivMain &m;
        // text -> concatenated sequence lines + offsets
        void call(const std::string &text, std::vector<uint8_t> &bases, std::vector<int64_t> &readOff) const;
    };
    struct DSFastqFilterOnlySeq {           // P/ReflexivDataFrameCounter.java:238-290 (the counter's line filter)
        ReflexivMain &m;
        void call(const std::string &text, std::vector<uint8_t> &bases, std::vector<int64_t> &readOff) const;
    };
    struct ReverseComplementKmerBinaryExtraction {   // :3002-3075
        ReflexivMain &m;
        std::vector<uint64_t> call(const std::vector<uint8_t> &bases, const std::vector<int64_t> &readOff) const;
    };
    struct KmerCounting_KmerCoverageFilter {         // reduceByKey(:2895-2899) + filter(:3115-3119)
        ReflexivMain &m;
        KmerBinaryRDD call(const std::vector<uint64_t> &kmers) const;
    };
    // ---- k > 31: P/ReflexivDataFrameCounter64.java (W = kmerBinarySlots words per k-mer)
    struct ReverseComplementKmerBinaryExtractionFromDataset64 {   // :390-687
        ReflexivMain &m;
        std::vector<uint64_t> call(const std::vector<uint8_t> &bases, const std::vector<int64_t> &readOff) const;
    };
    struct KmerBlocksCount {                         // groupBy("kmerBlocks").count() + filters :191-205
        ReflexivMain &m;
        // kmers: W words per k-mer; -> rows (W words, count) ascending
        void call(const std::vector<uint64_t> &kmers, std::vector<uint64_t> &keys, std::vector<int64_t> &counts) const;
    };
    struct DSBinaryKmerToString {                    // :335-384
        ReflexivMain &m;
        std::string call(const uint64_t *kmerBlocks) const;
    };
    struct KmerReverseComplement_ForwardSubKmerExtraction {   // :2901-2931 + :2703-2731
        ReflexivMain &m;
        ReflexivSubKmerRDD call(const KmerBinaryRDD &in) const;
    };
    struct SortByKey {                               // sortByKey() :179,191,211,235,247,286
        ReflexivMain &m;
        ReflexivSubKmerRDD call(ReflexivSubKmerRDD &in, int P) const;
    };
    struct FilterForkSubKmer {                       // :2406-2541 (with or without error correction)
        ReflexivMain &m;
        ReflexivSubKmerRDD call(ReflexivSubKmerRDD &in) const;
    };
    struct ReflectedSubKmerExtractionFromForward {   // :2734-2769
        ReflexivMain &m;
        ReflexivSubKmerRDD call(ReflexivSubKmerRDD &in) const;
    };
    struct FilterForkReflectedSubKmer {              // :2543-2697
        ReflexivMain &m;
        ReflexivSubKmerRDD call(ReflexivSubKmerRDD &in) const;
    };
    struct kmerRandomReflection {                    // :2774-2886
        ReflexivMain &m;
        ReflexivSubKmerRDD call(ReflexivSubKmerRDD &in) const;
    };
    struct ExtendReflexivKmer {                      // :2019-2401, :1564-2013, :762-1558 by stage
        ReflexivMain &m; int stage;
        ReflexivSubKmerRDD call(ReflexivSubKmerRDD &in) const;
    };
    struct KmerToContig {                            // :693-758 + :588-638 + :571-582
        ReflexivMain &m;
        std::string call(ReflexivSubKmerRDD &in, int64_t *nContigs) const;
    };

    // ---- drivers
    // assembly(): P/ReflexivMain.java:95-322 from FASTQ text to the contig text of saveAsTextFile
    std::string assembly(const std::string &fastqText, std::vector<int64_t> *trace = nullptr);
    // the same result through ONE call (rfx_assemble_reads): reads go up, contig text comes back.  k = 33..100: what
    // `counter` followed by `run -kmerc` gives (the counter's FASTQ reader; also assemblyResidentSharded)
    std::string assemblyResident(const std::string &fastqText, std::vector<int64_t> *trace = nullptr);
    // the same on the nGpus GPUs of this node: one host thread, context and RCCL communicator per GPU, every thread passes its
    // share of the reads to rfx_sharded_assemble_reads (the shuffle of reduceByKey, P/ReflexivMain.java:155, over RCCL)
    // P/ReflexivDSDynamicKmerDedup.java assemblyFromKmer (:138-339) on the contig text of a run: each contig once
    std::string dedupContigText(const std::string &contigText);
    // gatherBelow: the extend stage stays range-sharded over the GPUs (sortByKey as an RCCL all-to-all) while the record set has
    // more records than this (-1: the library's default; rfx_dev_sharded_assemble)
    std::string assemblyResidentSharded(const std::string &fastqText, int nGpus, std::vector<int64_t> *trace = nullptr, int64_t gatherBelow = -1);
    // ReflexivCounter.assembly(): P/ReflexivCounter.java:109-191 -> lines "KMER,count"
    std::string counter(const std::string &fastqText);
    // `counter --resident` at k = 33..100: the same CSV, counted in HBM (rfx_dev_count_reads_w / rfx_dev_count_reads_ragged_w)
    std::string counterResident(const std::string &fastqText);
    std::string countRows64(const std::vector<uint64_t> &keys, const std::vector<int64_t> &cnt);
    std::string assemblyFromCounts(const KmerBinaryRDD &counts, std::vector<int64_t> *trace = nullptr);
    // assemblyFromKmer(): P/ReflexivMain.java:327-568 / P/ReflexivDSMain.java:362-712 -- `run -kmerc`:
    // CSV rows "KMER,count" (also the legacy "(KMER,count)" tuple text) as written by `counter`
    struct KmerBinarizer {                           // P/ReflexivDSMain.java:3871-3947
        ReflexivMain &m;
        KmerBinaryRDD call(const std::string &csvText) const;
    };
    std::string assemblyFromKmer(const std::string &csvText, std::vector<int64_t> *trace = nullptr);
    // k > 31: ReflexivDSMain64.assemblyFromKmer (P/ReflexivDSMain64.java:374-826) -- `run -kmerc COUNTS -kmer 63`.
    // KmerBinarizer :10772-10836 writes kmerBinarySlotsAssemble = (k-1)/31+1 words of 31 bases per k-mer.
    struct KmerBinarizer64 {
        ReflexivMain &m;
        void call(const std::string &csvText, std::vector<uint64_t> &kmers, std::vector<int32_t> &counts) const;
    };
    std::string assemblyFromKmer64(const std::string &csvText, std::vector<int64_t> *trace = nullptr);
    // The dynamic-k ("meta") passes.  ReflexivDSDynamicKmerFirstFour.assemblyFromKmer
    // (P/ReflexivDSDynamicKmerFirstFour.java:137-224): CSV rows "KMER,marker|left|right" -> DynamicKmerBinarizerFromReducedToSubKmer
    // (:2931-3016) -> DSkmerRandomReflection -> 4 x (sort, DSExtendReflexivKmer) -> DSBinarySubKmerWithShortExtensionToString
    // (:226-263) rows "SUBKMER,marker|left|right,EXTENSION".  ReflexivDSDynamicKmerIteration.assemblyFromKmer
    // (P/ReflexivDSDynamicKmerIteration.java:134-205): those rows -> (end - start + 1) x (sort, DSExtendReflexivKmerToArrayLoop).
    std::string assemblyDynamicFirstFour(const std::string &csvText, std::vector<int64_t> *trace = nullptr);
    std::string assemblyDynamicIteration(const std::string &csvText, int startIteration, int endIteration,
                                         std::vector<int64_t> *trace = nullptr);
    // ReflexivDSKmerLeftAndRightSorting.assemblyFromKmer (P/ReflexivDSKmerLeftAndRightSorting.java:105-243) -- `sort -kmerc COUNTS
    // -kmer K`: CSV rows "KMER,count" of `counter` -> the rows "KMER,1|left|right" of Count_<K>_sorted, which `firstfour` reads.
    // One call (rfx_ksort_text): binarizer, reverse complement, both sorts, both fork filters and the text writer on the device.
    std::string kmerSorting(const std::string &csvText);
    // ReflexivDSDynamicMercyKmer.assemblyFromKmer (P/ReflexivDSDynamicMercyKmer.java:157-322; -sensitive, every k <= 31) -- `mercy -kmerc
    // O/Count_<K> -fastq F -kmer K`: the rows "KMER,count" of `counter` and the FASTQ text (DSFastqFilterOnlySeq, as the driver reads it,
    // :208-209) -> the rows "KMER,1" of Count_<K>_mercy: the k-mers of the holes between two solid windows of one read.  One call
    // (rfx_mercy_text): the solid set, the read store, the index, both passes and the text writer on the device.
    std::string mercyKmers(const std::string &countText, const std::string &fastqText);
    // ReflexivDSDynamicKmerRuduction.assemblyFromKmer (P/ReflexivDSDynamicKmerRuduction.java:143-287) -- `reduce`: the rows
    // "KMER,marker|left|right" of Count_<k1>_sorted and Count_<k2>_sorted -> the rows of Count_<k1>_reduced (reducedShort) and of the
    // rewritten Count_<k2>_sorted / Count_<k2>_reduced (rewrittenLong).  One call (rfx_reduce_text): everything between on the device.
    void kmerReduction(const std::string &shortText, const std::string &longText, int k1, int k2, int partitions, std::string *reducedShort,
                       std::string *rewrittenLong);
    // Pipelines.reflexivDSDynamicReductionPipe (P/Pipelines.java:1315-1737) -- `reduce -fastq F -klist K1,K2,... -partition P [-sensitive]`:
    // the FASTQ text (DSFastqFilterOnlySeq, as the counter reads it) -> the rows of Count_<k>_reduced of every k of the list, in list
    // order.  One call (rfx_reduce_reads): one upload and one 2-bit encode of the reads; counter, mercy k-mers, sorter and the reduction
    // of every pair on the device with no text between them; minErrorCoverage follows the orchestrator's rule (:1412-1416, :1489-1493).
    std::vector<std::string> kmerReductionFromReads(const std::string &fastqText, const std::vector<int> &klist, int partitions);
    // ReflexivDSDynamicKmerFixing.assemblyFromKmer (P/ReflexivDSDynamicKmerFixing.java:125-260) -- `fixing`: the rows
    // "SUBKMER,marker|left|right,EXTENSION" of the last iteration's output -> the rows of Assembly_intermediate/04Fixing.  One call
    // (rfx_fix_text): everything between on the device.  maxKmerSize is the last k of the k list.
    std::string contigFixing(const std::string &csvText, int partitions);
    // ReflexivDSDynamicKmerFixingRoundTwo.assemblyFromKmer (P/ReflexivDSDynamicKmerFixingRoundTwo.java:138-263) -- `fixing2`: the rows of
    // 04Fixing -> the rows "ID,contig" of Assembly_intermediate/05FixingAgain and the FASTA of contig ends of 06ContigEnds.  One call
    // (rfx_fix2_text): everything between on the device.  maxKmerSize is the last k of the k list.
    void contigFixingRoundTwo(const std::string &csvText, int partitions, std::string *contigRows, std::string *contigEnds);
    // ReflexivDSDynamicKmerMapping.assemblyFromKmer BEHIND its aligner (P/ReflexivDSDynamicKmerMapping.java:305-347) -- `endextend`: the
    // rows of 05FixingAgain and the alignment rows "contig \t start \t cigar \t seq" of any aligner run on 06ContigEnds -> the rows of
    // Assembly_intermediate/07EndExtend.  A line of 11 fields or more is a full SAM line: header and `*` lines are skipped, fields 3, 4, 6
    // and 10 taken (the commented awk of :1189).  One call (rfx_endext_text).  maxKmerSize is the last k of the k list.
    std::string contigEndExtend(const std::string &contigText, const std::string &samText);
    // The FRONT half of ReflexivDSDynamicKmerMapping.assemblyFromKmer (P/ReflexivDSDynamicKmerMapping.java:162-223, :1157-1266: every read
    // through an external aligner on 06ContigEnds) -- `mapping`: the rows of 05FixingAgain and the FASTQ text (DSFastqFilterOnlySeq, as the
    // driver reads it, :285-294) -> the rows of Assembly_intermediate/07EndExtend, with the library's own end-overhang mapper in the
    // aligner's place (rfx_map_text, DESIGN.md section 26: semantics of this project's own) and contigEndExtend behind it.  rows (optional)
    // receives the alignment rows "name \t start \t cigar \t seq" the mapper made.
    std::string contigMapping(const std::string &contigText, const std::string &fastqText, std::string *rows = nullptr);
    // ReflexivDSDynamicKmerExtend.assemblyFromKmer (P/ReflexivDSDynamicKmerExtend.java:125-254) -- `extend`: the rows of 07EndExtend -> the
    // rows "SUBKMER,marker|left|right,EXTENSION" of Assembly_intermediate/08Extend.  One call (rfx_ext_text).
    std::string contigExtend(const std::string &csvText, int partitions);
    // ReflexivDSDynamicKmerExtendRoundTwo.assemblyFromKmer (P/ReflexivDSDynamicKmerExtendRoundTwo.java:125-221) -- `extend2`: the rows of
    // 08Extend -> the rows ">Contig-<len>-<idx>,<contig>" of Assembly_intermediate/09ExtendAgain.  One call (rfx_ext2_text).
    std::string contigExtendAgain(const std::string &csvText, int partitions);
    // Pipelines.reflexivDSDynamicReductionPipe + Pipelines.reflexivDSDynamicAssemblyStepsPipe (P/Pipelines.java:1315-1737, :840-1291) --
    // `meta -fastq F -klist K1,K2,... -partition P`: the FASTQ text -> the file of ONE stage of the run from reads to contigs, stopAfter
    // = RFX_META_* (RFX_META_ASSEMBLY: the de-duplicated contigs of at least -mincontig bases).  One call (rfx_meta_reads): one upload
    // and one 2-bit encode of the reads, every stage on the device with no text between them, the partition rule the driver's.
    std::string metaAssemblyFromReads(const std::string &fastqText, const std::vector<int> &klist, int partitions, int stopAfter);
    // ReflexivDSDynamicKmerDedup.assemblyFromKmer (P/ReflexivDSDynamicKmerDedup.java:138-339) -- `dedup`: the rows
    // ">Contig-<len>-<idx>,<contig>" of 09ExtendAgain -> the text of Assembly (contigs of at least -mincontig bases).  One call
    // (rfx_dedup_contigs: pack, the three rounds and the text on the device).
    std::string dedupContigRows(const std::string &csvText);
    int lastKmerOfList() const;                      // param.kmerListInt[length - 1]

    rfx_ctx *ctx = nullptr;
    DefaultParam param;
    void check(int st, const char *where) const;     // a failure is `where: status N -- detail`
    // the library's parameter structs from param, each filled in one place
    rfx_params assembleParams() const;
    rfx_reduce_reads_params reduceReadsParams(int partitions) const;
    rfx_fix_params fixParams() const;                // maxKmerSize is the last k of the k list
    void residentReads(const std::string &fastqText, std::vector<uint8_t> &bases, std::vector<int64_t> &readOff);
    using FixTextFn = int (*)(rfx_ctx *, const char *, const int64_t *, int64_t, int, const rfx_fix_params *, char *, int64_t, int64_t *);
    std::string fixParamsText(FixTextFn fn, const char *name, const char *stage, const std::string &csvText, int partitions, int min_commas);
};

}  // namespace reflexiv
