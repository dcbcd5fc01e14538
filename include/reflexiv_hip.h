/*
 * reflexiv_hip.h -- C ABI of libreflexiv_hip.so, the MI355X (gfx950) implementation of
 * Reflexiv's k-mer counting + reflexible extend-and-merge hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI seam of its own:
 * the path sits behind Spark's Java functional interfaces, one inner class per operator,
 * called once per partition.  Every "operator" entry point below replaces the body of one
 * of those classes (cited as P/<file>:<lines>, P = src/main/java/uni/bielefeld/cmg/
 * reflexiv/pipeline) and takes / returns the same records as flat arrays; INTEGRATION.md
 * shows the JNI stub that binds each of them.  Conventions:
 *
 *  - plain pointers and sizes only; the caller owns every buffer (Java: direct
 *    ByteBuffers or arrays pinned with GetPrimitiveArrayCritical);
 *  - host entry points (rfx_*) take HOST pointers, stage through HBM and run the HIP
 *    kernels; device entry points (rfx_dev_*) take DEVICE pointers and run on the
 *    context's stream, for callers that keep the data resident (the Python/torch
 *    harness, the C++ driver, the multi-GPU path);
 *  - return value: RFX_OK or a negative rfx_status; never aborts, never falls back to a
 *    CPU path.  A k outside the entry's range, a negative clip and words_per_read * 32 <
 *    read_len are refused with RFX_E_ARG before anything is launched or written (*out_n and
 *    its like included).  RFX_E_CAP means an output buffer was too small: *out_n (and
 *    *out_words, *out_len) hold the needed size -- what to call again with.  What else was
 *    written depends on the family (DESIGN.md "Capacity contract"):
 *      - rfx_extract_canon[_w], rfx_count_filter[_w], every rfx_records and rfx_dyn_records
 *        output (host and rfx_dev_*), every rfx_contigs_packed output, the survivor arrays of
 *        rfx_dedup_contigs and rfx_dev_contigs_unpack, and the sort
 *        path of rfx_dev_count_reads_w (k >= 129) check before they copy or emit: no output
 *        array was written;
 *      - rfx_dev_count_reads[_ragged][_w], rfx_dev_count_kmers, rfx_dev_count_records,
 *        rfx_dev_count_wide_records, rfx_dev_count_wide_elems, rfx_dev_merge_pairs and
 *        rfx_dev_combine_reads (d_out_pairs; the scratch buffer is the callee's) know their
 *        survivors only after the leaves have emitted them: the first `cap` entries of the
 *        output arrays are unspecified, nothing at or past `cap` is written;
 *      - text buffers (rfx_contigs_text, rfx_dev_assemble[_w], rfx_assemble_counts_w,
 *        rfx_assemble_reads, the sharded drivers, rfx_dedup_contigs / rfx_dedup_contig_text,
 *        rfx_dev_contigs_to_text, rfx_dev_fix2_to_text, rfx_dev_fix2_ends_text, rfx_dev_endext_to_text,
 *        rfx_dev_ext2_to_text, rfx_dev_map_to_text, rfx_dev_mercy_to_text)
 *        are filled up to `cap`: the bytes below it are unspecified (a prefix of the text),
 *        nothing at or past `cap` is written;
 *  - re-entrant per context; one context = one device + one HIP stream.
 *
 * Record layout = the reference's: key is the (k-1)-mer, 2 bits per
 * base, first base in the highest used pair; marker 1 = forward (sequence = key||ext),
 * 2 = reflected (ext||key); ext words [ext_off[i], ext_off[i+1]): word 0 holds the first
 * f (1..31) bases under a 1-bit sentinel at bit 2f, every further word exactly 31 bases;
 * left/right are the bubble-distance markers (< 0: free end).
 */
#ifndef REFLEXIV_HIP_H
#define REFLEXIV_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    RFX_OK        =  0,
    RFX_E_ARG     = -1,   /* bad argument (k out of range, null pointer, ...)              */
    RFX_E_CAP     = -2,   /* output capacity too small; needed size reported              */
    RFX_E_HIP     = -3,   /* a HIP runtime call failed; see rfx_last_error()               */
    RFX_E_NOGPU   = -4,   /* no usable gfx950 device                                       */
    RFX_E_STATE   = -5,   /* "impossible" record state (the reference prints and goes on)  */
    RFX_E_LIMIT   = -6,   /* size beyond this build's limits (e.g. > 2^32-1 records)       */
    RFX_E_HOST    = -7    /* a C++ exception (std::bad_alloc, std::system_error ...) was caught at this boundary; what() in
                           * rfx_last_error().  Every entry point is a function-try-block: nothing unwinds into the caller  */
} rfx_status;

#define RFX_TWIN_DS  0    /* arithmetic of P/ReflexivDSMain.java (the wired, fixed twin)   */
#define RFX_TWIN_RDD 1    /* arithmetic of P/ReflexivMain.java (the RDD-surface twin)      */

typedef struct rfx_ctx rfx_ctx;

/* U/DefaultParam.java:74-120 -- the fields that reach the hot path. */
typedef struct {
    int32_t k;               /* kmerSize (<= 31: rfx_dev_assemble; 32..125: rfx_dev_assemble_w)  :74  */
    int32_t min_cov;         /* minKmerCoverage                                :103 */
    int32_t max_cov;         /* maxKmerCoverage                                :104 */
    int32_t min_error_cov;   /* minErrorCoverage (4 * 2)                       :105 */
    int32_t min_contig;      /* minContig                                      :107 */
    int32_t min_iter;        /* minimumIteration                               :115 */
    int32_t max_iter;        /* maximumIteration                               :114 */
    int32_t front_clip;      /* frontClip                                      :119 */
    int32_t end_clip;        /* endClip                                        :120 */
    int32_t partitions;      /* logical partitions P of the order contract */
    int32_t twin;            /* RFX_TWIN_DS / RFX_TWIN_RDD                      */
    int32_t coalesce;        /* apply P/ReflexivMain.java:277-281               */
    int32_t extras;          /* k > 31 only (rfx_dev_assemble_w): the from-counts extras of P/ReflexivDSMain64.java:584-619,
                              * 672-712 -- orientation doubling, extendable / unextendable split, end filters.  Default 1
                              * (the reference's driver always runs them); 0 iterates every record to the end. */
} rfx_params;

/* Flat record set.  n and the pointers are filled by the caller on input; on output the
 * callee sets n (and ext_off[n] words of ext).  cap_n / cap_words are the capacities of
 * the caller's output buffers (ext_off needs cap_n + 1 entries); on RFX_E_CAP nothing is
 * written except need_n / need_words (and key_words); no array is touched. */
typedef struct {
    int64_t   n;
    uint64_t *key;
    int32_t  *marker;
    int64_t  *ext_off;
    uint64_t *ext;
    int32_t  *left;
    int32_t  *right;
    int64_t   cap_n;
    int64_t   cap_words;
    int64_t   need_n;      /* set by the callee: records / words the output needs */
    int64_t   need_words;
    int32_t   key_words;   /* words per key: 0 or 1 for k <= 32; (k-2)/31+1 for k > 32, key then holds n * key_words
                            * words, record i at key[i * key_words ..] (31 bases per word, the last word the remaining
                            * (k-2)%31+1 bases right-aligned: P/ReflexivDSMain64.java, U/DefaultParam.java:93-94).
                            * The callee sets it on output records. */
    int32_t   reserved_;
} rfx_records;

/* ------------------------------------------------------------------ context */

int  rfx_version(void);
void rfx_default_params(rfx_params *p);                 /* U/DefaultParam.java defaults   */
/* device < 0: current device.  Fails with RFX_E_NOGPU when there is no gfx950 GPU.       */
int  rfx_ctx_create(int device, rfx_ctx **out);
void rfx_ctx_destroy(rfx_ctx *ctx);
int  rfx_ctx_sync(rfx_ctx *ctx);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the context's own. */
int  rfx_ctx_set_stream(rfx_ctx *ctx, void *hip_stream);
void *rfx_ctx_stream(rfx_ctx *ctx);
const char *rfx_last_error(rfx_ctx *ctx);               /* text of the last RFX_E_HIP / RFX_E_HOST / RFX_E_STATE */
/* The context keeps its large buffers between calls (grow-only workspaces: the count stage's record buffers ~ 3 B per
 * k-mer instance, the extend stage's two arenas, and -- rfx_assemble_reads -- the packed reads plus, up to
 * RFX_KEEP_STAGING_BYTES = 8 GiB, the ASCII staging).  rfx_ctx_workspace_bytes reports what is held; rfx_ctx_trim waits
 * for the context's stream and hands everything back to the driver (the next call allocates again). */
int  rfx_ctx_trim(rfx_ctx *ctx);
int64_t rfx_ctx_workspace_bytes(rfx_ctx *ctx);

/* ------------------------------------------------- operators, host buffers */

/* ReverseComplementKmerBinaryExtraction.call  P/ReflexivMain.java:3013-3075
 * (DS: P/ReflexivDSMain.java:3961-4024, P/ReflexivDataFrameCounter.java:459-526).
 * ASCII reads, read i = bases[read_off[i] .. read_off[i+1]); emits the canonical k-mers
 * in read order, window order. */
int rfx_extract_canon(rfx_ctx *ctx, const uint8_t *bases, const int64_t *read_off,
                      int64_t n_reads, int k, int front_clip, int end_clip,
                      uint64_t *out_kmers, int64_t cap, int64_t *out_n);

/* reduceByKey(KmerCounting) + filter(KmerCoverageFilter)
 * P/ReflexivMain.java:155,160-163,2895-2899,3115-3119 (DS :207-216).
 * Output ascending by k-mer (the order contract's count-stage order). */
int rfx_count_filter(rfx_ctx *ctx, const uint64_t *kmers, int64_t n,
                     int min_cov, int max_cov, int twin,
                     uint64_t *out_keys, int32_t *out_counts, int64_t cap,
                     int64_t *out_n, int64_t *out_distinct);

/* ---- k > 31: the counter's multi-word k-mers ----
 * W = k/32+1 words per k-mer, words 0..W-2 hold 32 bases each, the last word the k%32 remaining
 * bases right-aligned (P/ReflexivDataFrameCounter64.java:429-437); k > 32, k % 32 != 0, W <= 8.
 * Arrays hold W consecutive words per k-mer, as the reference's Row(long[]) does. */

/* ReverseComplementKmerBinaryExtractionFromDataset64.call
 * P/ReflexivDataFrameCounter64.java:401-650 (canonical by compareLongArrayBlocks :652-687:
 * base-wise fwd < rc, ties -> fwd).  Skip rule :410.  cap/out_n count k-mers, not words. */
int rfx_extract_canon_w(rfx_ctx *ctx, const uint8_t *bases, const int64_t *read_off,
                        int64_t n_reads, int k, int front_clip, int end_clip,
                        uint64_t *out_kmers, int64_t cap, int64_t *out_n);

/* groupBy("kmerBlocks").count() + filter(count >= min if min > 1) + filter(count <= max if
 * max < 10000000)  P/ReflexivDataFrameCounter64.java:191-205.  Output ascending by base string. */
int rfx_count_filter_w(rfx_ctx *ctx, const uint64_t *kmers, int64_t n, int k,
                       int min_cov, int max_cov,
                       uint64_t *out_keys, int64_t *out_counts, int64_t cap,
                       int64_t *out_n, int64_t *out_distinct);

/* KmerReverseComplement.call + ForwardSubKmerExtraction.call
 * P/ReflexivMain.java:2910-2930, 2709-2730 (DS :3849-3868, :3625-3644).
 * n (kmer,count) -> 2n single-word records; ext carries no sentinel yet. */
int rfx_rc_expand_subkmer(rfx_ctx *ctx, const uint64_t *kmers, const int32_t *counts,
                          int64_t n, int k, rfx_records *out);

/* sortByKey() / sort("k-1")  P/ReflexivMain.java:179,191,211,235,247,286: global stable
 * sort by key; also returns the logical partition starts part_start[P+1]. */
int rfx_sort_records(rfx_ctx *ctx, const rfx_records *in, int P,
                     rfx_records *out, int64_t *part_start);

/* FilterForkSubKmer[WithErrorCorrection].call  P/ReflexivMain.java:2412-2540
 * (DS :3375-3483).  Input sorted by key with its partition starts. */
int rfx_fork_filter_forward(rfx_ctx *ctx, const rfx_records *in, const int64_t *part_start,
                            int P, int k, int min_error_cov, int twin,
                            rfx_records *out, int64_t *out_part_start);

/* ReflectedSubKmerExtractionFromForward.call  P/ReflexivMain.java:2742-2768 (DS :3661-3685) */
int rfx_reflect_from_forward(rfx_ctx *ctx, const rfx_records *in, int k, rfx_records *out);

/* FilterForkReflectedSubKmer[WithErrorCorrection].call  P/ReflexivMain.java:2550-2696
 * (DS :3493-3616) */
int rfx_fork_filter_reflected(rfx_ctx *ctx, const rfx_records *in, const int64_t *part_start,
                              int P, int k, int min_error_cov, int twin,
                              rfx_records *out, int64_t *out_part_start);

/* kmerRandomReflection.call  P/ReflexivMain.java:2783-2885 (DS :3697-3805) */
int rfx_random_reflection(rfx_ctx *ctx, const rfx_records *in, const int64_t *part_start,
                          int P, int k, rfx_records *out);

/* ExtendReflexivKmer / ExtendReflexivKmerToArrayFirstTime / ExtendReflexivKmerToArrayLoop
 * .call  P/ReflexivMain.java:2048-2362, 1594-1974, 792-1519 (DS :3040-3329, :2589-2971,
 * :1776-2518).  One extend pass over records sorted by key.  stage: 0 single word,
 * 1 first array pass, 2 array loop -- the three classes share one algorithm and one
 * word layout; stage 0 additionally checks that every output fits one word. */
int rfx_extend_pass(rfx_ctx *ctx, const rfx_records *in, const int64_t *part_start, int P,
                    int k, int twin, int stage, rfx_records *out, int64_t *out_part_start);

/* ---- k > 31: the assembler's twin P/ReflexivDSMain64.java (assemblyFromKmer :374-826) ----
 * Every record operator above also takes k = 32 .. 125: keys are then (k-1)-mers of key_words = (k-2)/31+1 words
 * (rfx_records.key_words; 31 bases per word), the class bodies replaced are DSKmerReverseComplement +
 * DSForwardSubKmerExtraction (:10706-10755, :10363-10403; rfx_rc_expand_subkmer: k-mers of (k-1)/31+1 words each in
 * the layout KmerBinarizer writes, :10812-10819 -- NOT the counter's 32-bases-per-word layout), sort("k-1"),
 * DSFilterForkSubKmer[WithErrorCorrection] (:10072-10208), DSReflectedSubKmerExtractionFromForward (:10426-10475),
 * DSFilterForkReflectedSubKmer[WithErrorCorrection] (:10210-10360), DSkmerRandomReflection (:10491-10690),
 * DSExtendReflexivKmer / ...ToArrayFirstTime / ...ToArrayLoop (:9465-10070, :8733-9463, :7446-8731; twin is ignored,
 * this class has the DS arithmetic only) and DSBinaryReflexivKmerArrayToString + DSKmerToContig + TagRowContigID
 * (:1913-1975, :842-892, :830-841; header ">Contig-<len>-<idx>").  Flips and merges follow the sequence model
 * (SURVEY.md B.7); the one case where the reference's bit code differs is recorded in SURVEY.md C.9. */

/* DSExtendReflexivKmerToArrayLoop.call with param.scramble (2 or 3) as the class reads it (:7484-7486: the task's
 * emission marker starts at 1 instead of 2 once scramble == 3).  Any k the record operators take. */
int rfx_extend_pass_w(rfx_ctx *ctx, const rfx_records *in, const int64_t *part_start, int P, int k, int stage,
                      int scramble, rfx_records *out, int64_t *out_part_start);

/* The operator classes of the k > 31 from-counts extras (P/ReflexivDSMain64.java:584-619, 672-712), one `op` each, on
 * records sorted by key with their partition starts (any k the record operators take):
 *   RFX_OP_DOUBLE            DSReflexivAndForwardKmer :2126-3042: every record, then its other orientation (out: 2n
 *                            records, 2 x words; out_part_start = 2 x part_start)
 *   RFX_OP_EXTENDABLE_PAIRS  DSFilterExtendableKmerPairs :5305-6375: both members of every (forward, reflected) pair on
 *                            one key that the extend pass would merge, both as forward records; a task's last holder too
 *   RFX_OP_UNEXTENDABLE      DSFilterUnExtendableKmer :6377-7444: the rest (reflected holders come out forward)
 *   RFX_OP_FIRST_OF_KEY      DSFilterStillExtendableKmerFromPairs :3228-3390: of two records on one key the first
 *   RFX_OP_LONGER_OF_KEY     DSFilterStillExtendableKmerEnds :3044-3226: ... the one with the larger length*31+first word
 *   RFX_OP_ALL_FORWARD / RFX_OP_ALL_REFLECTED   DSFilterUnExtendableKmerLeftEnds :3392-4347 / ...RightEnds :4349-5303 */
#define RFX_OP_DOUBLE           0
#define RFX_OP_EXTENDABLE_PAIRS 1
#define RFX_OP_UNEXTENDABLE     2
#define RFX_OP_FIRST_OF_KEY     3
#define RFX_OP_LONGER_OF_KEY    4
#define RFX_OP_ALL_FORWARD      5
#define RFX_OP_ALL_REFLECTED    6
int rfx_extras_operator(rfx_ctx *ctx, int op, const rfx_records *in, const int64_t *part_start, int P, int k,
                        rfx_records *out, int64_t *out_part_start);

/* BinaryReflexivKmerArrayToString + KmerToContig + TagContigID
 * P/ReflexivMain.java:696-741, 590-637, 573-581 (DS :855-900, :743-795, :717-725):
 * the text saveAsTextFile writes (host-side formatting). */
int rfx_contigs_text(rfx_ctx *ctx, const rfx_records *in, int k, int min_contig, int twin,
                     char *out, int64_t cap, int64_t *out_len, int64_t *out_contigs);

/* ------------------------------------------- resident pipeline, device buffers */

/* 2-bit read store: read i occupies words [i*words_per_read, (i+1)*words_per_read), base j
 * in word j/32 at bits 63-2*(j%32)..62-2*(j%32) (code A0 C1 G2, anything else 3:
 * P/ReflexivMain.java:3062-3074), read_len[i] bases.  All pointers are device pointers. */
int rfx_dev_encode_reads(rfx_ctx *ctx, const uint8_t *d_bases, const int64_t *d_read_off,
                         int64_t n_reads, int words_per_read,
                         uint64_t *d_words, uint32_t *d_read_len);

/* Number of k-mer instances the extraction emits for uniform reads (host arithmetic). */
int64_t rfx_kmers_per_read(int read_len, int k, int front_clip, int end_clip);

/* Workspace bytes rfx_dev_count_reads needs for n_kmers instances. */
int64_t rfx_count_workspace_bytes(int64_t n_kmers);

/* extract + reduceByKey + filter fused, reads of one uniform length already packed in HBM.
 * d_out_keys/d_out_counts (cap entries) receive the survivors ascending by k-mer.
 * d_workspace: rfx_count_workspace_bytes(n_reads * kmers_per_read) bytes.
 * shard_lo/shard_hi select the radix shard [lo, hi) of 2^16 of the k-mer hash space that
 * this call counts (0, 65536 = everything); used by the multi-GPU path. */
int rfx_dev_count_reads(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads,
                        int words_per_read, int read_len, int k, int front_clip, int end_clip,
                        int min_cov, int max_cov, int twin,
                        void *d_workspace, int64_t workspace_bytes,
                        uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap,
                        int64_t *out_n, int64_t *out_distinct, int64_t *out_instances);

/* k > 31 twin of rfx_dev_count_reads (all device pointers; d_out_keys: cap*W words, W = k/32+1, ascending).  k = 33..127
 * (W = 2..4) count on the bucketed LDS-table path with no limit on the instances per call (only the survivors are sorted:
 * fewer than 2^32, else RFX_E_LIMIT); W >= 5 (k >= 128) keeps the sort path (fewer than 2^32 instances per call). */
int64_t rfx_kmers_per_read_w(int read_len, int k, int front_clip, int end_clip);
int rfx_dev_count_reads_w(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads,
                          int words_per_read, int read_len, int k, int front_clip, int end_clip,
                          int min_cov, int max_cov,
                          uint64_t *d_out_keys, int64_t *d_out_counts, int64_t cap,
                          int64_t *out_n, int64_t *out_distinct, int64_t *out_instances);

/* The same for reads of different lengths (real FASTQ): d_read_len[i] bases in read i, as
 * rfx_dev_encode_reads writes them; max_read_len <= 32 * words_per_read bounds them.  Every d_read_len[i] must be
 * <= max_read_len (the call cannot check it: the windows of a longer read beyond those of max_read_len are lost
 * while *out_instances still counts them); this holds for rfx_dev_count_reads_ragged_w as well. */
int rfx_dev_count_reads_ragged(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len,
                               int64_t n_reads, int words_per_read, int max_read_len, int k,
                               int front_clip, int end_clip, int min_cov, int max_cov, int twin,
                               uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap,
                               int64_t *out_n, int64_t *out_distinct, int64_t *out_instances);

/* k = 33..127 (not 64 or 96) twin of rfx_dev_count_reads_ragged, with the output of rfx_dev_count_reads_w (ascending,
 * k/32+1 words per key, int64 counts).  A read emits the k > 31 counter's windows of its own length: none when
 * len - k - end_clip + 1 <= 0 (P/ReflexivDataFrameCounter64.java:410) -- so a read of k (k + 1) bases emits 1 (2),
 * unlike the k <= 31 rule.  No base at or past d_read_len[i] reaches a k-mer: the words past a read's length may
 * hold anything (they may be loaded, but nothing of them is used).  RFX_E_CAP: *out_n = the survivors' need. */
int rfx_dev_count_reads_ragged_w(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len,
                                 int64_t n_reads, int words_per_read, int max_read_len, int k,
                                 int front_clip, int end_clip, int min_cov, int max_cov,
                                 uint64_t *d_out_keys, int64_t *d_out_counts, int64_t cap,
                                 int64_t *out_n, int64_t *out_distinct, int64_t *out_instances);

/* Multi-GPU exchange support for k = 33..63: the canonical two-word k-mers of packed reads (16-byte
 * elements {word0, word1}) written contiguously per owner (owner = mulhi(hash(k-mer), n_owners)),
 * d_owner_off[n_owners+1] element offsets; and the count of such elements after the exchange
 * (any order) -> ascending (2 words per key, int64 counts), as rfx_dev_count_reads_w returns them.
 * Two-word elements move as 128-bit units: d_out_elems, and d_elems at k = 33..63, lie at multiples of 16 bytes
 * (every element offset of such a buffer, e.g. an owner's bucket d_out_elems + 16 * d_owner_off[o], is one). */
int rfx_dev_bucket_wide_by_owner(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads,
                                 int words_per_read, int read_len, int k, int front_clip, int end_clip,
                                 int n_owners, void *d_out_elems, int64_t cap_elems,
                                 int64_t *d_owner_off, int64_t *h_owner_off);
/* rfx_dev_count_wide_elems also takes k = 65..127 (not 96): elements of k/32+1 words, counted with the same bucketed path
 * (as rfx_count_filter_w on host arrays and the sharded count's receiver at k = 65..125 do). */
int rfx_dev_count_wide_elems(rfx_ctx *ctx, const void *d_elems, int64_t n_elems, int k,
                             int min_cov, int max_cov,
                             uint64_t *d_out_keys, int64_t *d_out_counts, int64_t cap,
                             int64_t *out_n, int64_t *out_distinct);

/* The same two steps on 32-byte super-k-mer RECORDS of two-word k-mers (k = 33..63): a run of <= 16
 * consecutive windows that share the minimiser of their CENTRAL 31 (k odd) / 30 (k even) bases, carried
 * as the run's k + windows - 1 bases + a header; ~5 B per instance across the exchange instead of 16.
 * Bucketing: d_out_records = NULL / cap_records = 0 reports *out_n_records (RFX_E_CAP), as for k <= 31. */
int rfx_dev_bucket_wide_records_by_owner(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int words_per_read,
                                         int read_len, int k, int front_clip, int end_clip, int n_owners,
                                         void *d_out_records, int64_t cap_records, int64_t *d_owner_off,
                                         int64_t *h_owner_off, int64_t *out_n_records);
int rfx_dev_count_wide_records(rfx_ctx *ctx, const void *d_records, int64_t n_records, int64_t n_instances_hint, int k,
                               int min_cov, int max_cov, uint64_t *d_out_keys, int64_t *d_out_counts, int64_t cap,
                               int64_t *out_n, int64_t *out_distinct);

/* Same, from an explicit k-mer array (the reduceByKey input) in HBM. */
int rfx_dev_count_kmers(rfx_ctx *ctx, const uint64_t *d_kmers, int64_t n,
                        int min_cov, int max_cov, int twin,
                        void *d_workspace, int64_t workspace_bytes,
                        uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap,
                        int64_t *out_n, int64_t *out_distinct);

/* Multi-GPU exchange support: bucket the canonical k-mers of packed reads by owner
 * (owner = hash(kmer) * n_owners >> 64, the radix shard of the k-mer space), writing each
 * owner's k-mers contiguously into d_out with d_owner_off[n_owners+1] element offsets. */
int rfx_dev_bucket_by_owner(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads,
                            int words_per_read, int read_len, int k, int front_clip,
                            int end_clip, int n_owners, uint64_t *d_out, int64_t cap,
                            int64_t *d_owner_off, int64_t *h_owner_off);

/* The same two steps on super-k-mer RECORDS (16 bytes per run of <= 16 consecutive windows that
 * share a minimiser; ~2.6 B per instance instead of 8), for k = 21..31.  Bucketing: call with
 * d_out = NULL / cap_records = 0 to learn *out_n_records (returns RFX_E_CAP), then with a buffer.
 * Counting: n_instances_hint (k-mer instances the records hold, 0 = unknown) sizes the radix plan. */
int rfx_dev_bucket_records_by_owner(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int words_per_read,
                                    int read_len, int k, int front_clip, int end_clip, int n_owners,
                                    void *d_out_records, int64_t cap_records, int64_t *d_owner_off,
                                    int64_t *h_owner_off, int64_t *out_n_records);
int rfx_dev_count_records(rfx_ctx *ctx, const void *d_records, int64_t n_records, int64_t n_instances_hint,
                          int k, int min_cov, int max_cov, int twin, uint64_t *d_out_keys,
                          int32_t *d_out_counts, int64_t cap, int64_t *out_n, int64_t *out_distinct);

/* The same exchange AFTER a local combine -- the map-side combine of `reduceByKey`
 * (P/ReflexivMain.java:155; Spark sums per key inside every map task before the shuffle): a rank
 * counts its own reads first and ships (k-mer, partial count) PAIRS, 16 bytes {k-mer, count}, one per
 * distinct k-mer of the rank instead of one unit per instance (k <= 31).
 *   rfx_dev_combine_reads         reads -> every distinct canonical k-mer with its local count, no filter,
 *                                 grouped by owner = mulhi(kmer_hash(k-mer), n_owners) (bucket o =
 *                                 d_out_pairs[owner_off[o] .. owner_off[o+1]), *out_n pairs in all).  Both
 *                                 d_scratch_pairs and d_out_pairs hold cap_pairs pairs; RFX_E_CAP with
 *                                 *out_n = the capacity needed when that is short
 *   rfx_dev_bucket_pairs_by_owner the grouping step alone (pairs with count 0 are dropped)
 *   rfx_dev_merge_pairs           the owner's half: sum the partial counts per k-mer, then
 *                                 KmerCoverageFilter (P/ReflexivMain.java:3115-3119), ascending order */
int rfx_dev_combine_reads(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int words_per_read, int read_len,
                          int k, int front_clip, int end_clip, int n_owners, void *d_scratch_pairs, void *d_out_pairs,
                          int64_t cap_pairs, int64_t *d_owner_off, int64_t *h_owner_off, int64_t *out_n,
                          int64_t *out_instances);
int rfx_dev_bucket_pairs_by_owner(rfx_ctx *ctx, const void *d_pairs, int64_t n_pairs, int n_owners, void *d_out_pairs,
                                  int64_t *d_owner_off, int64_t *h_owner_off);
int rfx_dev_merge_pairs(rfx_ctx *ctx, const void *d_pairs, int64_t n_pairs, int k, int min_cov, int max_cov, int twin,
                        uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap, int64_t *out_n,
                        int64_t *out_distinct);

/* ---- the count stage on several GPUs of one node: the shuffle of `reduceByKey` (P/ReflexivMain.java:155, map-side
 * combine included) / `groupBy("value").count()` (P/ReflexivDSMain.java:207-209) as an all-to-all(v) over RCCL / xGMI.
 * One process or thread per GPU, each with its own rfx_ctx and one rfx_comm.  The k-mer space is radix-sharded by the
 * owner of each k-mer's minimiser; what crosses the links are super-k-mer records (16 B per run of windows for
 * k = 21..31, 32 B for k = 33..63: 2.6 / 5.4 bytes per k-mer instance).  RCCL is bound at run time (dlopen): the host
 * process's own RCCL when it has one, /opt/rocm/lib/librccl.so.1 otherwise; RFX_E_NOGPU when there is none.
 *   rfx_comm_unique_id      rank 0 makes the 128-byte id; the host hands it to every rank (Spark: a broadcast variable)
 *   rfx_comm_init           collective: every rank calls it with the same id, its rank and the world size (<= 64)
 *   rfx_comm_all_reduce_i64 sum (op 0) / max (op 1) of up to 8 host int64 over the ranks, in place (count() of the
 *                           stop rule, totals, a barrier)
 *   rfx_dev_sharded_count   collective: this rank's packed reads in HBM (d_read_len: per-read lengths for ragged reads,
 *                           k = 21..31 and 33..125, read_len their maximum; or NULL = every read has read_len bases) -> its shard of the filtered (k-mer, count) list,
 *                           ascending (d_out_counts: int32 for k <= 31, int64 beyond, as the fused calls; k / 32 + 1 words per
 *                           key).  k = 21..31 and 33..63 exchange super-k-mer records in generations; every other k of the
 *                           counters (3..20, 65..125; not a multiple of 32) exchanges its k-mer instances in one go (at
                           65..125 bucketed by owner straight from the reads and counted with the bucketed path);
 *                           out_totals[3] = instances, distinct, survivors over ALL ranks.  `generations` (1..8) cuts
 *                           the hash space so that generation g is counted while g+1.. travel.  RFX_E_CAP -- on
 *                           EVERY rank when the shard of ANY rank did not fit -- with *out_n = what this rank needs.
 *   rfx_dev_gather_shards   collective: every rank's shard to rank `root`, shard after shard in rank order
 * Environment: RFX_COMM_LIMIT_BYTES (per peer and call, default 512 MiB), RFX_COMM_SELF_VIA_RCCL=1 (tests: the rank's own
 * bucket through ncclSend / ncclRecv instead of a device copy). */
typedef struct rfx_comm rfx_comm;
int rfx_comm_unique_id(uint8_t *id128);
int rfx_comm_init(rfx_ctx *ctx, const uint8_t *id128, int rank, int world, rfx_comm **out);
void rfx_comm_destroy(rfx_comm *comm);
int rfx_comm_rank(const rfx_comm *comm);
int rfx_comm_world(const rfx_comm *comm);
int64_t rfx_comm_last_bytes_bucketed(const rfx_comm *comm);
int rfx_comm_all_reduce_i64(rfx_comm *comm, int64_t *h_vals, int n, int op);
int rfx_dev_sharded_count(rfx_ctx *ctx, rfx_comm *comm, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads,
                          int words_per_read, int read_len, int k, int front_clip, int end_clip, int generations, int min_cov,
                          int max_cov, int twin, uint64_t *d_out_keys, void *d_out_counts, int64_t cap, int64_t *out_n,
                          int64_t *out_totals);
/* The extend stage on several GPUs -- every sortByKey of the reference's driver (P/ReflexivMain.java:179,191,211,235,247,286;
 * k > 31: P/ReflexivDSMain64.java:504-563) as a range shuffle of whole records over RCCL: local stable sort, rank splitters
 * from ONE all-gather of a device-built sample, one count matrix, one all-to-all(v), local stable sort; the order contract's
 * logical partitions are cut out of the GLOBAL sorted sequence (any prm->partitions with any number of ranks: a partition may
 * go on on the next rank, the parity it brings along travels in one small all-gather); count() of the stop
 * rule and the trace are one all-reduce per pass.  d_keys / d_counts: this rank's shard of the filtered (k-mer, count) list
 * in HBM, any order (k <= 31: one word per k-mer, as rfx_dev_assemble; k = 32..124: (k-1)/31+1 words of 31 bases, as
 * rfx_dev_assemble_w).  The record set stays sharded while it has more than `gather_below` records over all ranks
 * (< 0: RFX_SHARD_GATHER_BELOW or 32 Mi; 0: to the end of the loop); then -- and before the k > 31 from-counts extras -- it is
 * gathered on rank 0, where the one-GPU driver takes the loop up.  The contig text (identical to rfx_dev_assemble[_w] on one
 * GPU for the same prm->partitions), *out_contigs and the trace arrive on rank 0 (*out_len = 0 elsewhere).  Collective: a
 * failure of any rank fails the call on every rank (RFX_E_STATE on the others), and RFX_E_CAP -- the text buffer of rank 0
 * is too short -- comes back on EVERY rank with *out_len = the length needed, so that retries re-enter together. */
int rfx_dev_sharded_assemble(rfx_ctx *ctx, rfx_comm *comm, const uint64_t *d_keys, const int32_t *d_counts, int64_t n,
                             const rfx_params *prm, int64_t gather_below, char *out, int64_t cap, int64_t *out_len,
                             int64_t *out_contigs, int64_t *trace, int64_t trace_cap, int64_t *n_trace);
/* The whole resident path on several GPUs from ASCII reads in host memory (the multi-GPU rfx_assemble_reads; what one
 * Spark executor per GPU calls with ITS partition of the reads): upload + 2-bit encode (any read lengths), the sharded
 * count above, then rfx_dev_sharded_assemble (gather_below as there: a bacterial genome's survivors go to rank 0 at once,
 * a record set that does not fit one GPU stays sharded).  The contig text arrives on rank 0 (*out_len = 0 on the others;
 * RFX_E_CAP on every rank, see there).  k = 21..31, and k = 33..124 as rfx_assemble_reads takes it (int64 counts, then
 * KmerBinarizer + the count filter on every rank's shard, then the k > 31 driver on (k-1)/31+1-word keys).  Collective. */
int rfx_sharded_assemble_reads(rfx_ctx *ctx, rfx_comm *comm, const uint8_t *bases, const int64_t *read_off, int64_t n_reads,
                               const rfx_params *prm, int generations, int64_t gather_below, char *out, int64_t cap,
                               int64_t *out_len, int64_t *out_contigs, int64_t *trace, int64_t trace_cap, int64_t *n_trace,
                               int64_t *out_totals);
int rfx_dev_gather_shards(rfx_ctx *ctx, rfx_comm *comm, const uint64_t *d_keys, const void *d_counts, int64_t n,
                          int key_words, int count_bytes, int root, uint64_t *d_out_keys, void *d_out_counts, int64_t cap,
                          int64_t *out_n);

/* ---- the record operators on sets that STAY in HBM (the multi-GPU extend stage: reflexiv_amd/dist.py puts the RCCL
 * all-to-all of whole records between them).  Same operators, same reference classes as the host
 * entry points above; here every pointer inside rfx_records, every part_start and the k-mer / count arrays are DEVICE
 * pointers.  Inputs: in->n records, in->need_words = ext_off[n] (the value the producing call reported), key_words
 * as above.  Outputs: caller-allocated arrays of cap_n records / cap_words words (ext_off: cap_n + 1); on return
 * n / need_n / need_words are set (host fields); RFX_E_CAP when a capacity is short.  All run on the context's stream
 * and return after it has drained. */
int rfx_dev_rc_expand_subkmer(rfx_ctx *ctx, const uint64_t *d_kmers, const int32_t *d_counts, int64_t n, int k,
                              rfx_records *d_out);
int rfx_dev_sort_records(rfx_ctx *ctx, const rfx_records *d_in, int P, int k, rfx_records *d_out, int64_t *d_part_start);
int rfx_dev_fork_filter(rfx_ctx *ctx, int reflected, const rfx_records *d_in, const int64_t *d_part_start, int P, int k,
                        int min_error_cov, int twin, rfx_records *d_out, int64_t *d_out_part_start);
int rfx_dev_reflect_from_forward(rfx_ctx *ctx, const rfx_records *d_in, int k, rfx_records *d_out);
int rfx_dev_random_reflection(rfx_ctx *ctx, const rfx_records *d_in, const int64_t *d_part_start, int P, int k,
                              rfx_records *d_out);
int rfx_dev_extend_pass(rfx_ctx *ctx, const rfx_records *d_in, const int64_t *d_part_start, int P, int k, int twin,
                        int stage, int scramble, rfx_records *d_out, int64_t *d_out_part_start);
/* positions of m values in n ascending one-word keys: d_out[j] = number of keys < values[j] (upper = 0) or <= (upper = 1)
 * -- the splitter search of the range shuffle that stands in for sortByKey's range partitioner */
int rfx_dev_lower_bound(rfx_ctx *ctx, const uint64_t *d_sorted_keys, int64_t n, const uint64_t *d_values, int64_t m,
                        int upper, int64_t *d_out);

/* Whole driver  P/ReflexivMain.java:168-310 (DS :221-352) from the filtered, ascending
 * (kmer,count) list in HBM to the contig text in host memory.  trace (optional) receives
 * the record count after every extend pass. */
int rfx_dev_assemble(rfx_ctx *ctx, const uint64_t *d_keys, const int32_t *d_counts, int64_t n,
                     const rfx_params *prm, char *out, int64_t cap, int64_t *out_len,
                     int64_t *out_contigs, int64_t *trace, int64_t trace_cap, int64_t *n_trace);

/* k = 33..127 (not 64 or 96): put (k/32+1-word k-mer, count) pairs that are in any order (e.g. the shards of the hash-partitioned count
 * gathered from several GPUs) into ascending k-mer order in place -- the order rfx_dev_count_reads_w returns and the
 * from-counts driver expects (order contract: ascending by base string). */
int rfx_dev_order_kmers_w(rfx_ctx *ctx, uint64_t *d_keys, int64_t *d_counts, int64_t n, int k);

/* KmerBinarizer.call + the count filter of the from-counts driver (P/ReflexivDSMain64.java:10772-10836, :473-478) for
 * k-mers that never left HBM: the counter's output (k/32+1 words of 32 bases per k-mer, int64 counts, ascending) ->
 * the assembler's input ((k-1)/31+1 words of 31 bases, int32 counts read as the CSV text would be: 10 digits or more
 * = 1000000000), keeping min_cov <= count <= max_cov.  Output buffers hold n entries.  All device pointers. */
int rfx_dev_counter_to_asm(rfx_ctx *ctx, const uint64_t *d_keys32, const int64_t *d_counts64, int64_t n, int k,
                           int min_cov, int max_cov, uint64_t *d_out_kmers, int32_t *d_out_counts, int64_t *out_n);

/* Whole k > 31 driver ReflexivDSMain64.assemblyFromKmer (P/ReflexivDSMain64.java:458-826) from the filtered, ascending
 * (k-mer, count) list in HBM (assembler layout) to the contig text.  prm->extras = 1 (default): at iteration
 * minimumIteration + 3 the records are doubled into both orientations and split into the members of mergeable pairs
 * and the rest (:584-619), only the first set is iterated further (:621-661), and after the loop the two are united and
 * records that share an end with a longer one are dropped (:672-712).  prm->extras = 0: the loop iterates all records.
 * Stop rule: checked from minimumIteration + 3 on, the first repeat of the count sets param.scramble = 3 (later passes
 * start their emission marker at 1), the second stops. */
int rfx_dev_assemble_w(rfx_ctx *ctx, const uint64_t *d_kmers, const int32_t *d_counts, int64_t n,
                       const rfx_params *prm, char *out, int64_t cap, int64_t *out_len,
                       int64_t *out_contigs, int64_t *trace, int64_t trace_cap, int64_t *n_trace);

/* The same driver from HOST arrays (what `run -kmerc COUNTS -kmer 63` holds after KmerBinarizer and the count filter,
 * P/ReflexivDSMain64.java:458-478): n k-mers of (k-1)/31+1 words each, ascending, with their int32 counts. */
int rfx_assemble_counts_w(rfx_ctx *ctx, const uint64_t *kmers, const int32_t *counts, int64_t n,
                          const rfx_params *prm, char *out, int64_t cap, int64_t *out_len,
                          int64_t *out_contigs, int64_t *trace, int64_t trace_cap, int64_t *n_trace);

/* The whole resident path from ASCII reads in host memory (any lengths) to the contig text:
 * upload, 2-bit encode, extract + count + filter (prm->min_cov .. max_cov), the driver above --
 * nothing but the reads goes up and nothing but the text comes back.  k <= 31, and k = 33..125 (not 64 or 96): the reference's two-step
 * route there (`counter -kmer K` then `run -kmerc ... -kmer K`): rfx_dev_count_reads_w (_ragged_w for reads of different
 * lengths) with the min_cov .. max_cov filter, rfx_dev_counter_to_asm with the same bounds, rfx_dev_assemble_w.
 * out_kept (optional) = number of k-mers that passed the coverage filter(s): those handed to the driver. */
int rfx_assemble_reads(rfx_ctx *ctx, const uint8_t *bases, const int64_t *read_off, int64_t n_reads,
                       const rfx_params *prm, char *out, int64_t cap, int64_t *out_len,
                       int64_t *out_contigs, int64_t *trace, int64_t trace_cap, int64_t *n_trace,
                       int64_t *out_kept);

/* Contig RC de-duplication: P/ReflexivDSDynamicKmerDedup.java `assemblyFromKmer` (:138-339) -- three rounds of
 * marker 31-mers (ReverseComplementKmerMarkerExtraction :2674-3096, ForwardAndReverseComplementKmerMarkerExtraction :2206-2673)
 * -> sort -> DSMarkerKmerSelection (:1788-1870) -> groupBy().count() >= 2 -> DSMarkerKmerShorterID (:3186-3207) ->
 * DSShorterRCContigSeqAndTargetExtraction (:3097-3132) -> DSShorterRCContigRemoval (:1405-1558) /
 * DSShorterForwardAndRCContigRemoval[Array] (:508-729, :959-1175), then TagRowContigDSID (:3397-3443).  The fixed-k path
 * emits every contig on both strands; this reports each once (and merges overlapping pieces as the reference does).
 *   rfx_dedup_contigs      contigs as ASCII bases + offsets (ids = positions, as zipWithIndex numbers them) -> the survivors
 *                          (ASCII + offsets; RFX_E_CAP when a capacity is short) and / or the text: ">Contig-<len>-<idx>" +
 *                          the sequence in lines of 10,000,000, contigs of at least min_contig bases; round_n[3] (optional)
 *                          = contigs left after each round
 *   rfx_dedup_contig_text  the same from the contig text the path writes (either twin's headers, 100-column lines) */
int rfx_dedup_contigs(rfx_ctx *ctx, const uint8_t *bases_ascii, const int64_t *contig_off, int64_t n_contigs, int min_contig,
                      uint8_t *out_bases_ascii, int64_t cap_bases, int64_t *out_off, int64_t cap_contigs, int64_t *out_n,
                      char *text, int64_t text_cap, int64_t *text_len, int64_t *round_n);
int rfx_dedup_contig_text(rfx_ctx *ctx, const char *contig_text, int64_t len, int min_contig, char *out, int64_t cap,
                          int64_t *out_len, int64_t *out_contigs, int64_t *round_n);

/* The same de-duplication on a PACKED contig set that stays in HBM.  Every pointer of rfx_contigs_packed
 * is a DEVICE pointer into arrays the caller allocated; the struct itself lives on the host.  Bases are 2 bits each, 32 to a
 * word, the first in the two highest bits -- the convention of the 2-bit read store and of rfx_dyn_packed --, codes A0 C1 G2,
 * anything else 3 (nucleotideValue), so a letter that is not ACGT comes back as T.  Every contig starts on a word and
 * word_off[0] = 0.  INVARIANT: every bit past a contig's last base is 0; every producer writes those bits (it never relies on
 * zeroed memory).  The two host forms above are pack (or from-text) -> these kernels -> unpack / to-text.
 *   rfx_dev_contigs_pack       host ASCII + offsets -> the packed set; needs cap_n >= n and cap_words >= n + bases / 32 at most
 *   rfx_dev_contigs_unpack     the packed set -> host ASCII + offsets (*out_n contigs; RFX_E_CAP when a capacity is short,
 *                              nothing written but *out_n)
 *   rfx_dev_contigs_from_text  the contig text the path writes, already in HBM (d_text, len bytes) -> the packed set: a line
 *                              that begins with '>' opens a contig, every other line behind the first header is that contig's
 *                              bases at any line width, '\r' is dropped, lines ahead of the first header are ignored, a header
 *                              followed by a header or by the end is a contig of 0 bases that keeps its position (ids are
 *                              positions).  Needs cap_n >= the headers and cap_words >= headers + len / 32 at most; a text of
 *                              2^32 bytes or more: RFX_E_LIMIT
 *   rfx_dev_contigs_to_text    TagRowContigDSID + changeLine (:3397-3443) into a device buffer: ">Contig-<len>-<idx>\n" + the
 *                              sequence in lines of 10,000,000 bases for the contigs of at least min_contig bases, idx = the
 *                              position among ALL contigs of the set; *out_len = the text's length, *out_contigs (optional) =
 *                              the contigs written; text-buffer rule: filled up to cap, nothing at or past it, RFX_E_CAP with
 *                              *out_len = the need
 *   rfx_dev_dedup_contigs      the three rounds, packed in, packed out; round_n[3] (optional, host) = contigs left after each
 * CAPACITY of rfx_dev_dedup_contigs: a merge of a and b bases needs ceil((a+b)/32) <= ceil(a/32) + ceil(b/32) words and removes a
 * contig, so an output with cap_n >= in.n and cap_words >= in.word_off[in.n] suffices whenever no marker row is left over.  A
 * leftover marker row (a contig named by two or more candidate pairs of one round) adds a contig of at most 62 bases = 2
 * words.  A contig of at least 300 bases is named by at most 155 candidate pairs a round (310 probe rows, two per pair), which
 * leave at most 77 rows; rows are shorter than 300 bases and never probe, and the contigs of at least 300 bases never grow in
 * number.  So with n300 = the input contigs of at least 300 bases, cap_n >= in.n + 231 * n300 and cap_words >=
 * in.word_off[in.n] + 462 * n300 ALWAYS suffice.  On a short output: RFX_E_CAP with need_n / need_words set -- what to call
 * again with -- and no output array written.
 * All run on the context's stream and return after it has drained.  A null pointer, a negative count, or an input whose
 * word_off and len disagree: RFX_E_ARG; 2^32 marker rows or 2^30 merges in one step: RFX_E_LIMIT.  n = 0 is valid everywhere. */
typedef struct {
    int64_t   n;
    uint64_t *words;     /* contig i = words [word_off[i], word_off[i+1]) */
    int64_t  *word_off;  /* n + 1 entries, in WORDS: every contig starts on a word */
    int64_t  *len;       /* bases; word_off[i+1] - word_off[i] = (len[i] + 31) / 32 */
    int64_t   cap_n, cap_words, need_n, need_words;
} rfx_contigs_packed;    /* every pointer is a DEVICE pointer, the struct lives on the host */
int rfx_dev_contigs_pack(rfx_ctx *ctx, const uint8_t *bases_ascii, const int64_t *contig_off, int64_t n, rfx_contigs_packed *d_out);
int rfx_dev_contigs_unpack(rfx_ctx *ctx, const rfx_contigs_packed *d_in, uint8_t *out_bases_ascii, int64_t cap_bases, int64_t *out_off,
                           int64_t cap_contigs, int64_t *out_n);
int rfx_dev_contigs_from_text(rfx_ctx *ctx, const char *d_text, int64_t len, rfx_contigs_packed *d_out);
int rfx_dev_contigs_to_text(rfx_ctx *ctx, const rfx_contigs_packed *d_in, int min_contig, char *d_text, int64_t cap, int64_t *out_len,
                            int64_t *out_contigs);
int rfx_dev_dedup_contigs(rfx_ctx *ctx, const rfx_contigs_packed *d_in, rfx_contigs_packed *d_out, int64_t *round_n);

/* The dynamic-k record format and passes: P/ReflexivDSDynamicKmerFirstFour.java (DSkmerRandomReflection
 * :2509-2762, DSExtendReflexivKmer :1581-2373) and P/ReflexivDSDynamicKmerIteration.java (DSExtendReflexivKmerToArrayLoop
 * :465-1249) -- the "meta" assembler's passes on keys of ANY length (a (k-1)-mer of whichever k the reduction kept).  In
 * a Row a key is left-aligned 31-base blocks with a 01 terminator, the attribute one long (marker << 62 | left << 32 |
 * right, negatives as 30000 - v), the extension in the same left-aligned form; across this boundary a record set is base
 * CODES (A0 C1 G2 T3, one byte per base) with offsets + marker / left / right (left / right as the reference reads them
 * back: clamped to +-30000).  Two keys meet when they are equal OR one is a prefix of the other; the forward record must
 * not be the shorter one; the merged key keeps the longer key's length.
 *   rfx_dyn_sort               sort("k-1") as Spark orders array<long> (element by element as signed longs, a proper prefix
 *                              first), stable, + the cut into P logical partitions (floor(p*n/P) moved past equal keys)
 *   rfx_dyn_random_reflection  DSkmerRandomReflection.call on the given partitions
 *   rfx_dyn_extend_pass        one pass over sorted records: stage 0 DSExtendReflexivKmer (extension in one long),
 *                              1 DSExtendReflexivKmerToArrayLoop (start_iteration = param.startIteration: from 61 on a
 *                              shorter forward record is dropped); start_marker 2, or 1 when param.scramble == 3
 *   rfx_dyn_run                the drivers with the records resident in HBM between the operators:
 *                              FirstFour.assemblyFromKmer (:137-224) = random_reflection 1, passes_first_four 4, no
 *                              iterations (end < start); Iteration.assemblyFromKmer (:134-205) = iterations start..end
 * Outputs: caller-allocated arrays of cap_n records / cap_key / cap_ext bases; n / need_key / need_ext are set; RFX_E_CAP
 * when a capacity is short.  Keys of more than 124 bases: RFX_E_LIMIT from each of the four (the reference's k-mer list ends
 * at 95); P outside 1..63: RFX_E_ARG.  A call that returns either writes nothing. */
typedef struct {
    int64_t n;
    uint8_t *key; int64_t *key_off;      /* key i = key[key_off[i] .. key_off[i+1]) */
    uint8_t *ext; int64_t *ext_off;
    int32_t *marker, *left, *right;
    int64_t cap_n, cap_key, cap_ext, need_key, need_ext;
} rfx_dyn_records;
/* DynamicKmerBinarizerFromReducedToSubKmer (P/ReflexivDSDynamicKmerFirstFour.java:2931-3016 and Iteration's twin) on the device: the
 * text rows of the hand-over files -> records.  text + row_off[n_rows + 1]: row i = text[row_off[i], row_off[i+1]), its fields joined
 * by ',' (a trailing newline is ignored).  form 0: (k-mer, "m|l|r") -> key = the k-mer without its last base, extension = that base,
 * orientation 1; form 1: (sub-k-mer, "m|l|r", extension).  A leading '(' / trailing ')' of the tuple text is dropped; left / right
 * clamped to +-30000 as the reference reads its attribute long back (:2340-2366).  Outputs as for the other rfx_dyn_* calls. */
int rfx_dyn_binarize(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int form, rfx_dyn_records *out);
int rfx_dyn_sort(rfx_ctx *ctx, const rfx_dyn_records *in, int P, rfx_dyn_records *out, int64_t *part_start);
int rfx_dyn_random_reflection(rfx_ctx *ctx, const rfx_dyn_records *in, const int64_t *part_start, int P, rfx_dyn_records *out);
int rfx_dyn_extend_pass(rfx_ctx *ctx, const rfx_dyn_records *in, const int64_t *part_start, int P, int stage, int start_iteration,
                        int start_marker, rfx_dyn_records *out, int64_t *out_part_start);
int rfx_dyn_run(rfx_ctx *ctx, const rfx_dyn_records *in, int P, int random_reflection, int passes_first_four, int start_iteration,
                int end_iteration, rfx_dyn_records *out, int64_t *trace, int64_t trace_cap, int64_t *n_trace);
/* the Row form of the layout, for the shim that converts: blocks <-> base codes, the attribute long <-> its three ints */
int rfx_dyn_blocks_to_bases(const int64_t *blocks, int n_blocks, uint8_t *out, int cap);
int rfx_dyn_bases_to_blocks(const uint8_t *bases, int n, int64_t *out, int cap);
int64_t rfx_dyn_attribute(int marker, int left, int right);
void rfx_dyn_attribute_unpack(int64_t attribute, int *marker, int *left, int *right);

/* The same passes on a PACKED record set that stays in HBM.  Every pointer of rfx_dyn_packed is a DEVICE
 * pointer into arrays the caller allocated; the struct itself lives on the host.  Bases are 2 bits each, 32 to a word, the
 * first in the two highest bits -- the convention of the 2-bit read store (rfx_dev_encode_reads).  INVARIANT: every bit past
 * a key's or an extension's last base is 0, and so is every unused key word; every producer writes those bits (it never
 * relies on zeroed memory) and every consumer compares whole words.  Keys hold at most 124 bases in RFX_DYN_KEY_WORDS words.
 * CAPACITY: no pass needs more records or more extension words than its input -- a flip keeps both lengths (the same
 * multiset of extension lengths, the same word count), a merge of extensions of a and b bases gives ceil((a+b)/32) <=
 * ceil(a/32) + ceil(b/32) words -- so an output with cap_n >= in.n and cap_words >= in.ext_off[in.n] always suffices for
 * sort, random reflection, extend pass and run; rfx_dev_dyn_pack needs cap_words >= n + ext bases / 32 at most,
 * rfx_dev_dyn_binarize cap_words >= n_rows + text bytes / 32 at most.
 *   rfx_dev_dyn_pack / _unpack    host base codes (rfx_dyn_records) <-> the packed set
 *   rfx_dev_dyn_binarize          rfx_dyn_binarize with the text and the row offsets (n_rows + 1, into d_text) in HBM
 *   rfx_dev_dyn_sort / _random_reflection / _extend_pass / _run
 *                                 operator for operator and argument for argument the host forms above; part starts are
 *                                 device arrays of P + 1 entries, `trace` is a host array
 *   rfx_dev_dyn_to_text           DSBinarySubKmerWith{Short,Long}ExtensionToString (FirstFour:226-263): rows
 *                                 "SUBKMER,marker|left|right,EXTENSION\n" into a device buffer; *out_len = the text's length
 *   rfx_dyn_run_text              host text in, host text out, everything between packed and in HBM: upload, binarize
 *                                 (form 0 / 1), run, to-text, one copy back -- for the dynamic-k passes what rfx_assemble_reads
 *                                 is for the fixed path
 * All run on the context's stream and return after it has drained.  P outside 1..63, a null pointer, a bad form / stage /
 * start_marker: RFX_E_ARG; a key of more than 124 bases: RFX_E_LIMIT (pack, binarize and every operator); a short output:
 * RFX_E_CAP with n / need_words (or *out_len) set.  In each of these cases no output array was written, except that the two
 * text buffers follow the text-buffer rule (filled up to cap, nothing at or past it).  n = 0 is valid everywhere. */
#define RFX_DYN_KEY_WORDS 4
typedef struct {
    int64_t   n;
    uint64_t *key;      /* n * 4 words; base j of key i in key[4*i + j/32] at bits 63-2*(j%32)..62-2*(j%32)   */
    uint8_t  *key_len;  /* bases, <= 124                                                                    */
    uint64_t *ext;      /* record i = words [ext_off[i], ext_off[i+1]), same 32-bases-per-word form         */
    int64_t  *ext_off;  /* n + 1 entries, in WORDS: every extension starts on a word                        */
    int32_t  *ext_len;  /* bases; ext_off[i+1] - ext_off[i] = (ext_len[i] + 31) / 32                         */
    int32_t  *marker, *left, *right;
    int64_t   cap_n, cap_words, need_words;
} rfx_dyn_packed;       /* every pointer is a DEVICE pointer */
int rfx_dev_dyn_pack(rfx_ctx *ctx, const rfx_dyn_records *host_in, rfx_dyn_packed *d_out);
int rfx_dev_dyn_unpack(rfx_ctx *ctx, const rfx_dyn_packed *d_in, rfx_dyn_records *host_out);
int rfx_dev_dyn_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, int form, rfx_dyn_packed *d_out);
int rfx_dev_dyn_sort(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int P, rfx_dyn_packed *d_out, int64_t *d_part_start);
int rfx_dev_dyn_random_reflection(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const int64_t *d_part_start, int P, rfx_dyn_packed *d_out);
int rfx_dev_dyn_extend_pass(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const int64_t *d_part_start, int P, int stage, int start_iteration,
                            int start_marker, rfx_dyn_packed *d_out, int64_t *d_out_part_start);
int rfx_dev_dyn_run(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int P, int random_reflection, int passes_first_four, int start_iteration,
                    int end_iteration, rfx_dyn_packed *d_out, int64_t *trace, int64_t trace_cap, int64_t *n_trace);
int rfx_dev_dyn_to_text(rfx_ctx *ctx, const rfx_dyn_packed *d_in, char *d_text, int64_t cap, int64_t *out_len);
int rfx_dyn_run_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int form, int P, int random_reflection,
                     int passes_first_four, int start_iteration, int end_iteration, char *out, int64_t cap, int64_t *out_len, int64_t *trace,
                     int64_t trace_cap, int64_t *n_trace);

/* The k-mer sorting stage (Count_<k>_sorted) on the same PACKED record sets in HBM:
 * P/ReflexivDSKmerLeftAndRightSorting.java `assemblyFromKmer` (:105-243) with param.bubble == true and param.minErrorCoverage > 0.
 * It is the link between the counter's `KMER,count` rows and the `KMER,marker|left|right` rows rfx_dyn_binarize form 0 reads.
 *   rfx_dev_ksort_binarize     steps 1-4: DynamicKmerBinarizer (:1666-1764; a leading '(' of the k-mer and a trailing ')' of the
 *                              count dropped, A0 C1 G2 anything else 3, a count of 10 or more digits reads as 1,000,000,000),
 *                              filter(count <= maxKmerCoverage) (:178-184; no lower bound, as in the reference),
 *                              DSKmerReverseComplement (:1569-1664), DSForwardSubKmerExtraction (:906-979): two records per kept
 *                              row, the k-mer's and then its reverse complement's, in row order; key = the k-mer without its last
 *                              base, extension = that base, marker 1, left = right = the count clamped to 30000
 *   rfx_dev_ksort_fork_filter  reflected 0: DSFilterForkSubKmerWithErrorCorrection (:426-624), 1:
 *                              DSFilterForkReflectedSubKmerWithErrorCorrection (:693-904) over a SORTED set (rfx_dev_dyn_sort, any P):
 *                              one survivor per run of equal keys
 *   rfx_dev_ksort_reflect      step 6, DSReflectedSubKmerExtractionFromForward (:1096-1179): key' = key[1:] + extension,
 *                              extension' = key[0], marker 2
 *   rfx_dev_ksort_full_kmers   step 8, DSSubKmerToFullKmer (:1301-1568): marker 2 extension + key, marker 1 key + extension; the
 *                              result has key = the k-mer, no extension (ext_len 0), marker 1
 *   rfx_dev_ksort_to_text      step 9, DSBinaryFullKmerArrayToString (:246-354): rows "KMER,1|left|right\n" of the records whose key
 *                              has k bases into a device buffer; *out_len = the text's length, *n_out = its rows; d_row_off
 *                              (nullable, a device array of d_in->n + 1 entries at least) receives the n_out + 1 row offsets, so
 *                              that d_text and d_row_off can go straight to rfx_dev_dyn_binarize form 0
 *   rfx_dev_ksort_run          steps 1-8 with the set resident between the operators (the two sort("k-1") are rfx_dev_dyn_sort's);
 *                              bubble == 0 skips steps 5-7, as the driver does (:195)
 *   rfx_ksort_text             host text in, host text out: upload, run, to-text, one copy back
 * SUPPORTED k: 8..124 (the sub-k-mer and the k-mer held as a key fit the 124-base key) except (k - 1) % 31 == 0, i.e. 32, 63 and
 * 94, where the reference's own classes are broken (DSForwardSubKmerExtraction special-cases currentSubKmerSize == 31 only, and
 * wrongly: tests/golden/ksort_vectors.npz `refused_k`).  Those and k outside 8..124: RFX_E_ARG.
 * DEVIATIONS, both stated: (1) one call handles ONE k -- a row whose k-mer has another length is dropped at the binarizer; the
 * reference would carry a row of another LISTED length through both folds (where subKmerSlotComparator on block arrays of
 * unequal length is not well defined) and drop it at step 9; its own pipeline never writes a mixed file.  (2) A count with a sign
 * is refused (Integer.parseInt would take it).  The folds reset at every new key and equal keys never straddle a Spark range
 * partition, so the stage takes no partition count.
 * CONTRACTS.  Every output set keeps the rfx_dyn_packed invariant (every bit past the last base 0, every unused key word 0; the
 * producers write those bits).  Capacities from the input alone: binarize and run cap_n >= 2 n_rows and cap_words >= 2 n_rows
 * (a one-base extension takes one word); the other operators cap_n >= in.n and cap_words >= in.ext_off[in.n]; full_kmers' (and
 * run's) cap_words may be 0.  A short output: RFX_E_CAP with n and need_words (or *out_len) set and no output array written; the
 * two text buffers follow the text-buffer rule (filled up to cap, nothing at or past it).  RFX_E_ARG, nothing written: a row
 * without a comma; a count field that is not 1 or more decimal digits, optionally followed by ')' (the reference throws) -- both
 * for EVERY row, kept or dropped; min_error_cov <= 0 (the reference's classes without error correction read a long column with
 * getInt and cannot run); min_repeat_fold < 1; max_k < 1; a null pointer; for fork_filter and reflect a set whose keys are not
 * all of one length; for fork_filter, reflect and full_kmers a record whose extension is not one base.  n_rows = 0 and n = 0 are
 * valid everywhere.  Row ends follow rfx_dyn_binarize's rule: a trailing newline is ignored.  All run on the context's stream
 * and return after it has drained. */
typedef struct {
    int    k;                /* the k of this call                                                               */
    int    max_k;            /* the LAST k of the k list (param.kmerListInt): the markers are max_k + 3          */
    int    min_error_cov;    /* minErrorCoverage, E                                                              */
    int    max_cov;          /* maxKmerCoverage                                                                  */
    int    bubble;           /* param.bubble                                                                     */
    double min_repeat_fold;  /* minRepeatFold, F: compared in double                                             */
} rfx_ksort_params;
void rfx_ksort_default_params(rfx_ksort_params *p, int k);   /* max_k 95, E 8, max_cov 10000000, F 1.5, bubble 1 */
int rfx_dev_ksort_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const rfx_ksort_params *params,
                           rfx_dyn_packed *d_out);
int rfx_dev_ksort_fork_filter(rfx_ctx *ctx, int reflected, const rfx_dyn_packed *d_sorted, const rfx_ksort_params *params,
                              rfx_dyn_packed *d_out);
int rfx_dev_ksort_reflect(rfx_ctx *ctx, const rfx_dyn_packed *d_in, rfx_dyn_packed *d_out);
int rfx_dev_ksort_full_kmers(rfx_ctx *ctx, const rfx_dyn_packed *d_in, rfx_dyn_packed *d_out);
int rfx_dev_ksort_to_text(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int k, char *d_text, int64_t cap, int64_t *out_len, int64_t *d_row_off,
                          int64_t *n_out);
int rfx_dev_ksort_run(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const rfx_ksort_params *params,
                      rfx_dyn_packed *d_out);
int rfx_ksort_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, const rfx_ksort_params *params, char *out,
                   int64_t cap, int64_t *out_len);
/* The same stage straight from the counter's arrays in HBM, no text between the counter and the set.
 *   rfx_dev_ksort_from_counts  steps 1-4: EXACTLY the set rfx_dev_ksort_binarize gives for the rows `KMER,count\n` of the n rows of
 *                              (d_keys, d_counts) followed by the rows `KMER,1\n` of the n_extra keys of d_extra_keys (the mercy
 *                              k-mers: duplicates allowed, nothing is merged) -- record for record, every word of the set included
 *   rfx_dev_ksort_run_counts   steps 1-8 behind that binarizer: EXACTLY the set of rfx_dev_ksort_run on those rows
 * KEYS: the counter's format, params->k / 32 + 1 words a row -- k <= 31: one word, the last base in the two lowest bits (what
 * rfx_dev_count_reads_ragged and rfx_dev_mercy_kmers write); k > 31: 32 bases a full word, the first in the two highest bits, and the
 * k % 32 last bases in the lowest bits of the last word (rfx_dev_count_reads_ragged_w).  Whatever the last word holds above its
 * bases is ignored.  The rows are taken in array order (the counter's is ascending; nothing here depends on it).
 * COUNTS: count_bytes 4 (int32, the k <= 31 counter) or 8 (int64, the k > 31 counter).  A count is read as the text path reads its
 * digits: 1,000,000,000 or more behaves as 1,000,000,000; a row is kept when that value is <= max_cov (an extra row when 1 <=
 * max_cov), and left = right = the value clamped to 30000.  A negative count has no text the binarizer takes: RFX_E_ARG.
 * Everything else as rfx_dev_ksort_binarize / _run with n + n_extra in place of n_rows: the supported k (and k % 32 == 0 is refused
 * here, RFX_E_ARG: the counter writes no keys of such a k), the parameter checks, cap_n >= 2 (n + n_extra), cap_words >= 2 (n +
 * n_extra) for from_counts and 0 for run_counts, RFX_E_CAP with n and need_words set and nothing written, n + n_extra = 0 valid,
 * 2^31 rows or more RFX_E_LIMIT.  count_bytes other than 4 or 8, a negative n, a null array where its n > 0: RFX_E_ARG. */
int rfx_dev_ksort_from_counts(rfx_ctx *ctx, const uint64_t *d_keys, const void *d_counts, int count_bytes, int64_t n,
                              const uint64_t *d_extra_keys, int64_t n_extra, const rfx_ksort_params *params, rfx_dyn_packed *d_out);
int rfx_dev_ksort_run_counts(rfx_ctx *ctx, const uint64_t *d_keys, const void *d_counts, int count_bytes, int64_t n,
                             const uint64_t *d_extra_keys, int64_t n_extra, const rfx_ksort_params *params, rfx_dyn_packed *d_out);

/* The k-mer reduction stage (Count_<k1>_reduced and the rewritten Count_<k2>_sorted / Count_<k2>_reduced) on
 * the same PACKED record sets in HBM: P/ReflexivDSDynamicKmerRuduction.java `assemblyFromKmer` (:143-287).  It compares the sorted
 * k-mers of two consecutive k of the k list, k1 < k2, and adjusts markers and variants of the longer ones; its inputs are two texts
 * of the k-mer sorting stage, its outputs feed rfx_dyn_binarize form 0.
 *   rfx_dev_reduce_union          DynamicKmerBinarizerFromSorted (:3175-3303) on both texts (rows "KMER,marker|left|right", a leading
 *                                 '(' and a trailing ')' dropped, A0 C1 G2 anything else 3, left / right clamped to +-30000) and the
 *                                 union (:202): the records of the LONGER text first, then the shorter one's, each in row order;
 *                                 key = the whole k-mer, no extension (ext_len 0), the marker as the text has it
 *   rfx_dev_reduce_left_prepare   LeftLongerToShorterComparisonPreparation (:860-888): key' = the first len - 1 bases REVERSED,
 *                                 extension' = the last base, marker 1
 *   rfx_dev_reduce_adjust         right 0: LeftLongerKmerVariantAdjustment (:1889-2245), 1:
 *                                 RightLongerKmerVariantAdjustmentAndNeutralization (:1203-1574) over a SORTED set (rfx_dev_dyn_sort)
 *                                 and its P partition starts.  A three-row window whose two pending rows are NOT given up at a new
 *                                 key, only at a partition's end -- the result depends on the cuts, so P and the starts are part of
 *                                 the call; d_out_part_start receives the P + 1 starts of the output.  The reference's quirks are
 *                                 kept: the left flush of a long row then a short row that fails the prefix test adds neither; the
 *                                 right adjustment drops the shorter row after a prefix test that holds, and one row of three when
 *                                 extensions coincide; an adjusted row takes the other row's extension and a -1 marker when the
 *                                 other's is negative and its own is not
 *   rfx_dev_reduce_right_prepare  RightLongerToShorterComparisonAndNeutralizationPreparation (:509-545): the key reversed back, joined
 *                                 with the extension (behind it for marker 1, ahead of it otherwise), the first base cut off as the
 *                                 new extension, marker 2; a map, so the partition starts of its input hold for its output
 *   rfx_dev_reduce_full_kmers     DSSubKmerToFullKmer (:2923-2968): as rfx_dev_ksort_full_kmers
 *   rfx_dev_reduce_neutralize     ShorterKmerNeutralization (:2563-2731, the code that is live) over a set of full k-mers SORTED by
 *                                 rfx_dev_dyn_sort and its P partition starts: a row is compared with the last KEPT row of its
 *                                 partition -- equal lengths keep it, a k1-mer that is a prefix of a kept k2-mer is dropped, a k2-mer
 *                                 whose prefix is the kept k1-mer replaces it
 *   rfx_dev_reduce_run            the whole driver, two device texts in, the final set of full k-mers out, resident between the
 *                                 operators (the three sorts are rfx_dev_dyn_sort's with the caller's P).  The two output files are
 *                                 rfx_dev_ksort_to_text of that set with k = k1 and with k = k2 (DSBinaryFullKmerArrayToStringShort /
 *                                 ...Long, :289-316 / :401-428, print what DSBinaryFullKmerArrayToString prints)
 *   rfx_reduce_text               two host texts in, two host texts out: upload, run, to-text twice, one copy back each
 * max_k is the LAST k of the k list: it decides only whether the second output is called Count_<k2>_reduced (k2 == max_k) or
 * Count_<k2>_sorted (:257-283); the callers that write files use it, the records do not depend on it.
 * SUPPORTED k: 8 <= k1 < k2 <= 124 (k2 itself is held as a key).  Unlike the sorting stage's, this stage's classes are sound
 * where k or k - 1 is a multiple of 31 (31, 32, 62, 63, 93, 94 as either member of the pair: tests/golden/reduce_vectors.npz
 * `probe_k`), so no pair inside that range is refused.  Anything else, and max_k < k2: RFX_E_ARG.
 * DEVIATIONS, both stated: (1) one call handles ONE pair -- a row whose k-mer is neither k1 nor k2 long is dropped at the binarizer;
 * the reference would carry a row of another LISTED length through (its own pipeline never writes one).  (2) A malformed attribute
 * reads as rfx_dyn_binarize reads it (a missing number is 0) where the reference throws.
 * CONTRACTS.  Every output set keeps the rfx_dyn_packed invariant.  Capacities from the input alone, no operator emits more rows
 * than it reads: union and run cap_n >= n_short + n_long, cap_words 0; left_prepare, adjust and right_prepare cap_n >= in.n and
 * cap_words >= in.n (a one-base extension takes one word); full_kmers and neutralize cap_n >= in.n, cap_words 0.  A short
 * output: RFX_E_CAP with n and need_words set and nothing written (the part starts neither); rfx_reduce_text with a short buffer:
 * RFX_E_CAP with BOTH lengths set and NEITHER buffer written.  RFX_E_ARG, nothing written: P outside 1..63; a bad pair; a row
 * without a comma; a set with a key length other than the two the operator expects (k1 and k2 for left_prepare and neutralize,
 * k1 - 1 and k2 - 1 for the others) or with extensions other than it expects (none for left_prepare and neutralize, one base for
 * the others); partition starts that do not run from 0 to n without going backwards; a null pointer.  n = 0 is valid everywhere.
 * All run on the context's stream and return after it has drained. */
typedef struct {
    int k1;      /* the shorter k of the pair (param.kmerSize1)                                    */
    int k2;      /* the longer k (param.kmerSize2)                                                 */
    int max_k;   /* the LAST k of the k list: names the second output, nothing else                */
} rfx_reduce_params;
void rfx_reduce_default_params(rfx_reduce_params *p, int k1, int k2);   /* max_k = max(95, k2) */
int rfx_dev_reduce_union(rfx_ctx *ctx, const char *d_text_short, const int64_t *d_row_off_short, int64_t n_short, const char *d_text_long,
                         const int64_t *d_row_off_long, int64_t n_long, const rfx_reduce_params *params, rfx_dyn_packed *d_out);
int rfx_dev_reduce_left_prepare(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_reduce_params *params, rfx_dyn_packed *d_out);
int rfx_dev_reduce_adjust(rfx_ctx *ctx, int right, const rfx_dyn_packed *d_sorted, const int64_t *d_part_start, int P,
                          const rfx_reduce_params *params, rfx_dyn_packed *d_out, int64_t *d_out_part_start);
int rfx_dev_reduce_right_prepare(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_reduce_params *params, rfx_dyn_packed *d_out);
int rfx_dev_reduce_full_kmers(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_reduce_params *params, rfx_dyn_packed *d_out);
int rfx_dev_reduce_neutralize(rfx_ctx *ctx, const rfx_dyn_packed *d_sorted, const int64_t *d_part_start, int P,
                              const rfx_reduce_params *params, rfx_dyn_packed *d_out, int64_t *d_out_part_start);
int rfx_dev_reduce_run(rfx_ctx *ctx, const char *d_text_short, const int64_t *d_row_off_short, int64_t n_short, const char *d_text_long,
                       const int64_t *d_row_off_long, int64_t n_long, int P, const rfx_reduce_params *params, rfx_dyn_packed *d_out);
int rfx_reduce_text(rfx_ctx *ctx, const char *text_short, const int64_t *row_off_short, int64_t n_short, const char *text_long,
                    const int64_t *row_off_long, int64_t n_long, int P, const rfx_reduce_params *params, char *out_short, int64_t cap_short,
                    int64_t *out_len_short, char *out_long, int64_t cap_long, int64_t *out_len_long);
/* The same stage on two PACKED sets of full k-mers, as rfx_dev_ksort_run / rfx_dev_reduce_run return them: no text between the
 * sorter and the reduction or between one pair and the next.
 *   rfx_dev_reduce_union_packed   EXACTLY the set of rfx_dev_reduce_union on the texts rfx_dev_ksort_to_text(d_short, k1) and
 *                                 rfx_dev_ksort_to_text(d_long, k2): the records of d_long whose key has k2 bases, then those of
 *                                 d_short whose key has k1 bases, each in its own order; a record of any other key length is
 *                                 dropped -- so the final set of the pair (k0, k1) is the short input of the pair (k1, k2) as it is
 *   rfx_dev_reduce_run_packed     the whole driver behind that union: EXACTLY the set of rfx_dev_reduce_run on those two texts
 * A field goes through what the text would do to it: the key's bases and nothing behind them, the marker as nine decimal digits
 * hold it, left / right the same and clamped to +-30000; an extension of the input is not read (the text writer prints none).
 * Capacities cap_n >= d_short->n + d_long->n, cap_words 0; RFX_E_CAP with n and need_words set and nothing written.  RFX_E_ARG,
 * nothing written: a bad pair, P outside 1..63, a null pointer or an input set without its arrays.  d_out's arrays must not be
 * the inputs'.  Either input, or both, may be empty. */
int rfx_dev_reduce_union_packed(rfx_ctx *ctx, const rfx_dyn_packed *d_short, const rfx_dyn_packed *d_long, const rfx_reduce_params *params,
                                rfx_dyn_packed *d_out);
int rfx_dev_reduce_run_packed(rfx_ctx *ctx, const rfx_dyn_packed *d_short, const rfx_dyn_packed *d_long, int P,
                              const rfx_reduce_params *params, rfx_dyn_packed *d_out);
/* Full k-mers back to the sub-k-mer records of the dynamic-k passes without their text: d_sets is a HOST
 * array of n_sets (0..64) packed sets of full k-mers, key_lens a host array of as many key lengths (1..124).  The output is, set
 * after set in array order, EXACTLY what rfx_dev_dyn_binarize form 0 gives for the rows rfx_dev_ksort_to_text(d_sets[j],
 * key_lens[j]) writes: of every record whose key has key_lens[j] bases, in set order, key = the k-mer without its last base,
 * extension = that base, marker 1, left / right through their decimal text and clamped to +-30000.  The same set may stand in the
 * array more than once, with another length each time.  Capacities cap_n >= the sum of the sets' n and cap_words the same (a
 * one-base extension takes one word); RFX_E_CAP with n and need_words set and nothing written; RFX_E_ARG, nothing written: n_sets or
 * a key length out of range, a null pointer, a set without its arrays. */
int rfx_dev_dyn_from_kmers(rfx_ctx *ctx, const rfx_dyn_packed *d_sets, const int *key_lens, int n_sets, rfx_dyn_packed *d_out);
/* REDUCE FROM READS in one resident call: Pipelines.reflexivDSDynamicReductionPipe (Pipelines.java:1315-1737,
 * `reflexiv reduce -fastq reads -klist ...`) on the 2-bit read store in HBM, which the caller encodes ONCE (rfx_dev_encode_reads).
 * For every k of klist, in order: (1) rfx_dev_count_reads_ragged (k <= 31) or rfx_dev_count_reads_ragged_w (k > 31) with min_cov,
 * max_cov and the clips; (2) if sensitive and k <= 31, rfx_dev_mercy_kmers on those solid keys; (3) rfx_dev_ksort_run_counts with
 * max_k = the last k of the list and E by the rule below; (4) from the second k on rfx_dev_reduce_run_packed(previous, this, P): the
 * records of k1 bases of its result are Count_<k1>_reduced, the whole result is the next pair's short input, and the last pair's
 * records of k_last bases are Count_<k_last>_reduced.  d_out receives what rfx_dev_dyn_from_kmers makes of all Count_*_reduced in
 * the order of the k list -- the set rfx_dev_dyn_run takes for the first-four passes -- and out_n_per_k (a HOST array of n_k
 * entries) each k's row count.  No text passes between the counter and that set.
 * THE E RULE (Pipelines.java:1412-1416, :1489-1493; the reference mutates param, so it is sticky): sorting the FIRST k of the list
 * sets E = 3 min_cov iff (k >= 61 and the second k < 81) or k >= 81; sorting any later k sets it iff k >= 61; once set it stays
 * set; until then E = min_error_cov.
 * DEVIATION, stated: the reference reads the glob Count_*_reduced (Pipelines.java:857), whose order differs from the list's once a
 * list reaches k >= 100 (Count_101 sorts ahead of Count_23); here the order is the list's, always.
 * RFX_E_ARG, nothing written: n_k outside 2..16; a list that is not strictly ascending; a k outside 8..124, or 32, 63, 94 (the
 * sorter refuses them), or 64, 96 (the k > 31 counter does); P outside 1..63; a negative clip, max_cov or min_cov; a switch that is
 * not 0 or 1; min_cov above 10000 (3 min_cov is the sorter's int E); words_per_read < 1 or 32 words_per_read < max_read_len; a null
 * pointer; and -- checked for EVERY k with the E the rule gives it, before any work -- whatever the stages themselves refuse
 * (min_error_cov <= 0 -- also 3 min_cov <= 0 where the rule sets it --, min_repeat_fold < 1, sensitive with more than 937 words a
 * read, a read of 30000 bases or more in sensitive mode).  n_reads = 0 gives an empty set.  A short d_out: RFX_E_CAP with n and
 * need_words set and NOTHING written -- the sets are not kept, so the caller's retry with arrays that hold them runs the whole call
 * again.  MEMORY: two k's sets and one stage's scratch at a time, beside the Count_<k>_reduced records of the k already done (a
 * pair's final set is cut down to them as soon as the next pair has consumed it). */
typedef struct {
    int    min_cov;          /* minKmerCoverage (2)                                          */
    int    max_cov;          /* maxKmerCoverage (10000000)                                   */
    int    min_error_cov;    /* minErrorCoverage, E, until the rule above replaces it (8)    */
    int    bubble;           /* param.bubble (1)                                             */
    int    sensitive;        /* -sensitive: the mercy k-mers of every k <= 31 (0)            */
    int    front_clip;       /* (0)                                                          */
    int    end_clip;         /* (0)                                                          */
    int    P;                /* the partitions of the reduction's sorts (8)                  */
    double min_repeat_fold;  /* minRepeatFold, F (1.5)                                       */
} rfx_reduce_reads_params;
void rfx_reduce_reads_default_params(rfx_reduce_reads_params *p);
int rfx_dev_reduce_reads(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int words_per_read,
                         int max_read_len, const int *klist, int n_k, const rfx_reduce_reads_params *params, rfx_dyn_packed *d_out,
                         int64_t *out_n_per_k);
/* HOST FORM: ASCII reads (bases + n_reads + 1 offsets, as rfx_mercy_text takes them; any base other than A, C, G reads as T) in, ONE
 * text buffer out that holds the rows `KMER,marker|left|right\n` of Count_<k>_reduced of every k in list order; out_off (a host
 * array of n_k + 1 entries) receives where each k's rows begin and end, *out_len = out_off[n_k].  One upload and one 2-bit encode of
 * the reads, the stages as in rfx_dev_reduce_reads, one copy back per k.  The rows of k are rfx_dev_ksort_to_text's of the set that
 * holds Count_<k>_reduced, so the text equals what `sort` per k and `reduce` pair by pair write, E rule included.  A short buffer
 * follows rfx_reduce_text's rule: RFX_E_CAP with *out_len and every out_off set and NOTHING written.  RFX_E_ARG as
 * rfx_dev_reduce_reads (words_per_read is the longest read's); offsets that run backwards; a null pointer.  RFX_E_LIMIT: 2^31 reads
 * or more.  n_reads = 0 gives an empty text. */
int rfx_reduce_reads(rfx_ctx *ctx, const uint8_t *bases, const int64_t *read_off, int64_t n_reads, const int *klist, int n_k,
                     const rfx_reduce_reads_params *params, char *out, int64_t cap, int64_t *out_len, int64_t *out_off);

/* The contig fixing stage (Assembly_intermediate/04Fixing) on the same PACKED record sets in HBM:
 * P/ReflexivDSDynamicKmerFixing.java `assemblyFromKmer` (:125-260).  It is the stage directly behind the last dynamic-k iteration: its
 * input is the text rfx_dev_dyn_to_text writes ("SUBKMER,marker|left|right,EXTENSION" rows), its output has the same form.
 * max_k = param.maxKmerSize = the LAST k of the k list; FixedKmerSize = 31 everywhere, so every key behind the contig ends has 30 bases.
 *   rfx_dev_fix_binarize      step 1, DynamicKmerBinarizerFromReducedToSubKmer (:3106-3203): rfx_dev_dyn_binarize form 1, then a row whose
 *                             sub-k-mer and extension together have fewer than 2 max_k bases is dropped (:3141)
 *   rfx_dev_fix_contig_ends   steps 2-3, DSExtractFixingKmerFromContigEnds (:1190-1256) + DSgetFixingLongKmer (:520-541) + DSgetFixingKmer
 *                             (:857-874).  The contig is key + extension for marker 1, extension + key otherwise, L bases; one of
 *                             L < 2 max_k gives nothing.  d_kmers receives the end 31-mers as 62-bit values (the first base in bits
 *                             61..60), contig by contig in the reference's emission order: for i = 0 .. max_k - 31 bases [i, i + 31) and
 *                             then bases [L - i - 31, L - i); *n_kmers = their count.  d_out_long receives one record per contig: the
 *                             trimmed contig, bases [max_k - 30, L - (max_k - 30)), cut key = its first 30 bases, extension = the rest,
 *                             marker 1, left and right each replaced by max_k + 3 where the input's was > 0 (:1240-1247)
 *   rfx_dev_fix_kmer_set      steps 4-5 up to the union: groupBy("kmer").count() (:206; the count is never read: distinct),
 *                             DSFixingKmerLeftAndRightMarkerAssignment (:1857-1878; key = the first 30 bases, extension = the last base,
 *                             attribute 1|-1|-1) and union (:213): the distinct 31-mers' records first, then d_long's.  d_kmers is read,
 *                             not changed; a value of 2^62 or more is RFX_E_ARG
 *   rfx_dev_fix_fork_filter   reflected 0: step 6, DSFilterForkSubKmerWithErrorCorrection (:2057-2116), 1: step 8,
 *                             DSFilterForkReflectedSubKmerWithErrorCorrection (:2232-2283) over a SORTED set (rfx_dev_dyn_sort) and its P
 *                             partition starts; d_out_part_start receives the P + 1 starts of the output (step 9's first pass runs on
 *                             them).  Within a partition, a run of equal keys that holds a row longer than one base keeps exactly those
 *                             rows, in order; any other run keeps its LAST row of the smallest base code.  The two classes are one text
 *                             (the base compared is the extension's first), so `reflected` is checked and selects nothing
 *   rfx_dev_fix_reflect       step 7, DSChangingFixingKmerToReflectedKmer (:1571-1608): key = the LAST 30 bases of the contig, extension =
 *                             its front, marker 2, left and right kept
 *   rfx_dev_fix_run           steps 1-9 with the set resident between the operators: the above, the two sort("k-1") (rfx_dev_dyn_sort with
 *                             the caller's P), then DSExtendFixingKmerLoop (:2371-3104) once on the right fold's partitions WITHOUT a sort
 *                             and behind a sort min(max_iteration + 1, 17) more times (:229-243; there is no stop rule).  With every key
 *                             30 bases long the loop is rfx_dev_dyn_extend_pass with stage 1 and a start_iteration below 61, reused
 *                             unchanged: no prefix relation, `extra` = 0, the stage branches out of reach -- every loop pass of every case
 *                             of tests/golden/fixing_vectors.npz agrees.  randomReflexivMarker starts at 2 in every partition, at 1 when
 *                             scramble == 3 (:2407-2409).  The output file is rfx_dev_dyn_to_text of the result
 *                             (DSBinaryFixingKmerWithLongExtensionToString, :262-299)
 *   rfx_fix_text              host text in, host text out: upload, run, to-text, one copy each way
 * DEVIATIONS, all stated: (1) a row whose sub-k-mer exceeds 124 bases is RFX_E_LIMIT for the set, kept or dropped, where the reference
 * would carry it.  (2) A ')' behind the EXTENSION is dropped, as rfx_dyn_binarize form 1 drops it; the reference drops one behind the
 * attribute only and would read that one as a base.  A malformed attribute reads as rfx_dyn_binarize reads it where the reference throws.
 * (3) groupBy's output order is Spark's hash order; rfx_dev_fix_kmer_set emits the distinct 31-mers in ascending order.  Nothing from the
 * first fold on depends on it (the one-base rows of a key are distinct 31-mers, so the smallest base code is one row whatever the
 * order): tests/golden/make_fixing_vectors.py runs every case under two orders and fails if a later stage differs.
 * CONTRACTS.  Every output set keeps the rfx_dyn_packed invariant.  Capacities from the input alone: binarize cap_n >= n_rows and
 * cap_words >= n_rows + text bytes / 32; contig ends cap_kmers >= 2 (max_k - 30) in.n, cap_n >= in.n and cap_words >=
 * in.ext_off[in.n] + 4 in.n -- together n (2 (max_k - 30) + 1) items; kmer_set cap_n >= n_kmers + long.n and cap_words >= n_kmers +
 * long.ext_off[long.n]; fork_filter and reflect cap_n >= in.n and cap_words >= in.ext_off[in.n]; run cap_n >= n_rows (2 (max_k - 30) +
 * 1) and cap_words >= cap_n + text bytes / 32.  A short output: RFX_E_CAP with n and need_words (*n_kmers, *out_len) set and nothing
 * written, the part starts neither; contig_ends checks both of its outputs before it writes either.  RFX_E_ARG, nothing written: max_k
 * outside 31..124; max_iteration < -1 (-1 runs the unsorted first pass only); P outside 1..63; partition starts that do not run
 * from 0 to n without going backwards (read back and checked before a kernel indexes with them); a key that is not 30 bases long, or a
 * record without an extension, where kmer_set, fork_filter and reflect expect them; a null pointer.  n_rows = 0 and n = 0 are valid
 * everywhere.  All run on the context's stream and return after it has drained. */
typedef struct {
    int max_k;           /* the LAST k of the k list (param.maxKmerSize)                                      */
    int scramble;        /* param.scramble: 3 starts the loop's marker at 1, anything else at 2               */
    int max_iteration;   /* param.maximumIteration: min(max_iteration + 1, 17) sort + loop rounds; the second   */
                         /* stage (rfx_*fix2_*) caps them at 29                                               */
} rfx_fix_params;
void rfx_fix_default_params(rfx_fix_params *p, int max_k);   /* scramble 2, max_iteration 150 */
int rfx_dev_fix_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const rfx_fix_params *params,
                         rfx_dyn_packed *d_out);
int rfx_dev_fix_contig_ends(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_fix_params *params, rfx_dyn_packed *d_out_long, uint64_t *d_kmers,
                            int64_t cap_kmers, int64_t *n_kmers);
int rfx_dev_fix_kmer_set(rfx_ctx *ctx, const uint64_t *d_kmers, int64_t n_kmers, const rfx_dyn_packed *d_long, rfx_dyn_packed *d_out);
int rfx_dev_fix_fork_filter(rfx_ctx *ctx, int reflected, const rfx_dyn_packed *d_sorted, const int64_t *d_part_start, int P, rfx_dyn_packed *d_out,
                            int64_t *d_out_part_start);
int rfx_dev_fix_reflect(rfx_ctx *ctx, const rfx_dyn_packed *d_in, rfx_dyn_packed *d_out);
int rfx_dev_fix_run(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, int P, const rfx_fix_params *params,
                    rfx_dyn_packed *d_out);
int rfx_fix_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, char *out, int64_t cap,
                 int64_t *out_len);
/* The seam between the last dynamic-k iteration and this stage without the text: the result is exactly what
 * rfx_dev_fix_run gives for the rows rfx_dev_dyn_to_text writes of d_in.  Step 1 becomes form 1's READING of the set -- of every record
 * the key's and the extension's bases and nothing behind them, the marker through its decimal text (pk_int_as_text: nine digits of ten),
 * left / right through theirs and then clamped to +-30000, as rfx_dev_dyn_from_kmers states it -- followed by the same length filter (a
 * record is kept iff key + extension >= 2 max_k bases) and steps 2-9 unchanged.  Capacities as rfx_dev_fix_run's with "text bytes / 32"
 * replaced by what the set bounds it with: cap_n >= in.n (2 (max_k - 30) + 1) and cap_words >= cap_n + in.ext_off[in.n] + 4 in.n.  A short
 * output: RFX_E_CAP with n and need_words set and nothing written.  RFX_E_ARG, nothing written: what rfx_dev_fix_run refuses of P and
 * params; a null pointer; a record without an extension (ext_len < 1), kept or dropped: it cannot be printed as a form-1 row; extension
 * offsets that do not follow the extension lengths (the rfx_dyn_packed layout; checked for every record before a kernel indexes with
 * them).  RFX_E_LIMIT: a key of more than 124 bases, kept or dropped; 2^31 records or more.  in.n = 0 is valid. */
int rfx_dev_fix_run_packed(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int P, const rfx_fix_params *params, rfx_dyn_packed *d_out);

/* The SECOND contig fixing stage (Assembly_intermediate/05FixingAgain and 06ContigEnds) on the same packed sets in
 * HBM: P/ReflexivDSDynamicKmerFixingRoundTwo.java `assemblyFromKmer` (:138-263).  Its input is the text of 04Fixing -- or the packed set
 * rfx_dev_fix_run leaves, with no text in between.  It is the last stage ahead of the Mapping stage, which needs an external aligner.
 *   rfx_dev_fix2_binarize     DynamicKmerBinarizerFromReducedToSubKmer (:562-752): rfx_dev_dyn_binarize form 1, NO length filter
 *   rfx_dev_fix2_run          min(max_iteration + 1, 29) x (sort("k-1") with the caller's P, DSExtendFixingKmerLoop) (:203-213); every
 *                             round sits behind a sort; max_iteration = -1 gives zero rounds, which copy the set.  The loop is the one
 *                             of the first stage, i.e. rfx_dev_dyn_extend_pass with stage 1 and a start_iteration below 61, reused
 *                             unchanged: every pass of every case of tests/golden/fixing2_vectors.npz agrees
 *   rfx_dev_fix2_contigs      DSBinaryFixingKmerWithLongExtensionToString (:293-560) without the text: key || extension for marker 1,
 *                             extension || key otherwise, the contigs of at least 2 max_k bases in input order as a packed contig set
 *                             (rfx_contigs_packed, its invariant included: what rfx_dev_dedup_contigs and rfx_dev_contigs_unpack
 *                             take); d_left / d_right (cap_n entries each) receive every kept contig's left / right
 *   rfx_dev_fix2_to_text      zipWithIndex + TagStringContigRDDID (:987-1005): the rows of 05FixingAgain,
 *                             "Contig_<L>_<left>_<right>_<idx>,<contig>\n", idx = the position in the set (the rank among the KEPT
 *                             contigs), left / right in decimal as rfx_dev_dyn_to_text prints them
 *   rfx_dev_fix2_ends_text    DSExtractContigEndsForAlignment (:265-291): the lines of 06ContigEnds; a contig of 400 bases or more gives
 *                             ">ID-L\n" + bases [0, 200) + "\n" + ">ID-R\n" + bases [L - 200, L) + "\n", a shorter one ">ID\n" + the
 *                             contig + "\n"; ID = "Contig_<L>_<left>_<right>_<idx>"
 *   rfx_fix2_text             host text in, both host texts out: one upload, binarize, run, contigs, both texts, one copy back each
 * DEVIATION, stated: the reference keeps the key in ONE long and would cut a longer key to it; here a row whose sub-k-mer is not 30
 * bases long, or a row without an extension, is RFX_E_ARG for the set (binarize, run and rfx_fix2_text), as in the first stage.  A ')'
 * behind the extension is dropped as rfx_dyn_binarize form 1 drops it.
 * CONTRACTS.  binarize: cap_n >= n_rows and cap_words >= n_rows + text bytes / 32.  run: cap_n >= in.n and cap_words >=
 * in.ext_off[in.n] (no pass needs more than its input).  contigs: the kept contigs need sum ceil((key_len + ext_len) / 32) words, and
 * ceil((a + b) / 32) <= ceil(a / 32) + ceil(b / 32), so cap_n >= in.n and cap_words >= in.ext_off[in.n] + sum ceil(key_len / 32) always
 * suffice: in.ext_off[in.n] + in.n for the 30-base keys of this stage, in.ext_off[in.n] + 4 in.n for any set (rfx_dev_fix2_contigs
 * takes keys of any length up to 124 bases).  A short output: RFX_E_CAP with n and need_words (contigs: need_n and need_words) set and
 * nothing written, d_left / d_right neither.  The two text writers follow the text-buffer rule: filled up to cap, nothing at or past it,
 * RFX_E_CAP with *out_len = the need; d_text may have any alignment.  rfx_fix2_text with a short buffer: RFX_E_CAP with BOTH lengths
 * set and NEITHER buffer written.  RFX_E_ARG, nothing written: max_k outside 31..124; max_iteration < -1; P outside 1..63; a key that
 * is not 30 bases long or a record without an extension (binarize, run); a contig set whose word_off and len disagree (the text
 * writers); a null pointer.  RFX_E_LIMIT: a sub-k-mer of more than 124 bases, 2^31 rows / records / contigs or more, a contig of 2^30
 * bases or more.  n_rows = 0 and n = 0 are valid everywhere.  All run on the context's stream and return after it has drained. */
int rfx_dev_fix2_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, rfx_dyn_packed *d_out);
int rfx_dev_fix2_run(rfx_ctx *ctx, const rfx_dyn_packed *d_in, int P, const rfx_fix_params *params, rfx_dyn_packed *d_out);
int rfx_dev_fix2_contigs(rfx_ctx *ctx, const rfx_dyn_packed *d_in, const rfx_fix_params *params, rfx_contigs_packed *d_out, int32_t *d_left,
                         int32_t *d_right);
int rfx_dev_fix2_to_text(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, char *d_text, int64_t cap,
                         int64_t *out_len);
int rfx_dev_fix2_ends_text(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, char *d_text, int64_t cap,
                           int64_t *out_len);
int rfx_fix2_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, char *out, int64_t cap,
                  int64_t *out_len, char *ends_out, int64_t ends_cap, int64_t *ends_len);

/* The END EXTENSION of contigs from alignment rows (Assembly_intermediate/07EndExtend) on the same packed sets in
 * HBM: P/ReflexivDSDynamicKmerMapping.java BEHIND its aligner (driver :305-347).  The caller runs any aligner on 06ContigEnds and hands
 * over its rows "name \t start \t cigar \t seq" (RNAME, POS, CIGAR, SEQ of a SAM line; a seq that is exactly L, R or L-R is a repeat
 * marker), as text in HBM in the form rfx_dev_dyn_binarize takes (d_text + d_row_off, a trailing "\n" or "\r\n" is not part of a row).  The
 * input contigs are what rfx_dev_fix2_contigs returns (the set, d_left, d_right), so fix2 feeds this stage with no text in between;
 * contig i is named Contig_<len[i]>_<left[i]>_<right[i]>_<i>, with -L or -R behind it for an end of 200 bases.
 *   rfx_dev_endext_consensus  SAMString2ROW (:369-388: a row of fewer than 4 fields is skipped) + DSProcessSAMandExtendContigs (:564-994):
 *                             per contig the two [300][4] pile-ups and their consensus (the highest count, a tie to the HIGHER code, at
 *                             most 300 bases) as two packed contig sets of in.n entries each -- left: from the base next to the contig
 *                             OUTWARDS, right: in read order -- and flags[i]: 1 = two or more left repeat markers, 2 = right
 *   rfx_dev_endext_contigs    the union with 05FixingAgain, sort("ID") (:320-331), DSExtendContigs (:413-562) and the index and filter of
 *                             zipWithIndex + TagStringContigRDDID (:1268-1286) without the text: the contigs of 07EndExtend in OUTPUT order
 *                             (the byte order of the ID strings: Contig_100_ sorts ahead of Contig_99_) as a packed contig set of BASES
 *                             ONLY, reversed left consensus || contig || right consensus, with per contig left_len / right_len (the
 *                             lengths the ID carries: 3 more on a flagged side), flags, the new left / right (a flagged side's field
 *                             becomes 1 where it was 1 or less), src_idx (the input contig) and new_idx (the position among ALL spliced
 *                             contigs; only those of at least 2 max_k TEXT characters are in the set).  The literals "-1l" / "r1-" that
 *                             the reference leaves in a flagged contig's text live in flags, not in the words
 *   rfx_dev_endext_to_text    the rows ">Contig_<L>_<left>_<right>_<idx>_<ll>_<rl>_<new>,<sequence>\n" (L the ORIGINAL length, as in the
 *                             reference), the literals at the two seams, byte for byte
 *   rfx_endext_text           host form: the text of 05FixingAgain (row i must be Contig_<L>_<left>_<right>_<i>,<L bases of ACGT>: RFX_E_ARG
 *                             otherwise) + the row text in, the text of 07EndExtend out; one upload each and one copy back
 * DEVIATIONS, all stated.  (1) All alignment rows form ONE logical partition: every row of a contig is counted, in any order of the
 * rows, so the stage takes no P (for P > 1 the reference cuts a contig's rows between partitions and the last part wins in an order
 * Spark does not define).  (2) RFX_E_ARG for the set, nothing written, where the reference throws: a row that is no marker whose CIGAR is
 * not ([0-9]+[A-Z=])+ (operations of up to 9 digits), whose start is no decimal int, or whose overhang would index outside seq.  (3) A
 * row whose name is not the ID of the contig at its <idx> (L, left and right all equal, as Integer.toString writes them, one suffix at
 * most) is ignored before anything else of it is read, as the reference's result ignores it.
 * CAPACITIES, derived from the input.  consensus: cap_n >= in.n and cap_words >= 10 in.n for each of the two sets (a consensus has at
 * most 300 bases = 10 words).  contigs: a spliced contig of cl + L + cr bases takes ceil((cl + L + cr) / 32) <= ceil(L / 32) + ceil(cl /
 * 32) + ceil(cr / 32) words, so cap_n >= in.n and cap_words >= in.word_off[in.n] + 20 in.n always suffice (+ in.n more covers any other
 * rounding).  A short output: RFX_E_CAP with need_n / need_words set and nothing written.  rfx_dev_endext_to_text follows the
 * text-buffer rule: filled up to cap, nothing at or past it, RFX_E_CAP with *out_len = the need; d_text may have any alignment;
 * rfx_endext_text with a short buffer writes nothing.  RFX_E_ARG, nothing written: the cases above; max_k outside 31..124; a null pointer;
 * a set whose word_off and len disagree, a consensus of more than 300 bases, flags other than 0..3.  RFX_E_LIMIT: 2^31 rows or contigs, a
 * contig of 2^30 bases.  n = 0 and n_rows = 0 are valid everywhere.  All run on the context's stream and return after it has drained. */
typedef struct {
    rfx_contigs_packed left, right;   /* in.n entries each; left: from the base next to the contig outwards      */
    int32_t *flags;                   /* cap_n entries: 1 = left flagged, 2 = right flagged                       */
} rfx_endext_consensus;               /* every pointer is a DEVICE pointer, the struct lives on the host          */
typedef struct {
    rfx_contigs_packed set;           /* bases only, in output order                                              */
    int32_t *left, *right;            /* cap_n entries each, as every array below                                 */
    int32_t *left_len, *right_len;    /* text characters of both consensus strings (3 more where flagged)        */
    int32_t *flags, *src_idx, *new_idx;
} rfx_endext_set;
int rfx_dev_endext_consensus(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, const char *d_text,
                             const int64_t *d_row_off, int64_t n_rows, rfx_endext_consensus *d_out);
int rfx_dev_endext_contigs(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right,
                           const rfx_endext_consensus *d_cons, int max_k, rfx_endext_set *d_out);
int rfx_dev_endext_to_text(rfx_ctx *ctx, const rfx_endext_set *d_in, char *d_text, int64_t cap, int64_t *out_len);
int rfx_endext_text(rfx_ctx *ctx, const char *contig_text, const int64_t *contig_off, int64_t n_contigs, const char *row_text, const int64_t *row_off,
                    int64_t n_rows, int max_k, char *out, int64_t cap, int64_t *out_len);

/* The contig EXTENSION stages (Assembly_intermediate/08Extend and 09ExtendAgain) on the same packed sets in HBM:
 * P/ReflexivDSDynamicKmerExtend.java `assemblyFromKmer` (:125-254) and P/ReflexivDSDynamicKmerExtendRoundTwo.java (:125-221).  08Extend is
 * the contig fixing stage (rfx_dev_fix_*) with another binarizer and other contig ends; its input is the set rfx_dev_endext_contigs
 * leaves -- no text in between -- or the text of 07EndExtend.  09ExtendAgain is rfx_dev_fix2_binarize + rfx_dev_fix2_run +
 * rfx_dev_fix2_contigs, called as they are, and another row header; the contig set it leaves is what rfx_dev_dedup_contigs takes.
 *   rfx_dev_ext_from_text     DynamicKmerBinarizerFromReducedToSubKmer (:3118-3219) up to the packed set: the rows
 *                             ">Contig_<L>_<left>_<right>_<idx>_<ll>_<rl>_<new>,<sequence>" of 07EndExtend (d_text + d_row_off, as
 *                             rfx_dev_dyn_binarize takes them) -> an rfx_endext_set of the rows whose sequence has 2 max_k characters or
 *                             more (:3157), in order: every character other than A, C and G is a T base (the literals "-1l" / "r1-" of
 *                             a flagged seam among them), flags 0, left / right / left_len / right_len / src_idx / new_idx = the
 *                             header's <left> / <right> / <ll> / <rl> / <idx> / <new> (the stage reads neither index)
 *   rfx_dev_ext_contig_ends   DSExtractFixingKmerFromContigEnds (:1189-1267) + DSgetFixingLongKmer (:514-535) + DSgetFixingKmer
 *                             (:853-870) on a set with flags 0..3.  With T = the TEXT length of a contig (len + 3 per flagged side, the
 *                             three characters of a flagged seam read as T bases at [left_len - 3, left_len) and [T - right_len, T -
 *                             right_len + 3)): d_kmers receives the end 31-mers as 62-bit values, contig by contig in the reference's
 *                             emission order -- characters [i, i + 31) for i = 0 .. left_len - 1, then [T - i - 31, T - i) for i =
 *                             right_len - 1 .. 0; d_out_long one record per contig: the cut contig [left_len, T - right_len), which is the
 *                             original contig of 05FixingAgain, key = its first 30 bases, extension = the rest, marker 1, left and right
 *                             KEPT (clamped to +-30000 as buildingAlongFromThreeInt clamps them; the fixing stage's replacement by
 *                             max_k + 3 is commented out in this class).  A contig of fewer than 2 max_k characters gives nothing (:1207)
 *   rfx_dev_ext_run           the set and P -> the record set of 08Extend, resident between the operators: the contig ends above, then
 *                             steps 4-9 of the fixing stage, the same code (the distinct 31-mers, union, sort, fold, reflection, sort,
 *                             fold, DSExtendFixingKmerLoop once unsorted and min(max_iteration + 1, 17) times behind a sort, :206-243);
 *                             max_iteration = -1 runs the unsorted first pass only.  The output file is rfx_dev_dyn_to_text of the result
 *   rfx_ext_text              host text of 07EndExtend in, host text of 08Extend out: one upload and one copy back
 *   rfx_dev_ext2_to_text      zipWithIndex + TagRowContigRDDID (ExtendRoundTwo :674-692) behind DSBinaryFixingKmerToFullKmer (:415-456, which
 *                             is rfx_dev_fix2_contigs): the rows ">Contig-<len>-<idx>,<contig>\n" of a packed contig set, idx = the
 *                             position in the set
 *   rfx_ext2_text             host text of 08Extend in, host text of 09ExtendAgain out: one upload, the second fixing stage's binarizer,
 *                             min(max_iteration + 1, 29) x (sort, loop) and contigs, the text, one copy back
 * DEVIATIONS, all stated.  (1) A kept contig whose cut part, T - left_len - right_len characters, is below 32 is RFX_E_ARG for the set:
 * the reference turns 31 characters into an end 31-mer and anything shorter into a record with a short key; 05FixingAgain holds no contig
 * below 2 max_k >= 62.  (2) The distinct 31-mers come out ascending, as in rfx_dev_fix_kmer_set; nothing from the first fold on depends
 * on it (tests/golden/make_extend_vectors.py runs every case under two orders and fails if a later stage differs).  (3) A contig of
 * 10,000,000 bases or more is RFX_E_LIMIT in rfx_dev_ext2_to_text and rfx_ext2_text: the reference's changeLine would put a line break
 * inside the csv field.
 * CAPACITIES, from the input alone.  from_text: cap_n >= n_rows and cap_words >= n_rows + text bytes / 32.  contig_ends: cap_kmers >=
 * sum(left_len + right_len) -- 606 in.n always suffices --, cap_n >= in.n and cap_words >= in.word_off[in.n].  run: cap_n >= 607 in.n and
 * cap_words >= cap_n + in.word_off[in.n].  A short output: RFX_E_CAP with the needs set (need_n / need_words; n / need_words and
 * *n_kmers; *out_len) and nothing written; contig_ends checks both of its outputs before it writes either.  rfx_dev_ext2_to_text follows
 * the text-buffer rule: filled up to cap, nothing at or past it, RFX_E_CAP with *out_len = the need; d_text may have any alignment; the
 * host forms write nothing into a short buffer.  RFX_E_ARG, nothing written: max_k outside 31..124; max_iteration < -1; P outside 1..63;
 * a null pointer; a set whose word_off and len disagree; flags outside 0..3; left_len or right_len outside 0..303, or below 3 on a
 * flagged side; deviation (1); a row whose ID is not ">Contig_" and seven decimal ints separated by '_' with a ',' behind them; a
 * sequence that starts with '('.  RFX_E_LIMIT: 2^31 rows or contigs, a contig of 2^30 bases, 2^32 end 31-mers.  n = 0 and n_rows = 0 are
 * valid everywhere.  All run on the context's stream and return after it has drained. */
int rfx_dev_ext_from_text(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n_rows, const rfx_fix_params *params,
                          rfx_endext_set *d_out);
int rfx_dev_ext_contig_ends(rfx_ctx *ctx, const rfx_endext_set *d_in, const rfx_fix_params *params, rfx_dyn_packed *d_out_long, uint64_t *d_kmers,
                            int64_t cap_kmers, int64_t *n_kmers);
int rfx_dev_ext_run(rfx_ctx *ctx, const rfx_endext_set *d_in, int P, const rfx_fix_params *params, rfx_dyn_packed *d_out);
int rfx_ext_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, char *out, int64_t cap,
                 int64_t *out_len);
int rfx_dev_ext2_to_text(rfx_ctx *ctx, const rfx_contigs_packed *d_in, char *d_text, int64_t cap, int64_t *out_len);
int rfx_ext2_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, char *out, int64_t cap,
                  int64_t *out_len);

/* READS ONTO THE CONTIG ENDS (the front half of the Mapping stage) on the same packed sets in HBM.  The reference
 * pipes every read through an external `minimap2 -x sr` on 06ContigEnds and a script it does not ship
 * (P/ReflexivDSDynamicKmerMapping.java :162-223, :1157-1266); rfx_dev_endext_consensus only uses rows that hang over an end of a target.
 * So this stage is an ungapped END-OVERHANG mapper whose SEMANTICS ARE ITS OWN (stated deviation: nothing here is compared with the
 * reference or with minimap2, whose sensitivity nobody has measured against it).  With it the device chain is rfx_dev_fix2_contigs ->
 * rfx_dev_map_ends -> rfx_dev_map_to_text -> rfx_dev_endext_consensus -> ... with nothing on the host.
 * TARGETS: the records of 06ContigEnds as rfx_dev_fix2_ends_text defines them, from the set rfx_dev_fix2_contigs returns.  Contig i of
 * L >= 400 bases gives ID-L = bases [0, 200) with a LEFT end only and ID-R = bases [L - 200, L) with a RIGHT end only; a shorter one gives
 * ID = the whole contig with both ends; ID = Contig_<L>_<left>_<right>_<i>.  End number = 2 i + side (0 left, 1 right): contig ascending,
 * left before right.  A target shorter than `seed` has no ends.
 * READS: the 2-bit read store as rfx_dev_count_reads_ragged takes it (d_words, d_read_len, n_reads, words_per_read); codes A0 C1 G2,
 * anything else 3, so an N reads as T, here and in the seq written out; words and bits past a read's length may hold anything.  Each read
 * is tried as stored (strand 0) and as its reverse complement (strand 1); r is that orientation, n its length.
 * LEFT END of target T, read offset o, 1 <= o <= n - seed: the seed matches exactly, r[o, o + seed) == T[0, seed); v = min(n - o, len T),
 * p = n - o - v; valid iff v >= min_overlap and r[o, o + v) differs from T[0, v) at max_mismatch positions at most (on codes).  Row:
 * "name \t 1 \t <o>S<v>M[<p>S] \t r \n", the <p>S part only where p > 0.
 * RIGHT END, read offset q, 0 <= q, q + seed <= n - 1: r[q, q + seed) == T[len - seed, len); overhang o = n - q - seed >= 1; v = min(q +
 * seed, len T), p = q + seed - v; r[p, p + v) against T[len - v, len).  Row: "name \t <len - v + 1> \t [<p>S]<v>M<o>S \t r \n".
 * WHOLE-CONTIG targets: a placement with p > 0 (read bases past BOTH ends) is emitted by neither end.  Two targets with the same end seed
 * each get their rows; one read may give several rows; a palindromic seed is treated like any other, each strand on its own.  No
 * repeat-marker rows (seq L, R, L-R) are written, so `flags` stay 0 behind this stage (stated deviation: they come from the script).
 * ORDER of rows: read index, strand (0 first), end number, offset (o at a left end, q at a right end).
 * (A fact of the consumer, left as it is: rfx_dev_endext_consensus adds nothing for a LEFT overhang of exactly one base -- it computes
 * clip - start, start is 1 here, and 0 is skipped (:683-713).  The row is written all the same.)
 *   rfx_map_default_params  seed 21 (minimap2 -x sr uses k = 21), min_overlap 31, max_mismatch 2
 *   rfx_dev_map_ends        the rows as rfx_map_hits: device arrays of cap_n entries, one entry per row in the order above -- read
 *                           index, end number, strand, offset, v -- and the host fields n, need_n and seed (the seed of the call, which
 *                           rfx_dev_map_to_text needs for a right end's clips)
 *   rfx_dev_map_to_text     the rows as text in HBM and their n + 1 int64 offsets into d_row_off (cap_rows entries), in exactly the form
 *                           rfx_dev_endext_consensus takes; `hits` must be what rfx_dev_map_ends wrote for the same contigs and reads
 *                           (every hit is checked against them before anything indexes with it, except that a read index cannot be
 *                           checked against n_reads, which the call does not take)
 *   rfx_map_text            host form: the text of 05FixingAgain (as rfx_endext_text takes it) and ASCII reads (bases + n_reads + 1
 *                           offsets) in, the row text out; one upload each and one copy back
 * A short output.  map_ends: RFX_E_CAP with need_n set and nothing written.  map_to_text follows the text-buffer rule: filled up to cap,
 * nothing at or past it, RFX_E_CAP with *out_len = the need, d_text may have any alignment; cap_rows below n + 1 is RFX_E_CAP with
 * *out_len set and NOTHING written.  rfx_map_text with a short buffer writes nothing.  RFX_E_ARG, nothing written: seed outside 11..31,
 * min_overlap outside seed..200, max_mismatch outside 0..31; a null pointer; a contig set whose word_off and len disagree;
 * words_per_read < 1; a d_read_len[i] above 32 words_per_read (found by the counting pass); a hit that map_ends cannot have written.
 * RFX_E_LIMIT: 2^31 hits or reads, 2^29 contigs, a contig of 2^30 bases.  n_reads = 0 and n = 0 are valid everywhere.  All run on the
 * context's stream and return after it has drained. */
typedef struct { int seed, min_overlap, max_mismatch; } rfx_map_params;
typedef struct {
    int64_t n;                                    /* rows (host field, set by rfx_dev_map_ends)                    */
    int32_t *read, *end, *strand, *offset, *v;    /* cap_n entries each                                            */
    int64_t cap_n, need_n;
    int32_t seed;                                 /* the seed of the call that wrote them (host field)             */
} rfx_map_hits;                                   /* every pointer is a DEVICE pointer, the struct lives on the host */
void rfx_map_default_params(rfx_map_params *p);
int rfx_dev_map_ends(rfx_ctx *ctx, const rfx_contigs_packed *d_contigs, const int32_t *d_left, const int32_t *d_right, const uint64_t *d_words,
                     const uint32_t *d_read_len, int64_t n_reads, int words_per_read, const rfx_map_params *params, rfx_map_hits *d_out);
int rfx_dev_map_to_text(rfx_ctx *ctx, const rfx_contigs_packed *d_contigs, const int32_t *d_left, const int32_t *d_right, const uint64_t *d_words,
                        const uint32_t *d_read_len, int words_per_read, const rfx_map_hits *hits, char *d_text, int64_t cap, int64_t *out_len,
                        int64_t *d_row_off, int64_t cap_rows);
int rfx_map_text(rfx_ctx *ctx, const char *contig_text, const int64_t *contig_off, int64_t n_contigs, const uint8_t *bases, const int64_t *read_off,
                 int64_t n_reads, const rfx_map_params *params, char *out, int64_t cap, int64_t *out_len);
/* The seam between this stage and the end extension (rfx_dev_endext_consensus above) without the row text: the result is exactly what rfx_dev_endext_consensus gives on the rows rfx_dev_map_to_text writes for the same contigs, reads
 * (d_words, d_read_len, words_per_read) and hits.  What a hit adds follows from (read, end, strand, offset, v), the seed, the read's and
 * the contig's length (reflexiv_amd/csrc/rfx_endext_hits.h restates the row and what the row parser reads out of it); the bases come out of
 * the 2-bit read store, strand 1 as the reverse complement.  flags stay 0: the mapper writes no repeat-marker rows.  Capacities as
 * rfx_dev_endext_consensus; a short output: RFX_E_CAP with need_n / need_words set and nothing written.  RFX_E_ARG, nothing written: what
 * rfx_dev_map_to_text refuses -- a null pointer, words_per_read < 1, n above cap_n, a seed outside 11..31 where there are hits, a hit that
 * rfx_dev_map_ends cannot have written for these contigs and reads (every hit is checked before anything indexes with it, except that a
 * read index cannot be checked against n_reads, which the call does not take).  RFX_E_LIMIT: 2^31 hits or contigs. */
int rfx_dev_endext_consensus_hits(rfx_ctx *ctx, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, const uint64_t *d_words,
                                  const uint32_t *d_read_len, int words_per_read, const rfx_map_hits *hits, rfx_endext_consensus *d_out);

/* THE MERCY K-MER STAGE (Count_<k>_mercy) on the 2-bit read store in HBM: P/ReflexivDSDynamicMercyKmer.java
 * `assemblyFromKmer` (:157-322), which the reference runs behind the counter for every k <= 31 in -sensitive mode.  It replaces
 * ReverseComplementKmerBinaryExtractionFromDataset (:1680-1960), DynamicKmerBinarizer (:477-660), sort("seed"), RamenReadExtraction
 * (:1414-1605), sort("ID"), RamenReadRangeCal (:1233-1412), FastqTuple2Dataset (:1607-1678), sort("ID"), ExtractMercyKmerFromRead
 * (:913-1232) and DSBinaryKmerToString (:831-911).
 * SOLID SET: the k-mers of the Count_<k> rows whose k-mer has k bases; on the device the counter's d_out_keys (ascending, one word each,
 * the last base in the lowest bits).  LETTERS: any base other than A, C, G reads as T (the read store does this); the canonical form is
 * the smaller of a k-mer and its reverse complement.  A READ GIVES NOTHING when len - k - end_clip + 1 <= 0, when front_clip > len, when
 * len - 15 - end_clip <= 1 (FastqTuple2Dataset's filter, whose 15 is fixed), or when it has 32 bases or more and its first 31 are A (its
 * first block is 0, which ExtractMercyKmerFromRead :932 takes for a marker row).  HITS: the window positions p, front_clip <= p <= len -
 * end_clip - k, whose canonical k-mer is solid.  GAPS: for neighbouring hits a < b, g = b - a - 1 is kept iff g >= 1 and not k - 1 <= g
 * <= k + 1 (the footprint of one substitution, :1336); nothing before the first or behind the last hit is rescued.  OUTPUT: for every
 * kept gap and every j in (a, b) the canonical k-mer of read[j, j + k), count 1, in (read, j) order, duplicates not merged; text rows
 * "KMER,1\n".  Equal seeds and equal IDs never straddle a Spark range partition, so the stage takes no partition count.
 *   rfx_dev_mercy_kmers    the solid keys and the read store (as rfx_dev_count_reads_ragged takes it) -> the mercy k-mers in the counter's
 *                          key format; *out_n of them.  RFX_E_CAP: *out_n = the need, nothing written
 *   rfx_dev_mercy_to_text  n keys -> the rows in HBM (text-buffer rule: filled up to cap, nothing at or past it, RFX_E_CAP with *out_len
 *                          = the need; d_text may have any alignment) and their n + 1 int64 offsets into d_row_off (nullable), so that
 *                          both can go straight to rfx_dev_ksort_binarize
 *   rfx_mercy_text         host form: the rows of Count_<k> (read as rfx_dev_ksort_binarize reads them: a leading '(' and a trailing ')'
 *                          dropped, a trailing newline ignored; rows of another length are dropped; the rest are sorted and made
 *                          distinct on the device, since a text file promises no order) and ASCII reads (bases + n_reads + 1 offsets)
 *                          in, the row text out; one upload each and one copy back; a short buffer is not written
 * DEVIATIONS, all stated: (1) one call handles ONE k.  (2) The count column of a solid row is not read (the reference parses it and
 * drops it); it must still be decimal digits.  (3) The reference's RamenReadRangeCal throws on an empty partition; here an empty input
 * gives an empty output.  (4) rfx_mercy_text sorts the count rows itself; rfx_dev_mercy_kmers requires them ascending, as the counter
 * returns them.  The reference stores window indices clamped at 30000, so a read of 30000 bases or more is refused.
 * RFX_E_ARG, nothing written: k outside 8..31; a negative clip; words_per_read < 1 or above 937 (rfx_dev_mercy_kmers); a null pointer;
 * solid keys not strictly ascending or not below 4^k; a d_read_len[i] above 32 words_per_read or of 30000 or more; a count row without a
 * comma or with a count that is not digits.  RFX_E_LIMIT: 2^31 reads, solid keys or mercy k-mers.  n_solid = 0, n_reads = 0 and an
 * empty result are valid.  Words and bits past a read's length may hold anything and reach no result.  All run on the context's stream
 * and return after it has drained. */
int rfx_dev_mercy_kmers(rfx_ctx *ctx, const uint64_t *d_solid_keys, int64_t n_solid, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads,
                        int words_per_read, int k, int front_clip, int end_clip, uint64_t *d_out_keys, int64_t cap, int64_t *out_n);
int rfx_dev_mercy_to_text(rfx_ctx *ctx, const uint64_t *d_keys, int64_t n, int k, char *d_text, int64_t cap, int64_t *out_len, int64_t *d_row_off);
int rfx_mercy_text(rfx_ctx *ctx, const char *count_text, const int64_t *count_row_off, int64_t n_rows, const uint8_t *bases, const int64_t *read_off,
                   int64_t n_reads, int k, int front_clip, int end_clip, char *out, int64_t cap, int64_t *out_len);

/* READS TO CONTIGS with the dynamic-k ("meta") assembler in ONE resident call: `reflexiv reduce` + `reflexiv meta`,
 * i.e. the orchestrator Pipelines.reflexivDSDynamicAssemblyStepsPipe (Pipelines.java:840-1291) over the stages above.  The sets between
 * the stages are the library's own and stay in HBM; no text is made between two stages (the two seams that went through text are
 * rfx_dev_fix_run_packed and rfx_dev_endext_consensus_hits); nothing goes to the caller's arrays but the final set; at most one stage's
 * input, output and scratch are live beside the read store.
 * STAGES, in order (the values of stop_after): 00firstFour (the random reflection and 4 passes); the EIGHT iteration jobs 5-9, 10-14,
 * 15-19 (:886), 21-30, 31-40, 41-50, 51-60, 61-70 (:925) -- there is no iteration 20 --, each an rfx_dev_dyn_run with ITS OWN
 * start_iteration, which a pass reads: only the job 61-70 drops the shorter forward records; between two jobs the set is read as the
 * file between them would be (marker, left, right through their decimal text, left / right clamped to +-30000); 04Fixing
 * (rfx_dev_fix_run_packed); 05FixingAgain and 06ContigEnds (rfx_dev_fix2_run, rfx_dev_fix2_contigs); the end mapping on the read store
 * (rfx_dev_map_ends); 07EndExtend (rfx_dev_endext_consensus_hits, rfx_dev_endext_contigs); 08Extend (rfx_dev_ext_run); 09ExtendAgain
 * (rfx_dev_fix2_run, rfx_dev_fix2_contigs); Assembly (rfx_dev_dedup_contigs).
 * THE PARTITION RULE (Pipelines.java:877-883, 914-921, 954-974, repeated ahead of every later stage) is the driver's: O = params->P, one P
 * for `partitions` and `shufflePartition` alike, integer divisions.  First four: O.  Iterations 5-19: O >= 10 ? O * 80 / 100 : O.
 * Iterations 21-70: O >= 10 ? O * 60 / 100 : O.  Fixing, fixing again, extend, extend again: O >= 10 ? O * 40 / 100 : O.  The reference's
 * 20 % and 10 % tiers need O >= 100, which the stages' limit of 63 excludes.  The contig set is a function of P.
 * STATED DEVIATIONS are those of the stages: the end mapping is this library's own and takes no P, the de-duplication takes no P, all
 * alignment rows form one partition, no repeat-marker rows are written.  The reduction takes reduce_params->P as rfx_dev_reduce_reads does.
 *   rfx_meta_default_params     P 8, scramble 2, max_iteration 150, min_contig 500, the mapper's 21 / 31 / 2, stop_after = Assembly
 *   rfx_dev_meta_from_reduced   the set rfx_dev_reduce_reads leaves + the read store (as rfx_dev_map_ends takes it) + max_k (the LAST k of
 *                               the list) -> the de-duplicated contigs as an rfx_contigs_packed
 *   rfx_dev_meta_reads          the read store and the k list -> the same; the reduction (the body of rfx_dev_reduce_reads) first
 *   rfx_meta_reads              host form: ASCII reads in (as rfx_reduce_reads takes them), ONE text out: the file of the stage
 *                               stop_after names, written by that stage's existing writer -- rfx_dev_dyn_to_text's rows for 00firstFour,
 *                               every 01Iteration*, 04Fixing and 08Extend; rfx_dev_fix2_to_text's for 05FixingAgain;
 *                               rfx_dev_fix2_ends_text's for 06ContigEnds; rfx_dev_map_to_text's for the mapper's rows;
 *                               rfx_dev_endext_to_text's for 07EndExtend; rfx_dev_ext2_to_text's for 09ExtendAgain;
 *                               rfx_dev_contigs_to_text with min_contig for Assembly.  report may be null
 * rfx_meta_report (host): n_reduced = the records the reduction leaves; n[s] = the records or contigs the stage s leaves (06ContigEnds
 * repeats 05FixingAgain's, the mapper's entry is its rows, as `hits`); stages behind stop_after stay 0.
 * CONTRACTS.  Every argument of every stage is checked before any work: what rfx_dev_reduce_reads refuses; P outside 1..63; max_k outside
 * 31..124; max_iteration < -1; min_contig < 0; the mapper's parameters out of range; stop_after outside the enum, or other than
 * RFX_META_ASSEMBLY in a device form; a null pointer: RFX_E_ARG, nothing written.  A short d_out: RFX_E_CAP with need_n / need_words
 * set and nothing written; the sets are not kept, so the retry runs the call again.  A short text buffer: RFX_E_CAP with *out_len set
 * and nothing written.  No reads give an empty set and empty texts.  RFX_META_TRACE (environment, set to anything) prints each stage's
 * host time on stderr.  All run on the context's stream and return after it has drained. */
enum {
    RFX_META_FIRST_FOUR = 0,
    RFX_META_ITERATION_5_9, RFX_META_ITERATION_10_14, RFX_META_ITERATION_15_19, RFX_META_ITERATION_21_30, RFX_META_ITERATION_31_40,
    RFX_META_ITERATION_41_50, RFX_META_ITERATION_51_60, RFX_META_ITERATION_61_70,
    RFX_META_FIXING, RFX_META_FIXING_AGAIN, RFX_META_CONTIG_ENDS, RFX_META_MAPPING, RFX_META_END_EXTEND, RFX_META_EXTEND, RFX_META_EXTEND_AGAIN,
    RFX_META_ASSEMBLY,
    RFX_META_STAGES
};
typedef struct {
    int P;                 /* the caller's partition count O; the rule above derives every stage's                 */
    int scramble;          /* param.scramble (2)                                                                    */
    int max_iteration;     /* param.maximumIteration (150): the loop rounds of the fixing and extension stages      */
    int min_contig;        /* param.minContig (500): the shortest contig the Assembly text holds                    */
    int map_seed, map_min_overlap, map_max_mismatch;   /* rfx_map_params (21, 31, 2)                               */
    int stop_after;        /* RFX_META_*: the stage whose file rfx_meta_reads writes (RFX_META_ASSEMBLY)            */
} rfx_meta_params;
typedef struct {
    int64_t n_reduced;
    int64_t n[RFX_META_STAGES];
    int64_t hits;
} rfx_meta_report;
void rfx_meta_default_params(rfx_meta_params *p);
int rfx_dev_meta_from_reduced(rfx_ctx *ctx, const rfx_dyn_packed *d_reduced, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads,
                              int words_per_read, int max_k, const rfx_meta_params *params, rfx_meta_report *report, rfx_contigs_packed *d_out);
int rfx_dev_meta_reads(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int words_per_read, int max_read_len,
                       const int *klist, int n_k, const rfx_reduce_reads_params *reduce_params, const rfx_meta_params *params, rfx_meta_report *report,
                       rfx_contigs_packed *d_out);
int rfx_meta_reads(rfx_ctx *ctx, const uint8_t *bases, const int64_t *read_off, int64_t n_reads, const int *klist, int n_k,
                   const rfx_reduce_reads_params *reduce_params, const rfx_meta_params *params, rfx_meta_report *report, char *out, int64_t cap,
                   int64_t *out_len);

/* Synthetic reads: integer-only counter-based generator, bit-identical to
 * oracle/reflexiv_oracle.c orc_synth_*.  Writes packed reads straight into HBM. */
int rfx_dev_synth_genome(rfx_ctx *ctx, uint64_t seed, int64_t genome_len, uint64_t *d_genome);
int rfx_dev_synth_reads(rfx_ctx *ctx, uint64_t seed, const uint64_t *d_genome, int64_t genome_len,
                        int64_t first_read, int64_t n_reads, int read_len, uint32_t err_per_2_32,
                        int words_per_read, uint64_t *d_words);

/* Plain stable radix sort of (key, value) pairs in HBM -- exposed for tests and for the
 * driver; d_tmp_* are same-sized scratch arrays. key_bits = significant low bits. */
int rfx_dev_sort_pairs(rfx_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, int64_t n,
                       int key_bits, uint64_t *d_tmp_keys, uint32_t *d_tmp_vals);

/* Timing of the last rfx_dev_count_* call, per kernel family, from HIP events recorded on
 * the context's stream (ms).  names: "hist1","part1","hist2","part2","leaf","sort". */
int rfx_last_count_timing(rfx_ctx *ctx, const char *name, float *ms, int64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
