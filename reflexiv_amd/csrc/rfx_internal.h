// rfx_internal.h -- host-side plumbing shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <time.h>
#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>
#include <map>
#include "../../include/reflexiv_hip.h"
#include "rfx_asm_loop.h"

struct rfx_timing_slot { float ms = 0.f; int64_t launches = 0; };
// a kernel timer that has been stopped and not yet read (ScopedTimer below): events of the context's own pool
struct rfx_timer_pending { const char *name; hipEvent_t a, b; int64_t launches; };

// RFX_POISON=1 (debugging): every fresh workspace slot and every scratch allocation is filled with 0xA5 before it is handed
// out, so a kernel that reads what nobody wrote sees the same junk in a fresh process as deep into a test session.
// A bit mask: 1 = fresh workspace slots, 2 = scratch allocations (DevBuf), 4 = workspace slots 0 and 1 each time they are
// handed out again.
inline int rfx_poison() {
    static const int on = [] { const char *e = getenv("RFX_POISON"); return e && *e ? atoi(e) : 0; }();
    return on;
}

struct rfx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;
    std::string foreign_hip_error;        // a HIP error RCCL left on this thread (rfx_comm.hip note_foreign_hip_error): reported, never fatal
    std::string last_error_text;          // what rfx_last_error() hands out (last_error + the note above)
    int num_cu = 256;
    // per-kernel-family timing of the last count call (HIP events on `stream`)
    std::map<std::string, rfx_timing_slot> timing;
    bool timing_enabled = true;
    // stopped timers waiting for ScopedTimer::collect.  They belong to the CONTEXT, like the events they name: until round 4
    // this list was a thread_local, so a timer stopped on a path that never collected (order_wide2 through
    // rfx_dev_order_kmers_w, any early error return) outlived its context, and the next context's first collect() handed
    // destroyed events to hipEventElapsedTime -- the host abort of gpurun_out/s3_both.log.
    std::vector<rfx_timer_pending> timers_pending;
    // grow-only workspace slots for the large, reused buffers (instance arrays of the count
    // stage): allocated once with hipMalloc, kept until the context dies
    struct WsSlot { void *p = nullptr; size_t bytes = 0; };
    WsSlot ws[7];          // 0, 1: the count stage's record / instance buffers; 2, 3: the extend stage's arenas; 4: the count stage's arena;
                           // 5, 6: rfx_assemble_reads' ASCII staging and packed reads (multi-gigabyte stream-ordered allocations of
                           // changing sizes cost 100-600 ms a call in the pool; these are allocated once and kept)
    void *ws_get(int slot, size_t bytes) {
        WsSlot &w = ws[slot];
        if (w.bytes >= bytes && w.p) {
            // slots 0 and 1 are only ever asked for as the DESTINATION of the next kernel (rfx_kmer.hip, rfx_count_sk.hip)
            if ((rfx_poison() & 4) && slot < 2) (void)hipMemsetAsync(w.p, 0xA5, bytes, stream);
            return w.p;
        }
        if (w.p) { (void)hipStreamSynchronize(stream); (void)hipFree(w.p); w.p = nullptr; w.bytes = 0; }
        size_t want = bytes + (bytes >> 4) + (1 << 20);
        if (hipMalloc(&w.p, want) != hipSuccess) { w.p = nullptr; return nullptr; }
        if (rfx_poison() & 1) (void)hipMemsetAsync(w.p, 0xA5, want, stream);
        if (rfx_poison() & 8) { (void)hipMemset(w.p, 0, want); (void)hipDeviceSynchronize(); }      // (8: zeros, the same way)
        w.bytes = want;
        return w.p;
    }
    void ws_free() {
        for (auto &w : ws) { if (w.p) (void)hipFree(w.p); w.p = nullptr; w.bytes = 0; }
        if (pinned) (void)hipHostFree(pinned);
        pinned = nullptr; pinned_bytes = 0;
        if (scan_desc) (void)hipFree(scan_desc);
        if (scan_ticket) (void)hipFree(scan_ticket);
        if (scan_fault) (void)hipHostFree(scan_fault);
        scan_fault = nullptr;
        if (mailbox) (void)hipHostFree((void *)mailbox);
        mailbox = nullptr;
        scan_desc = nullptr; scan_ticket = nullptr; scan_desc_cap = 0;
        timers_pending.clear();
        for (auto e : ev_pool) (void)hipEventDestroy(e);
        ev_pool.clear(); ev_next = 0;
    }
    // grow-only pinned host staging for result downloads (a pageable copy of a few MB costs
    // milliseconds the first time the runtime stages it)
    // events of the kernel timers: created once, handed out round-robin until the next collect()
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;
    hipEvent_t ev_get() {
        if (ev_next == ev_pool.size()) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return nullptr; ev_pool.push_back(e); }
        return ev_pool[ev_next++];
    }
    // single-pass scans (rfx_scan.hip): tile descriptors and the ticket counter live in the context; a descriptor is
    // valid only under the epoch of the call that wrote it, so nothing is cleared between calls
    uint64_t *scan_desc = nullptr;
    size_t scan_desc_cap = 0;              // descriptors (two per tile for the dual scan)
    unsigned long long *scan_ticket = nullptr;
    int *scan_fault = nullptr;             // host-mapped: set by a look-back that gave up (never expected)
    unsigned long long scan_tickets_issued = 0;
    uint32_t scan_epoch = 0;
    // A mailbox in host-mapped pinned memory: the last (one-workgroup) kernel of a chain writes up to seven values and then a
    // sequence number into it, the host spins on the number instead of queueing a 24-byte copy and waiting for the stream
    // (mailbox_wait below).  The extend stage waits twice per pass for a handful of bytes; a stream wait + the copy cost 25-40 us
    // each, the mailbox a few.  RFX_MAILBOX=0: the copies again.
    volatile uint64_t *mailbox = nullptr;          // [0] sequence, [1..7] values
    uint64_t mailbox_seq = 0;
    void *pinned = nullptr;
    size_t pinned_bytes = 0;
    void *pinned_get(size_t bytes) {
        if (pinned && pinned_bytes >= bytes) return pinned;
        if (pinned) { (void)hipStreamSynchronize(stream); (void)hipHostFree(pinned); pinned = nullptr; pinned_bytes = 0; }
        size_t want = bytes + (bytes >> 2) + (1 << 20);
        if (hipHostMalloc(&pinned, want, hipHostMallocDefault) != hipSuccess) { pinned = nullptr; return nullptr; }
        pinned_bytes = want;
        return pinned;
    }
};

#define RFX_HIP(call)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            char buf_[512];                                                               \
            snprintf(buf_, sizeof buf_, "%s:%d: %s -> %s", __FILE__, __LINE__, #call,     \
                     hipGetErrorString(e_));                                              \
            if (ctx) ctx->last_error = buf_;                                              \
            return RFX_E_HIP;                                                             \
        }                                                                                 \
    } while (0)

// The boundary keeps its word ("never aborts", include/reflexiv_hip.h): every extern "C" entry point is a function-try-block
// that ends in one of these, so a C++ exception raised under it (std::bad_alloc from a vector or a map, std::system_error
// from a thread, std::length_error ...) becomes RFX_E_HOST with its what() in rfx_last_error() instead of std::terminate
// inside the JVM / Python process that loaded the library.
int rfx_api_exception(rfx_ctx *ctx, const char *where) noexcept;
#define RFX_API_CATCH(ctxexpr) catch (...) { return rfx_api_exception((ctxexpr), __func__); }
#define RFX_API_CATCH_VOID(ctxexpr) catch (...) { (void)rfx_api_exception((ctxexpr), __func__); }

#define RFX_TRY(call)                              \
    do {                                           \
        int s_ = (call);                           \
        if (s_ != RFX_OK) return s_;               \
    } while (0)

// Every host wait on the context's stream goes through here: a single-pass scan whose look-back gave up (rfx_scan.hip:
// it substitutes prefix 0 and raises the host-mapped flag) fails the call that waited, not some later one.
static inline int sync_checked(rfx_ctx *ctx) {
    hipError_t e_ = hipStreamSynchronize(ctx->stream);
    if (e_ != hipSuccess) {
        ctx->last_error = std::string("hipStreamSynchronize -> ") + hipGetErrorString(e_);
        return RFX_E_HIP;
    }
    if (ctx->scan_fault && *ctx->scan_fault) {
        *ctx->scan_fault = 0;
        ctx->last_error = "scan: look-back gave up waiting for a predecessor tile (offsets of this call are invalid)";
        return RFX_E_HIP;
    }
    return RFX_OK;
}

// The mailbox (see rfx_ctx): mailbox_next() -> the number the kernel must post (0: no mailbox, use a copy + sync_checked);
// mailbox_wait() spins for it -- everything queued before the posting kernel has completed by then -- and falls back to a
// stream wait after two seconds (a faulted kernel never posts) or when the stream already reports an error.
static inline uint64_t mailbox_next(rfx_ctx *ctx) {
    static const bool off = [] { const char *e = getenv("RFX_MAILBOX"); return e && atoi(e) == 0; }();
    if (off) return 0;
    if (!ctx->mailbox) {
        void *p = nullptr;
        if (hipHostMalloc(&p, 64, hipHostMallocMapped) != hipSuccess) return 0;
        memset(p, 0, 64);
        ctx->mailbox = (volatile uint64_t *)p;
        ctx->mailbox_seq = 0;
    }
    return ++ctx->mailbox_seq;
}
static inline int mailbox_wait(rfx_ctx *ctx, uint64_t seq, uint64_t *vals, int nvals) {
    timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint64_t spins = 0;; spins++) {
        if (ctx->mailbox[0] == seq) break;
        if ((spins & 0xFFF) == 0xFFF) {
            timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) * 1000 + (t1.tv_nsec - t0.tv_nsec) / 1000000 > 2000) {
                const int st = sync_checked(ctx);
                if (st != RFX_OK) return st;
                if (ctx->mailbox[0] != seq) { ctx->last_error = "mailbox: the posting kernel finished without posting"; return RFX_E_STATE; }
                break;
            }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    for (int i = 0; i < nvals; i++) vals[i] = ctx->mailbox[1 + i];
    if (ctx->scan_fault && *ctx->scan_fault) {
        *ctx->scan_fault = 0;
        ctx->last_error = "scan: look-back gave up waiting for a predecessor tile (offsets of this call are invalid)";
        return RFX_E_HIP;
    }
    return RFX_OK;
}

// up to 56 bytes of device memory to the host through the mailbox (one tiny launch instead of a queued copy + a stream wait);
// anything larger, or with the mailbox off: the copy and sync_checked.  Everything queued before it has completed on return.
int small_readback(rfx_ctx *ctx, void *h_dst, const void *d_src, size_t nbytes);

// Bump arena for the temporaries of one pass of the extend loop: two of them alternate, so a
// pass reads its inputs from the previous pass's arena and nothing is allocated or freed per pass
// (hipMallocAsync with ever-changing sizes cost ~5 ms per pass, far more than the kernels).
struct Arena { char *base = nullptr; size_t cap = 0, off = 0; };
inline thread_local Arena *tl_arena = nullptr;

// Stream-ordered scratch allocation that frees itself (or a slice of the current arena).
struct DevBuf {
    void *p = nullptr;
    hipStream_t s = nullptr;
    bool borrowed = false;        // points into a context workspace slot: never freed here
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), s(o.s), borrowed(o.borrowed) { o.p = nullptr; o.borrowed = false; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; s = o.s; borrowed = o.borrowed; o.p = nullptr; o.borrowed = false; }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t bytes, hipStream_t stream) {
        release();
        s = stream;
        if (bytes == 0) bytes = 16;
        if (tl_arena) {
            const size_t need = (bytes + 255) & ~(size_t)255;
            if (tl_arena->off + need <= tl_arena->cap) {
                p = tl_arena->base + tl_arena->off;
                tl_arena->off += need;
                borrowed = true;
                if (rfx_poison() & 2) (void)hipMemsetAsync(p, 0xA5, bytes, stream);
                return hipSuccess;
            }
        }
        hipError_t e = hipMallocAsync(&p, bytes, stream);
        if (e == hipSuccess && (rfx_poison() & 2)) (void)hipMemsetAsync(p, 0xA5, bytes, stream);
        return e;
    }
    void release() {
        if (p && !borrowed) (void)hipFreeAsync(p, s);
        p = nullptr; borrowed = false;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// The temporaries of one count-stage call (histogram tables, scans, hole lists, sort buffers) from one bump arena the
// context keeps (workspace slot 4): the stream-ordered allocator left the GPU idle for half a millisecond between the
// levels of every step (30.9 -> 28.6 ms per step).  Nothing if an arena is already active; a request the arena cannot
// take goes to the stream-ordered allocator as before.
struct StageArena {
    Arena arena;
    Arena *prev;
    bool on = false;
    StageArena(rfx_ctx *ctx, size_t bytes) : prev(tl_arena) {
        if (tl_arena) return;
        arena.base = (char *)ctx->ws_get(4, bytes);
        if (arena.base) { arena.cap = bytes; tl_arena = &arena; on = true; }
    }
    ~StageArena() { if (on) tl_arena = prev; }
    StageArena(const StageArena &) = delete;
    StageArena &operator=(const StageArena &) = delete;
};

// The two alternating bump arenas of the extend drivers (workspace slots 2 and 3, `bytes` each): next() turns to the other
// one and empties it, so what the step before allocated stays valid for exactly one more step.  No arena once it is gone.
struct ArenaPair {
    Arena arena[2];
    int turn = 0;
    Arena *prev;
    ArenaPair() : prev(tl_arena) {}
    ~ArenaPair() { tl_arena = prev; }
    ArenaPair(const ArenaPair &) = delete;
    ArenaPair &operator=(const ArenaPair &) = delete;
    bool init(rfx_ctx *ctx, size_t bytes) {
        for (int i = 0; i < 2; i++) {
            arena[i].base = (char *)ctx->ws_get(2 + i, bytes);
            if (!arena[i].base) return false;
            arena[i].cap = bytes;
        }
        return true;
    }
    void next() { Arena *a = &arena[turn++ & 1]; a->off = 0; tl_arena = a; }
};
// No arena inside this block: what is allocated here comes from the stream-ordered allocator and outlives the arenas' turns.
struct ArenaOff {
    Arena *prev;
    ArenaOff() : prev(tl_arena) { tl_arena = nullptr; }
    ~ArenaOff() { tl_arena = prev; }
    ArenaOff(const ArenaOff &) = delete;
    ArenaOff &operator=(const ArenaOff &) = delete;
};

// Event pair that accumulates into ctx->timing[name].
struct ScopedTimer {
    rfx_ctx *ctx; const char *name; hipEvent_t a = nullptr, b = nullptr; bool on;
    ScopedTimer(rfx_ctx *c, const char *n) : ctx(c), name(n), on(c && c->timing_enabled) {
        if (on) { a = ctx->ev_get(); b = ctx->ev_get(); on = a && b; }
        if (on) (void)hipEventRecord(a, ctx->stream);
    }
    void stop(int64_t launches = 1) {
        if (!on) return;
        (void)hipEventRecord(b, ctx->stream);
        ctx->timers_pending.push_back({name, a, b, launches});
        on = false;
    }
    ~ScopedTimer() { stop(); }
    // call after a stream sync (a timer whose events have not completed is dropped, not waited for)
    static void collect(rfx_ctx *ctx) {
        for (auto &p : ctx->timers_pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
                ctx->timing[p.name].ms += ms;
                ctx->timing[p.name].launches += p.launches;
            }
        }
        ctx->timers_pending.clear();
        ctx->ev_next = 0;                  // the pool's events are free again
    }
};

static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
// Every kernel launch of the library: on the context's stream, and checked -- a launch that failed (a bad shape, too much LDS)
// returns RFX_E_HIP from the CALLER with the line of the launch in last_error, which is why these are macros.
#define RFX_LAUNCH(kernel, grid, block, lds_bytes, ...)                                          \
    do {                                                                                         \
        hipLaunchKernelGGL(kernel, grid, block, lds_bytes, ctx->stream, ##__VA_ARGS__);          \
        RFX_HIP(hipGetLastError());                                                              \
    } while (0)
// the shape of the one-thread-per-item kernels: ceil(n / 256) blocks (one for n = 0) of 256 threads, no LDS
#define RFX_LAUNCH_N(kernel, n, ...) \
    RFX_LAUNCH(kernel, dim3((unsigned)ceil_div(std::max<int64_t>((n), 1), 256)), dim3(256), 0, ##__VA_ARGS__)
// scratch for `count` elements of T
#define RFX_ALLOC(buf, T, count) RFX_HIP((buf).alloc((size_t)(count) * sizeof(T), ctx->stream))

namespace rfx {

// ---- rfx_scan.hip
int exclusive_scan_u64(rfx_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, int64_t n);   // out[n] = total (n+1 entries)
int exclusive_scan_u32_to_u64(rfx_ctx *ctx, const uint32_t *d_in, uint64_t *d_out, int64_t n);
// two arrays in one launch (the emission indices and the word offsets of an extend pass)
int exclusive_scan2_u32_to_u64(rfx_ctx *ctx, const uint32_t *d_in_a, const uint32_t *d_in_b, uint64_t *d_out_a,
                               uint64_t *d_out_b, int64_t n);

// ---- rfx_sort.hip
int sort_pairs(rfx_ctx *ctx, uint64_t *d_keys, uint32_t *d_vals, int64_t n, int key_bits,
               uint64_t *d_tmp_keys, uint32_t *d_tmp_vals);   // result in d_keys/d_vals

// ---- the count stage: rfx_kmer.hip, and rfx_count_sk.hip for level 1 of the record paths (the bucket_*records_by_owner* calls);
// what the two units share among themselves is in rfx_count.h
struct ReadStore {
    const uint64_t *words; int64_t n_reads; int words_per_read; int read_len;
    int k, front_clip, end_clip;
    // ragged reads: per-read lengths in HBM (read_len is then the maximum) and the exact number of
    // k-mer instances (-1: uniform reads, kmers_per_read(read_len) each)
    const uint32_t *read_len_arr = nullptr;
    int64_t n_instances = -1;
};
// wide: the k > 31 counter's skip rule (k = 33..63 reads; kmers_per_read_w), else the k <= 31 one
int ragged_instances(rfx_ctx *ctx, const uint32_t *d_read_len, int64_t n_reads, int k, int front_clip,
                         int end_clip, int64_t *out_total, bool wide = false);
int64_t kmers_per_read(int read_len, int k, int front_clip, int end_clip);
int encode_reads(rfx_ctx *ctx, const uint8_t *d_bases, const int64_t *d_read_off, int64_t n_reads,
                 int words_per_read, uint64_t *d_words, uint32_t *d_read_len);
int extract_ordered_packed(rfx_ctx *ctx, const uint64_t *d_words, int wpr, const uint64_t *d_kmer_off,
                           int64_t n_reads, int k, int front_clip, uint64_t *d_out);
int kmer_counts_per_read(rfx_ctx *ctx, const int64_t *d_read_off, int64_t n_reads, int k,
                         int front_clip, int end_clip, uint64_t *d_nk);
int64_t count_workspace_bytes(int64_t n_kmers);
int count_filter(rfx_ctx *ctx, const ReadStore *reads, const uint64_t *d_kmers, int64_t n,
                 int min_cov, int max_cov, int twin, void *ws, int64_t ws_bytes,
                 uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap,
                 int64_t *out_n, int64_t *out_distinct, bool pair_out = false);
int bucket_pairs_by_owner(rfx_ctx *ctx, const void *d_pairs, int64_t n, int n_owners, void *d_out,
                          int64_t *d_owner_off, int64_t *h_owner_off);
int merge_pairs(rfx_ctx *ctx, const void *d_pairs, int64_t n, int k, int min_cov, int max_cov, int twin,
                uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap, int64_t *out_n, int64_t *out_distinct);
int bucket_by_owner(rfx_ctx *ctx, const ReadStore *reads, int n_owners, uint64_t *d_out,
                    int64_t cap, int64_t *d_owner_off, int64_t *h_owner_off);
int bucket_records_by_owner_sweep(rfx_ctx *ctx, const ReadStore *reads, int n_owners, void *d_out, int64_t cap_records,
                                  int64_t *h_begin, int64_t *h_end, int64_t *out_n_records, bool *done);
int bucket_wide_records_by_owner_sweep(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                                       int n_owners, void *d_out, int64_t cap_records, int64_t *h_begin, int64_t *h_end,
                                       int64_t *out_n_records, bool *done, const uint32_t *d_read_len = nullptr, int ec = 0);
int bucket_records_by_owner(rfx_ctx *ctx, const ReadStore *reads, int n_owners, void *d_out, int64_t cap_records,
                            int64_t *d_owner_off, int64_t *h_owner_off, int64_t *out_n_records);
int count_records(rfx_ctx *ctx, const void *d_records, int64_t n_records, int64_t n_instances_hint, int k,
                  int min_cov, int max_cov, int twin, uint64_t *d_out_keys, int32_t *d_out_counts, int64_t cap,
                  int64_t *out_n, int64_t *out_distinct);
int bucket_wide_records_by_owner(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                                 int n_owners, void *d_out, int64_t cap_records, int64_t *d_owner_off, int64_t *h_owner_off,
                                 int64_t *out_n_records, const uint32_t *d_read_len = nullptr, int ec = 0);
int count_wide_records(rfx_ctx *ctx, const void *d_records, int64_t n_records, int64_t n_instances_hint, int k, int min_cov,
                       int max_cov, uint64_t *d_out_keys, int64_t *d_out_counts, int64_t cap, int64_t *out_n,
                       int64_t *out_distinct);
// ragged reads: d_read_len (per-read lengths; nk = the longest read's k-mers), their end clip and instances
int count_wide2_reads(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                      int min_cov, int max_cov, uint64_t *d_out_keys, int64_t *d_out_counts, int64_t cap, int64_t *out_n,
                      int64_t *out_distinct, const uint32_t *d_read_len = nullptr, int ec = 0, int64_t n_inst = -1);
int bucket_wide_by_owner(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                         int n_owners, void *d_out, int64_t cap_elems, int64_t *d_owner_off, int64_t *h_owner_off);
// the element path (rfx_kmer.hip): AoS W-word elements (W = 2..4: k = 33..127; two-word elements at 16-byte multiples) ->
// distinct keys and counts, unordered; the same from packed reads at W = 3, 4 (uniform, or d_read_len with nk = the longest
// read's k-mers and n_inst their instances; W = 2 goes through count_wide2_reads); the k-mers of packed reads grouped by
// owning rank (W = 2..4; AoS elements, offsets as bucket_wide_by_owner)
int count_wide_elems(rfx_ctx *ctx, const void *d_elems, int64_t n, int k, int min_cov, int max_cov, uint64_t *d_out_keys,
                     int64_t *d_out_counts, int64_t cap, int64_t *out_n, int64_t *out_distinct);
int count_wide_n_from_reads(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                            int min_cov, int max_cov, uint64_t *d_out_keys, int64_t *d_out_counts, int64_t cap, int64_t *out_n,
                            int64_t *out_distinct, const uint32_t *d_read_len = nullptr, int ec = 0, int64_t n_inst = -1);
int bucket_wide_n_by_owner(rfx_ctx *ctx, const uint64_t *d_words, int64_t n_reads, int wpr, int64_t nk, int k, int fc,
                           const uint32_t *d_read_len, int ec, int n_owners, void *d_out, int64_t *d_owner_off, int64_t *h_owner_off);
// ---- rfx_synth.hip : the benchmark's reads, generated on the device
int synth_genome(rfx_ctx *ctx, uint64_t seed, int64_t genome_len, uint64_t *d_genome);
int synth_reads(rfx_ctx *ctx, uint64_t seed, const uint64_t *d_genome, int64_t genome_len,
                int64_t first_read, int64_t n_reads, int read_len, uint32_t err, int words_per_read,
                uint64_t *d_words);

// ---- rfx_wide.hip : k > 31, W = k/32+1 words per k-mer (the counter's layout)
int check_k_w(int k);
int64_t kmers_per_read_w(int read_len, int k, int fc, int ec);
int kmer_counts_per_read_w(rfx_ctx *ctx, const int64_t *d_read_off, int64_t n_reads, int k, int fc, int ec,
                           uint64_t *d_nk);
int extract_w(rfx_ctx *ctx, const uint64_t *d_words, int wpr, const uint64_t *d_kmer_off, int64_t nk_uniform,
              int64_t n_reads, int k, int fc, uint64_t *d_soa, int64_t N, int aos = 0);
bool wide_fast_path(int k);
bool wide_elem_path(int k);      // W = 2..4 (k = 33..127, k % 32 != 0): the bucketed count on the device
// (the survivors of W = 2..4 ordered; N AoS elements of W = 2..4 words counted, filtered and ordered)
int order_wide2(rfx_ctx *ctx, uint64_t *d_out_keys, int64_t *d_out_counts, int64_t m, int k);
int count_filter_w2(rfx_ctx *ctx, const uint64_t *d_elems, int64_t N, int k, int min_cov, int max_cov,
                    uint64_t *d_out_keys, int64_t *d_out_counts, int64_t cap, int64_t *out_n, int64_t *out_distinct);
int aos_to_soa(rfx_ctx *ctx, const uint64_t *d_aos, int64_t n, int W, uint64_t *d_soa);
int soa_to_aos(rfx_ctx *ctx, const uint64_t *d_soa, int64_t n, int W, uint64_t *d_aos);
int count_filter_w(rfx_ctx *ctx, uint64_t *d_soa, int64_t N, int k, int min_cov, int max_cov, uint64_t *d_out_keys,
                   int64_t *d_out_counts, int64_t cap, int64_t *out_n, int64_t *out_distinct);

// ---- rfx_graph.hip : device record set (reference layout, in HBM)
struct DevRecords {
    int64_t n = 0, words = 0;
    int kw = 1;                 // words per key (AoS): 1 up to k = 32, (k-2)/31+1 beyond
    DevBuf key, marker, ext_off, ext, left, right;
};
inline int sub_words(int k) { return k <= 32 ? 1 : (k - 2) / 31 + 1; }     // subKmerBinarySlots, U/DefaultParam.java:94
inline int asm_words(int k) { return k <= 31 ? 1 : (k - 1) / 31 + 1; }     // kmerBinarySlotsAssemble, U/DefaultParam.java:85
constexpr int MAX_KEY_WORDS = 4;                                           // k <= 125
int dev_records_alloc(rfx_ctx *ctx, DevRecords &r, int64_t cap_n, int64_t cap_words, int kw = 1);
int dev_records_upload(rfx_ctx *ctx, const rfx_records *h, DevRecords &d);
int dev_records_download(rfx_ctx *ctx, const DevRecords &d, rfx_records *h);
// the fixed fields and the extension words of `src` into `dst` from record `record_at` / word `word_at` on (queued; ext_off, n
// and words of `dst` are the caller's: only a copy to the front keeps the offsets)
int dev_records_copy(rfx_ctx *ctx, const DevRecords &src, DevRecords &dst, int64_t record_at = 0, int64_t word_at = 0);

int rc_expand_subkmer(rfx_ctx *ctx, const uint64_t *d_kmers, const int32_t *d_counts, int64_t n,
                      int k, DevRecords &out);
// key_bits: significant bits of a one-word key (ignored for kw > 1: k gives the word widths)
int sort_records(rfx_ctx *ctx, const DevRecords &in, int P, int key_bits, DevRecords &out,
                 DevBuf &part_start /* int64[P+1] */, int k = 0);
int counter_to_asm(rfx_ctx *ctx, const uint64_t *d_keys32, const int64_t *d_counts64, int64_t n, int k, int min_cov,
                   int max_cov, uint64_t *d_out31, int32_t *d_out_counts, int64_t *out_n);
int fork_filter(rfx_ctx *ctx, bool reflected, const DevRecords &in, const int64_t *d_part_start,
                int P, int k, int min_error_cov, int twin, DevRecords &out,
                DevBuf &out_part_start);
int reflect_from_forward(rfx_ctx *ctx, const DevRecords &in, int k, DevRecords &out);
// Several GPUs (rfx_shard.hip): a logical partition may begin on an earlier rank.  What it brings from there is the PARITY
// of a count -- records for the random reflection, emissions for an extend pass -- as device int32[2] = {partition, parity}.
// The extend pass learns its count only after its scan, so it calls back between the scan and the emission.
struct PartCarry {
    virtual ~PartCarry() {}
    // d_cum: n + 1 prefix counts of the quantity whose parity decides (nullptr: the record index itself)
    virtual int compute(rfx_ctx *ctx, const int64_t *d_part_start, int P, const uint64_t *d_cum, int64_t n, const int32_t **d_carry) = 0;
};
int random_reflection(rfx_ctx *ctx, const DevRecords &in, const int64_t *d_part_start, int P,
                      int k, DevRecords &out, const int32_t *d_carry = nullptr);
int extend_pass(rfx_ctx *ctx, const DevRecords &in, const int64_t *d_part_start, int P, int k,
                int twin, int stage, DevRecords &out, DevBuf &out_part_start, int start_marker = 2, PartCarry *carry_hook = nullptr);

// the k > 31 from-counts extras (P/ReflexivDSMain64.java:584-619, 672-712): op 0 DSReflexivAndForwardKmer (2n out),
// 1 DSFilterExtendableKmerPairs, 2 DSFilterUnExtendableKmer, 3 DSFilterStillExtendableKmerFromPairs,
// 4 DSFilterStillExtendableKmerEnds, 5 / 6 DSFilterUnExtendableKmerLeftEnds / ...RightEnds
int extras_operator(rfx_ctx *ctx, int op, const DevRecords &in, const int64_t *d_part_start, int P, int k, DevRecords &out,
                    DevBuf &out_part_start);
// the driver (rfx_api.hip), and the state with which the sharded driver (rfx_shard.hip) hands its loop over to it
struct AsmResume {
    DevRecords *recs;            // the record set, in global arrival order (taken over)
    AsmLoop loop;                // the loop's variables as they stood (passes_done 0..4: passes before the loop are still to come)
};
int assemble_impl(rfx_ctx *ctx, bool wide, const uint64_t *d_keys, const int32_t *d_counts, int64_t n, const rfx_params *prm,
                  char *out, int64_t cap, int64_t *out_len, int64_t *out_contigs, int64_t *trace, int64_t trace_cap,
                  int64_t *n_trace, AsmResume *resume);
// the rest of the driver's loop on <= small_pass_limit() records: two launches per pass, state in HBM (rfx_extend.hip)
int small_passes(rfx_ctx *ctx, DevRecords &recs, int k, int twin, AsmLoop &loop, const AsmRule &rule, int64_t *trace,
                 int64_t trace_cap);
int small_pass_limit();
int small_pass_max_partitions();

// ---- rfx_dynamic.hip : a packed dynamic-k record set in HBM (rfx_dyn_packed), shared with every stage on packed sets
struct DynDev {                       // a packed record set in HBM
    int64_t n = 0, words = 0;         // records; a BOUND on the extension words (the exact count is ext_off[n], in HBM)
    DevBuf key, key_len, ext, ext_off, ext_len, marker, left, right;
};
// what the kernels take
struct DynView {
    const uint64_t *key; const uint8_t *key_len; const uint64_t *ext; const int64_t *ext_off; const int32_t *ext_len, *marker, *left, *right;
};
struct DynOut {
    uint64_t *key; uint8_t *key_len; uint64_t *ext; int64_t *ext_off; int32_t *ext_len, *marker, *left, *right;
};
inline DynView dyn_view(const DynDev &d) {
    return DynView{d.key.as<uint64_t>(), d.key_len.as<uint8_t>(), d.ext.as<uint64_t>(), d.ext_off.as<int64_t>(), d.ext_len.as<int32_t>(),
                   d.marker.as<int32_t>(), d.left.as<int32_t>(), d.right.as<int32_t>()};
}
inline DynOut dyn_out(const DynDev &d) {
    return DynOut{d.key.as<uint64_t>(), d.key_len.as<uint8_t>(), d.ext.as<uint64_t>(), d.ext_off.as<int64_t>(), d.ext_len.as<int32_t>(),
                  d.marker.as<int32_t>(), d.left.as<int32_t>(), d.right.as<int32_t>()};
}
int dyn_alloc(rfx_ctx *ctx, DynDev &d, int64_t n, int64_t words);
// The flags of one call of a stage on packed sets, in HBM: what is wrong with the input (a mask of the stage's own bits), the
// shortest and the longest key (pk_note_lengths, rfx_packed_words.h) and up to three 64-bit totals -- one small read-back for all of
// them.  call_flags_init: zeros, min_len = 2^32 - 1.  call_flags_read: one one-thread launch (k_put_totals) copies *t0, *t1, *t2
// (each may be nullptr: 0) into total[], then the read-back; everything queued before it has completed on return.
struct CallFlags { uint32_t bad, min_len, max_len, pad; uint64_t total[3]; };
int call_flags_init(rfx_ctx *ctx, DevBuf &flags);
int call_flags_read(rfx_ctx *ctx, const DevBuf &flags, const uint64_t *d_t0, const uint64_t *d_t1, const uint64_t *d_t2, CallFlags *h);
// host checks of the entry points and operators: a caller's output set has its arrays (n is the callee's to set) / an input set
// has them and n >= 0 / text rows are (n >= 0, and pointers where n > 0) / an empty set in the library's own buffers / the
// caller's partition starts -- P + 1 entries, 0 first, n last, never running backwards -- read back and checked BEFORE a kernel
// indexes with them ("<stage>: partition starts that do not run from 0 to n")
bool dyn_packed_out_ok(const rfx_dyn_packed *p);
bool dyn_packed_ok(const rfx_dyn_packed *p);
bool text_rows_ok(const char *text, const int64_t *row_off, int64_t n);
int dyn_empty(rfx_ctx *ctx, DynDev &d);
int check_part_starts(rfx_ctx *ctx, const int64_t *d_ps, int P, int64_t n, const char *stage_name);
#pragma GCC visibility push(hidden)                               // (the library's own: its exported symbols stay as they were)
bool parts_ok(int P);                                              // 1 <= P <= 63: what the one-workgroup partition kernels take
// host steps the stages share.  scan_keep: d_rank[0..n] = the exclusive scan of n keep flags, *total = d_rank[n] read back (one host
// wait; a site whose CallFlags read-back carries the total does not use it).  part_starts_alloc: out_ps = int64[P + 1], zeros when
// `zeroed` (the empty set).  part_starts_store: P + 1 entries of ops into the caller's device array, then the wait that ends the call.
// out_part_starts: d_out[p] = d_prefix[d_ps[p]], p = 0..P (one workgroup of 64).  index_kept: d_idx[d_rank[i]] = i where d_keep[i]
int scan_keep(rfx_ctx *ctx, const uint32_t *d_keep, int64_t n, uint64_t *d_rank, int64_t *total);
int part_starts_alloc(rfx_ctx *ctx, DevBuf &out_ps, int P, bool zeroed);
int part_starts_store(rfx_ctx *ctx, int64_t *d_dst, const DevBuf &ops, int P);
int out_part_starts(rfx_ctx *ctx, const int64_t *d_ps, int P, const uint64_t *d_prefix, int64_t *d_out);
int index_kept(rfx_ctx *ctx, const uint32_t *d_keep, const uint64_t *d_rank, int64_t n, int64_t *d_idx);
// The tail of the host-text entry points: every length out, then the texts from the library's buffers to the caller's, one wait.
// A buffer that is too short gives RFX_E_CAP with every length set, and there are two behaviours, kept per entry point:
// fill_to_cap (rfx_dyn_run_text, rfx_ksort_text): each buffer is filled up to its capacity; otherwise (rfx_reduce_text, rfx_fix_text,
// rfx_fix2_text): nothing is written and nothing is waited for
struct TextOut { const DevBuf &d; int64_t total; char *out; int64_t cap; int64_t *out_len; };
int text_to_host(rfx_ctx *ctx, std::initializer_list<TextOut> outs, bool fill_to_cap);
#pragma GCC visibility pop
// sort("k-1") + the cut into P logical partitions: in -> out (sorted), d_ps[P + 1]; *lmin = the shortest key
int dyn_sort(rfx_ctx *ctx, const DynDev &in, int P, DynDev &out, DevBuf &d_ps, uint32_t *lmin);
// a stable sort by a key of W 64-bit words in W columns of n entries, the most significant first: d_perm[q] = the item at position q
int sort_columns(rfx_ctx *ctx, const uint64_t *d_cols, int W, int64_t n, uint32_t *d_perm);
// a view of the caller's input set (nothing copied, nothing freed) / the result into the caller's arrays (both capacities are
// checked before anything is copied) / host text rows -> HBM with offsets relative to the first row
int dyn_borrow(rfx_ctx *ctx, const rfx_dyn_packed *p, DynDev &d);
int dyn_store(rfx_ctx *ctx, const DynDev &d, rfx_dyn_packed *o);
int dyn_upload_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, DevBuf &d_text, DevBuf &d_off);
// shared with rfx_fixing.hip: the text rows of a hand-over file in HBM -> a packed set (form 0 / 1 of rfx_dyn_binarize) / one extend
// pass over a sorted set and its P partition starts (lmin = the set's shortest key; d_out_ps optional) / the rows
// "SUBKMER,marker|left|right,EXTENSION\n" (own: a buffer of the library's)
int dyn_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, int form, DynDev &d);
int dyn_pass(rfx_ctx *ctx, const DynDev &in, const int64_t *d_ps, int P, uint32_t lmin, int stage, int start_iteration, int start_marker,
             DynDev &out, int64_t *d_out_ps);
int dyn_to_text(rfx_ctx *ctx, const DynDev &d, char *d_text, int64_t cap, int64_t *total, DevBuf *own);

// ---- rfx_ksort.hip, shared with rfx_reduce.hip: sub-k-mers -> full k-mers (marker 2: extension + key, marker 1: key + extension; every
// extension one base) / the rows "KMER,marker|left|right\n" of the records whose key has k bases (own: a buffer of the library's)
int ks_set_full_kmers(rfx_ctx *ctx, const DynDev &in, DynDev &out);
int ks_set_to_text(rfx_ctx *ctx, const DynDev &d, int k, char *d_text, int64_t cap, int64_t *total, int64_t *d_row_off, int64_t *n_rows, DevBuf *own);
// ... and the choice that text writer makes, without the text: keep flags of the records whose key has len bases, their exclusive
// scan (n + 1 entries) and the total (one host wait; an empty set allocates nothing)
int ks_select_length(rfx_ctx *ctx, const DynDev &in, int len, DevBuf &keep, DevBuf &rank, int64_t *total);
// ... and for the driver from reads (rfx_reduce.hip): the body of rfx_dev_ksort_run_counts (its argument checks
// included) into a set of the library's / the body of rfx_dev_dyn_from_kmers on sets of the library's
int ks_run_counts(rfx_ctx *ctx, const uint64_t *d_keys, const void *d_counts, int count_bytes, int64_t n, const uint64_t *d_extra, int64_t n_extra,
                  const rfx_ksort_params *params, DynDev &out);
int ks_kmers_to_records(rfx_ctx *ctx, const DynDev *const *sets, const int *key_lens, int n_sets, DynDev &out, int64_t *kept_per_set = nullptr);
int ks_params_check(rfx_ctx *ctx, const rfx_ksort_params *params);   // what the sorter refuses of its parameters, nothing else

// ---- rfx_fixing.hip, shared with rfx_ctgext.hip: everything of the fixing stage behind its contig ends --
// the distinct end 31-mers (d_kmers, n31 values in emission order, left as they are) as one-base records + the long records, sort,
// fold, reflection, sort, fold, the loop once on the fold's partitions and min(max_iteration + 1, 17) times behind a sort
int fx_from_ends(rfx_ctx *ctx, const uint64_t *d_kmers, int64_t n31, const DynDev &lng, int P, int scramble, int max_iteration, DynDev &out);
// what a stage's contig ends left (lng as dyn_alloc or dyn_empty made it, so lng.words is the exact count) into the caller's arrays;
// both outputs are checked before either is written
int fx_ends_store(rfx_ctx *ctx, const DynDev &lng, const DevBuf &kmers, int64_t n31, rfx_dyn_packed *d_out_long, uint64_t *d_kmers, int64_t cap_kmers,
                  int64_t *n_kmers);

// ---- rfx_fixing2.hip : the second contig fixing stage
// text rows -> a packed set (form 1, no length filter; keys of 30 bases and extensions of one base or more, RFX_E_ARG otherwise) /
// min(max_iteration + 1, 29) x (sort, loop) on a set of such records, zero rounds copy it / the contigs of at least 2 max_k bases:
// what they take (plan), then into arrays that hold it (fill) / the rows of 05FixingAgain (ends 0) or the lines of 06ContigEnds
// (ends 1) or the rows of 09ExtendAgain (ends 2: left / right are not read) of a packed contig set (own: a buffer of the library's)
struct Fx2Plan { int64_t m = 0, words = 0; DevBuf keep, rank, woff; };
struct Fx2View { int64_t n; const uint64_t *w; const int64_t *woff, *len; const int32_t *left, *right; };
int fx2_binarize(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, DynDev &out);
int fx2_run(rfx_ctx *ctx, const DynDev &in, int P, int scramble, int max_iteration, DynDev &out);
int fx2_contigs_plan(rfx_ctx *ctx, const DynDev &in, int max_k, Fx2Plan &plan);
int fx2_contigs_fill(rfx_ctx *ctx, const DynDev &in, const Fx2Plan &plan, uint64_t *d_words, int64_t *d_word_off, int64_t *d_len, int32_t *d_left,
                     int32_t *d_right);
int fx2_text(rfx_ctx *ctx, const Fx2View &v, int ends, char *d_text, int64_t cap, int64_t *total, DevBuf *own);

// ---- rfx_endext.hip : the end extension of contigs from alignment rows
// the consensus of both ends of every contig of a set (Fx2View: a packed contig set with left / right) from text rows "name \t start
// \t cigar \t seq" in HBM: what both consensus sets take (plan), then into arrays that hold it (fill) / the order of the IDs and what
// the spliced set takes (plan), then reversed left || contig || right in output order (fill) / the rows of 07EndExtend (own: a buffer of
// the library's) / the rows of 05FixingAgain in HBM -> a packed contig set with left / right in the library's buffers
struct EeConsPlan { int64_t n = 0, lwords = 0, rwords = 0; DevBuf cons, clen, cflags, offl, offr; };
struct EeConsOut { uint64_t *lw; int64_t *lwoff, *llen; uint64_t *rw; int64_t *rwoff, *rlen; int32_t *flags; };
struct EeConsIn { const uint64_t *lw; const int64_t *lwoff, *llen; const uint64_t *rw; const int64_t *rwoff, *rlen; const int32_t *flags; };
struct EePlan { int64_t m = 0, words = 0; DevBuf perm, keep, nidx, opos, woff; };
struct EeSetOut { uint64_t *w; int64_t *woff, *len; int32_t *left, *right, *left_len, *right_len, *flags, *src_idx, *new_idx; };
struct EeSetIn { int64_t n; const uint64_t *w; const int64_t *woff, *len; const int32_t *left, *right, *left_len, *right_len, *flags, *src_idx, *new_idx; };
struct CtgDev;
int ee_consensus_plan(rfx_ctx *ctx, const Fx2View &in, const char *d_text, const int64_t *d_row_off, int64_t n_rows, EeConsPlan &plan);
int ee_consensus_fill(rfx_ctx *ctx, const EeConsPlan &plan, const EeConsOut &o);
int ee_contigs_plan(rfx_ctx *ctx, const Fx2View &in, const EeConsIn &c, int max_k, EePlan &plan);
int ee_contigs_fill(rfx_ctx *ctx, const Fx2View &in, const EeConsIn &c, const EePlan &plan, const EeSetOut &o);
int ee_text(rfx_ctx *ctx, const EeSetIn &s, char *d_text, int64_t cap, int64_t *total, DevBuf *own);
int ee_contigs_from_rows(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, CtgDev &c);

// ---- rfx_ctgext.hip : the contig extension stages
// the rows of 07EndExtend in HBM -> what the set of the rows of at least 2 max_k characters takes (plan), then into arrays that hold it
// (fill: the literals of a flagged seam as T bases, flags 0) / a set (flags 0..3) -> the long records of its cut contigs and the end
// 31-mers in emission order (kmers: a buffer of the library's)
struct ExRowsPlan { int64_t n = 0, m = 0, words = 0; DevBuf keep, rank, woff, fld, sbeg, slen; };
int ex_rows_plan(rfx_ctx *ctx, const char *d_text, const int64_t *d_row_off, int64_t n, int max_k, ExRowsPlan &plan);
int ex_rows_fill(rfx_ctx *ctx, const char *d_text, const ExRowsPlan &plan, const EeSetOut &o);
int ex_contig_ends(rfx_ctx *ctx, const EeSetIn &s, int max_k, DynDev &out, DevBuf &kmers, int64_t *n_kmers);

// ---- rfx_endmap.hip : reads onto the contig ends
// the parameters are in range (last_error says which is not) / the seed table of a contig set, the counting pass over the read store
// (d_words, d_read_len, words_per_read as rfx_dev_count_reads_ragged takes them) and the scan of its counts: plan.hits rows / the rows
// into arrays that hold them, in order / the rows as text "name \t start \t cigar \t seq \n" (filled up to cap) and their n + 1
// offsets (own: a buffer of the library's)
struct MpPlan { int64_t hits = 0, m = 0; DevBuf keys, vals, filter, cnt, hoff; };
struct MpHits { int32_t *read, *end, *strand, *off, *v; };
bool mp_params_ok(rfx_ctx *ctx, const rfx_map_params *p);
int mp_plan(rfx_ctx *ctx, const Fx2View &c, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, const rfx_map_params &p,
            MpPlan &plan);
int mp_fill(rfx_ctx *ctx, const Fx2View &c, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, const rfx_map_params &p,
            const MpPlan &plan, const MpHits &o);
int mp_text(rfx_ctx *ctx, const Fx2View &c, const uint64_t *d_words, const uint32_t *d_read_len, int wpr, const MpHits &hits, int64_t n, int seed,
            char *d_text, int64_t cap, int64_t *total, int64_t *d_row_off, DevBuf *own);
// ... and rfx_endext.hip on those rows without their text: ee_consensus_plan from the hits and the read store
int ee_consensus_plan_hits(rfx_ctx *ctx, const Fx2View &in, const uint64_t *d_words, const uint32_t *d_read_len, int wpr, const MpHits &hits,
                           int64_t n_hits, int seed, EeConsPlan &plan);

// ---- for rfx_meta.hip, the driver from reads to contigs: the bodies of rfx_dev_dyn_run (a is replaced by the
// result), rfx_dev_reduce_reads (and its argument checks) and rfx_dev_fix_run_packed on sets of the library's
int dyn_run_set(rfx_ctx *ctx, DynDev &a, int P, int random_reflection, int passes_first_four, int start_iteration, int end_iteration);
int rr_check_args(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, int max_read_len, const int *klist, int n_k,
                  const rfx_reduce_reads_params *p);
int rr_reduce_set(rfx_ctx *ctx, const uint64_t *d_words, const uint32_t *d_read_len, int64_t n_reads, int wpr, int max_read_len, const int *klist, int n_k,
                  const rfx_reduce_reads_params &p, DynDev &a, int64_t *per_k);
int fx_run_set(rfx_ctx *ctx, const DynDev &in, int P, const rfx_fix_params &params, DynDev &out);

// ---- packed contig sets in HBM (rfx_contigs_packed and what is built on it), shared by the four stages above: DESIGN.md section 27
#pragma GCC visibility push(hidden)
// What owns the buffers of a set the library makes for itself.  Every array has max(n, 1) entries (woff one more) and w max(words, 1)
// words, so an empty set still has something to point at; the *_alloc functions are the only places that know these rules.
struct CtgDev { int64_t n = 0, words = 0; DevBuf w, woff, len, left, right; };                  // a packed contig set with left / right
struct EeSetDev { int64_t n = 0, words = 0; DevBuf w, woff, len, i32; };                         // a set of 07EndExtend; i32: its seven int32 arrays, one block
struct EeConsDev { int64_t n = 0, lwords = 0, rwords = 0; DevBuf lw, lwoff, llen, rw, rwoff, rlen, flags; };    // both consensus sets of n contigs, their flags
struct MpHitsDev { int64_t n = 0; DevBuf i32; };                                                 // n rows of the end mapping; i32: its five int32 arrays, one block
inline size_t at_least_1(int64_t n) { return (size_t)std::max<int64_t>(n, 1); }
// (ee_contigs_from_rows learns the words only after it has filled the other arrays: it allocates the two halves apart, rows first)
inline int ctg_alloc_rows(rfx_ctx *ctx, CtgDev &c, int64_t n) {
    const size_t m = at_least_1(n);
    c.n = n;
    RFX_ALLOC(c.woff, int64_t, m + 1); RFX_ALLOC(c.len, int64_t, m); RFX_ALLOC(c.left, int32_t, m); RFX_ALLOC(c.right, int32_t, m);
    return RFX_OK;
}
inline int ctg_alloc_words(rfx_ctx *ctx, CtgDev &c, int64_t words) { c.words = words; RFX_ALLOC(c.w, uint64_t, at_least_1(words)); return RFX_OK; }
inline int ctg_alloc(rfx_ctx *ctx, CtgDev &c, int64_t n, int64_t words) { RFX_TRY(ctg_alloc_words(ctx, c, words)); return ctg_alloc_rows(ctx, c, n); }
inline int ee_set_alloc(rfx_ctx *ctx, EeSetDev &s, int64_t n, int64_t words) {
    const size_t m = at_least_1(n);
    s.n = n; s.words = words;
    RFX_ALLOC(s.w, uint64_t, at_least_1(words)); RFX_ALLOC(s.woff, int64_t, m + 1); RFX_ALLOC(s.len, int64_t, m); RFX_ALLOC(s.i32, int32_t, 7 * m);
    return RFX_OK;
}
inline int ee_cons_alloc(rfx_ctx *ctx, EeConsDev &c, int64_t n, int64_t lwords, int64_t rwords) {
    const size_t m = at_least_1(n);
    c.n = n; c.lwords = lwords; c.rwords = rwords;
    RFX_ALLOC(c.lw, uint64_t, at_least_1(lwords)); RFX_ALLOC(c.lwoff, int64_t, m + 1); RFX_ALLOC(c.llen, int64_t, m);
    RFX_ALLOC(c.rw, uint64_t, at_least_1(rwords)); RFX_ALLOC(c.rwoff, int64_t, m + 1); RFX_ALLOC(c.rlen, int64_t, m);
    RFX_ALLOC(c.flags, int32_t, m);
    return RFX_OK;
}
inline int mp_hits_alloc(rfx_ctx *ctx, MpHitsDev &h, int64_t n) { h.n = n; RFX_ALLOC(h.i32, int32_t, 5 * at_least_1(n)); return RFX_OK; }
// What the kernels take, by name, from a set of the library's or from the caller's public struct (whose arrays the entry point has
// checked): the ONLY places that write one of these six structs as a list of pointers, or carve an int32 block (tests/
// test_source_idioms.py).  An *_out of a const owner is what dyn_out is: the owner stays, what it points at is written.
inline Fx2View fx2_view(const CtgDev &c) { return Fx2View{c.n, c.w.as<uint64_t>(), c.woff.as<int64_t>(), c.len.as<int64_t>(), c.left.as<int32_t>(), c.right.as<int32_t>()}; }
inline Fx2View fx2_view(const rfx_contigs_packed *p, const int32_t *d_left, const int32_t *d_right) { return Fx2View{p->n, p->words, p->word_off, p->len, d_left, d_right}; }
inline EeSetOut ee_set_out(const EeSetDev &s) {
    const size_t m = at_least_1(s.n);
    int32_t *a = s.i32.as<int32_t>();
    return EeSetOut{s.w.as<uint64_t>(), s.woff.as<int64_t>(), s.len.as<int64_t>(), a, a + m, a + 2 * m, a + 3 * m, a + 4 * m, a + 5 * m, a + 6 * m};
}
inline EeSetOut ee_set_out(const rfx_endext_set *s) {
    return EeSetOut{s->set.words, s->set.word_off, s->set.len, s->left, s->right, s->left_len, s->right_len, s->flags, s->src_idx, s->new_idx};
}
inline EeSetIn ee_set_in(int64_t n, const EeSetOut &o) { return EeSetIn{n, o.w, o.woff, o.len, o.left, o.right, o.left_len, o.right_len, o.flags, o.src_idx, o.new_idx}; }
inline EeSetIn ee_set_in(const EeSetDev &s) { return ee_set_in(s.n, ee_set_out(s)); }
inline EeSetIn ee_set_in(const rfx_endext_set *s) { return ee_set_in(s->set.n, ee_set_out(s)); }
inline EeConsOut ee_cons_out(const EeConsDev &c) {
    return EeConsOut{c.lw.as<uint64_t>(), c.lwoff.as<int64_t>(), c.llen.as<int64_t>(), c.rw.as<uint64_t>(), c.rwoff.as<int64_t>(), c.rlen.as<int64_t>(), c.flags.as<int32_t>()};
}
inline EeConsOut ee_cons_out(const rfx_endext_consensus *c) { return EeConsOut{c->left.words, c->left.word_off, c->left.len, c->right.words, c->right.word_off, c->right.len, c->flags}; }
inline EeConsIn ee_cons_in(const EeConsOut &o) { return EeConsIn{o.lw, o.lwoff, o.llen, o.rw, o.rwoff, o.rlen, o.flags}; }
inline EeConsIn ee_cons_in(const EeConsDev &c) { return ee_cons_in(ee_cons_out(c)); }
inline EeConsIn ee_cons_in(const rfx_endext_consensus *c) { return ee_cons_in(ee_cons_out(c)); }
inline MpHits mp_hits(const MpHitsDev &h) {
    const size_t m = at_least_1(h.n);
    int32_t *a = h.i32.as<int32_t>();
    return MpHits{a, a + m, a + 2 * m, a + 3 * m, a + 4 * m};
}
inline MpHits mp_hits(const rfx_map_hits *h) { return MpHits{h->read, h->end, h->strand, h->offset, h->v}; }
// host checks of the entry points on these sets, beside text_rows_ok / dyn_packed_out_ok above: a caller's text output (a capacity of 0
// takes no buffer) / the gate between plan and fill: what the plan found goes into need_n / need_words, and the answer is whether the
// caller's output holds it -- where it does not, the entry point returns RFX_E_CAP with n untouched and no array written
inline bool text_out_ok(const char *out, int64_t cap, const int64_t *out_len) { return out_len && cap >= 0 && (cap == 0 || out); }
inline bool packed_out_fits(rfx_contigs_packed *o, int64_t n, int64_t words) { o->need_n = n; o->need_words = words; return n <= o->cap_n && words <= o->cap_words; }
inline bool packed_out_fits(rfx_map_hits *o, int64_t n) { o->need_n = n; return n <= o->cap_n; }
// shared by the entry points of rfx_fixing2.hip, rfx_endext.hip, rfx_ctgext.hip and rfx_endmap.hip (defined in rfx_fixing2.hip): a
// caller's contig set has its arrays / as an input: n >= 0 too, and left / right where n > 0 / max_k 31..124, max_iteration >= -1 and
// parts_ok(P), last_error in the name of `stage` / the body of the rfx_dev_*_to_text entry points on a contig set (ends as fx2_text) /
// the front of the host forms of 05FixingAgain and 09ExtendAgain: one upload, binarize, run, the contigs in the library's buffers
bool fx2_contigs_ok(const rfx_contigs_packed *p);
bool fx2_contigs_in_ok(const rfx_contigs_packed *p, const int32_t *d_left, const int32_t *d_right);
int fx2_params(rfx_ctx *ctx, const rfx_fix_params *p, int P, const char *stage = "contig fixing, round two");
int fx2_text_call(rfx_ctx *ctx, int ends, const rfx_contigs_packed *d_in, const int32_t *d_left, const int32_t *d_right, char *d_text, int64_t cap,
                  int64_t *out_len);
int fx2_contigs_of_text(rfx_ctx *ctx, const char *text, const int64_t *row_off, int64_t n_rows, int P, const rfx_fix_params *params, CtgDev &c);
// ... and of rfx_endext.hip with rfx_ctgext.hip: a caller's set of 07EndExtend has its arrays
bool ee_set_ok(const rfx_endext_set *s);
#pragma GCC visibility pop

}  // namespace rfx
