// rfx_asm_loop.h -- the variables of the fixed-k extend driver's loop and the rule at its head, once: P/ReflexivMain.java:265-296
// (k <= 31) and P/ReflexivDSMain64.java:582, 621-661 (k > 31).  Plain C++, no HIP types: the one-GPU driver (rfx_api.hip), the
// sharded driver (rfx_shard.hip), thread 0 of k_small_pass (rfx_extend.hip) and a host program (tests/asm_loop_main.cpp) share it.
#ifndef RFX_ASM_LOOP_H
#define RFX_ASM_LOOP_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RFX_ASM_FN __host__ __device__ inline
#else
#define RFX_ASM_FN inline
#endif

namespace rfx {

// what the loop carries from pass to pass, on the host and (inside k_small_pass's state) in HBM
struct AsmLoop {
    int64_t contig_number = 0;   // the record count at the last check (:264 / 64 :580)
    int64_t nt = 0;              // trace entries written
    int iterations = 0;
    int scramble = 2;            // U/DefaultParam.java:131; 3 after the first repeat of the count at k > 31
    int partition_number = 1;    // what the coalesce rule divides (:263); P follows it at k <= 31
    int passes_done = 0;         // extend passes behind the record set (the first five come before the loop)
    int P = 1;                   // logical partitions of the next pass
};
// what the caller fixes for the whole loop
struct AsmRule { int wide, coalesce, min_iter, max_iter; };

// The five passes before the loop: :221-222 (stage 0), :233-241 (three more, iterations 1..3), :247-254 (first-array, stage 1).
// -> the stage of pass number s.passes_done, or -1 once the five are behind; the caller counts the pass it ran.
RFX_ASM_FN int asm_loop_before(AsmLoop &s) {
    if (s.passes_done >= 5) return -1;
    if (s.passes_done >= 1) s.iterations++;
    return s.passes_done < 4 ? 0 : 1;
}

// `while (iterations <= maximumIteration)` (:265 / 64 :582) alone, for what a caller decides before the head
RFX_ASM_FN bool asm_loop_open(const AsmLoop &s, const AsmRule &r) { return s.iterations <= r.max_iter; }

// The head of the loop with `current` records in the set: 0 = stop, else run a pass whose marker starts at the value returned
// (2; 1 at k > 31 once scramble is 3, 64 :7484-7486).  A stop by the count leaves `iterations` incremented, a stop by
// max_iter does not.  k > 31: the count is checked from min_iter + 3 on, its first repeat flips scramble 2 -> 3 and still
// runs the pass, only the second stops.
RFX_ASM_FN int asm_loop_head(AsmLoop &s, const AsmRule &r, int64_t current) {
    if (!asm_loop_open(s, r)) return 0;
    s.iterations++;
    if (s.iterations >= (r.wide ? r.min_iter + 3 : r.min_iter) && s.iterations % 3 == 0) {     // :267-268 / 64 :621-622
        if (s.contig_number == current) {                                                     // count() :270-271 / 64 :633-639
            if (!r.wide || s.scramble != 2) return 0;                                         // :272 / 64 :644
            s.scramble = 3;                                                                   // 64 :640-642
        } else {
            s.contig_number = current;                                                        // :274 / 64 :647
            // the coalesce of 64 :651-655 is assigned to a variable the loop does not read: no effect at k > 31
            if (!r.wide && r.coalesce && s.partition_number >= 16 && current / s.partition_number <= 20) {
                s.partition_number = s.partition_number / 4 + 1;                              // :277-281
                s.P = s.partition_number;
            }
        }
    }
    return r.wide && s.scramble == 3 ? 1 : 2;                                                 // 64 :659-660, :667-669
}

}  // namespace rfx

#endif
