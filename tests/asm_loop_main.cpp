// Drives reflexiv_amd/csrc/rfx_asm_loop.h through the enumeration of tests/test_asm_loop_host.py and writes, after every step,
// the decision and the whole state to the file named on the command line.  The enumeration (which configurations, which
// starting states, which counts) is stated there; the two programs walk it in the same order.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "rfx_asm_loop.h"

using rfx::AsmLoop;
using rfx::AsmRule;

static FILE *out;
static const int64_t FILL = 1000000;          // counts of the positions that are not enumerated: strictly decreasing

static void record(int decision, const AsmLoop &s) {
    fprintf(out, "%d %d %lld %d %d %d %d %lld\n", decision, s.iterations, (long long)s.contig_number, s.scramble, s.P,
            s.partition_number, s.passes_done, (long long)s.nt);
}

// every continuation from `s`, `pos` head calls into the loop; `room`: the calls that max_iter leaves when the loop begins
static void walk(const AsmLoop &s, const AsmRule &r, const int64_t *alphabet, int pos, int room, int head_free, int tail_free) {
    const bool is_free = pos < room && (pos < head_free || pos >= room - tail_free);
    for (int c = 0; c < (is_free ? 3 : 1); c++) {
        AsmLoop t = s;
        const int d = rfx::asm_loop_head(t, r, is_free ? alphabet[c] : FILL - pos);
        if (d) { t.passes_done++; t.nt++; }               // (the driver counts the pass it ran)
        record(d, t);
        if (d && pos <= r.max_iter + 2) walk(t, r, alphabet, pos + 1, room, head_free, tail_free);
    }
}

int main(int argc, char **argv) {
    if (argc != 2 || !(out = fopen(argv[1], "w"))) return 2;
    const int min_iters[5] = {0, 1, 3, 4, 15}, max_iters[4] = {0, 2, 5, 20}, pns[5] = {1, 15, 16, 17, 64};
    for (int wide = 0; wide < 2; wide++)
        for (int coalesce = 0; coalesce < 2; coalesce++)
            for (int mi = 0; mi < 5; mi++)
                for (int ma = 0; ma < 4; ma++)
                    for (int pi = 0; pi < 5; pi++) {
                        const int pn = pns[pi], max_iter = max_iters[ma];
                        if (max_iter == 20 && !(coalesce && !wide) && pn != 64) continue;
                        const AsmRule r{wide, coalesce, min_iters[mi], max_iter};
                        const int64_t alphabet[3] = {21 * (int64_t)pn - 1, 21 * (int64_t)pn, 0};
                        for (int start = -1; start <= 5; start++) {           // -1: fresh; 0..5: resumed with that many passes done
                            fprintf(out, "C %d %d %d %d %d %d\n", wide, coalesce, r.min_iter, max_iter, pn, start);
                            AsmLoop s;
                            s.P = s.partition_number = pn;
                            if (start >= 0) {
                                s.scramble = 3;
                                s.passes_done = start;
                                s.nt = start;
                                s.iterations = start < 5 ? (start > 0 ? start - 1 : 0) : (max_iter - 6 > 4 ? max_iter - 6 : 4);
                                s.contig_number = alphabet[start % 3];
                            }
                            for (int stage; (stage = rfx::asm_loop_before(s)) >= 0;) { s.passes_done++; s.nt++; record(stage, s); }
                            const int room = max_iter + 1 - s.iterations > 0 ? max_iter + 1 - s.iterations : 0;
                            walk(s, r, alphabet, 0, room, room <= 7 ? room : 3, room <= 7 ? 0 : 4);
                        }
                    }
    if (fclose(out) != 0) return 3;
    printf("ok\n");
    return 0;
}
