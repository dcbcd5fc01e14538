// eh_row and eh_add (reflexiv_amd/csrc/rfx_endext_hits.h), the arithmetic that replaces the row text between the end mapping and the end
// extension, as a host program.  Built by tests/test_endext_hits_host.py with the host compiler and -fsanitize=address,undefined.  It
// enumerates every hit the mapper can write at seed 21 -- reads of 22..340 bases, both sides, every offset, on a whole-contig target of
// 60 and of 399 bases and on the 200-base targets of a contig of 400 bases; v follows from the offset, and over the offsets it takes both
// of its limits (what is left of the read, the target's length) -- and writes one record of 16 ints per hit to the file named on the
// command line: side, L, n, off, v, then the row (suf, start, c0, c1, c2), then what it adds (lsrc, lcnt, rsrc, rcnt, bad) and a 0.  The
// Python test walks the same enumeration through tests/map_model.py and tests/endext_model.py.  Here: an (off, v) the mapper cannot have
// written is refused -- v one off in either direction, the offsets next to both limits -- and nothing eh_add returns points outside
// the read.  Exit status 0: nothing found.
#define __host__
#define __device__
#include "rfx_endext_hits.h"

#include <cstdint>
#include <cstdio>
#include <vector>

static const int SEED = 21;
static const int TARGETS[] = {60, 399, 400};

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: endext_hits OUT\n"); return 2; }
    int failures = 0;
    std::vector<int32_t> out;
    for (int L : TARGETS) {
        for (int n = SEED + 1; n <= 340; n++) {
            for (int side = 0; side < 2; side++) {
                const int lo = side ? 0 : 1, hi = side ? n - 1 - SEED : n - SEED;
                const int tlen = L < 2 * EH_END ? L : EH_END;
                EhRow r{};
                for (int off = lo - 2; off <= hi + 2; off++) {
                    const int span = side ? off + SEED : n - off, v = span < tlen ? span : tlen;
                    const bool valid = off >= lo && off <= hi;
                    if (eh_row(side, L, n, off, v, SEED, &r) != valid) { fprintf(stderr, "eh_row(side %d, L %d, n %d, off %d, v %d)\n", side, L, n, off, v); failures++; }
                    if (!valid) continue;
                    if (eh_row(side, L, n, off, v - 1, SEED, &r) || eh_row(side, L, n, off, v + 1, SEED, &r)) {
                        fprintf(stderr, "eh_row takes a v one off (side %d, L %d, n %d, off %d)\n", side, L, n, off);
                        failures++;
                    }
                    if (!eh_row(side, L, n, off, v, SEED, &r)) continue;
                    const EhAdd a = eh_add(r, n, L);
                    if (a.bad || a.lcnt < 0 || a.lcnt > EH_LONGEST || a.rcnt < 0 || a.rcnt > EH_LONGEST || (a.lcnt && (a.lsrc >= n || a.lsrc - (a.lcnt - 1) < 0)) ||
                        (a.rcnt && (a.rsrc < 0 || a.rsrc + a.rcnt > n))) {
                        fprintf(stderr, "eh_add outside the read (side %d, L %d, n %d, off %d)\n", side, L, n, off);
                        failures++;
                    }
                    const int32_t rec[16] = {side, L, n, off, v, r.suf, r.start, r.c0, r.c1, r.c2, a.lsrc, a.lcnt, a.rsrc, a.rcnt, a.bad, 0};
                    out.insert(out.end(), rec, rec + 16);
                }
            }
        }
    }
    // an operation of ten digits is what the row parser refuses
    {
        const EhRow big{0, 1, 1000000000, 40, 0};
        if (eh_add(big, 2000000000, 300).bad != 1) { fprintf(stderr, "a ten-digit operation\n"); failures++; }
    }
    FILE *f = fopen(argv[1], "wb");
    if (!f || fwrite(out.data(), sizeof(int32_t), out.size(), f) != out.size() || fclose(f)) { fprintf(stderr, "cannot write %s\n", argv[1]); return 2; }
    if (failures) { fprintf(stderr, "%d differences\n", failures); return 1; }
    printf("ok %zu\n", out.size() / 16);
    return 0;
}
