// rfx_endext_hits.h -- what a hit of the end mapping (rfx_dev_map_ends: read, end, strand, offset, v) adds to the two pile-ups of the end
// extension, without the row text between the two stages (rfx_dev_endext_consensus_hits).  Plain integer arithmetic,
// `__host__ __device__` and force-inlined on the device, so a host program can compile it with the two words defined away
// (tests/endext_hits_main.cpp enumerates it against the two string models, as rfx_reduce_fsm.h and rfx_packed_words.h are held).
//
// It restates two things and nothing else.  eh_row: the row rfx_dev_map_to_text prints for a hit (mp_row, rfx_endmap.hip) -- the name's
// suffix, the start and the three parts of the CIGAR, "<o>S<v>M[<p>S]" with start 1 at a left end and "[<p>S]<v>M<o>S" with start
// len - v + 1 at a right end -- with the same test of (offset, v) against the read's and the contig's length.  eh_add: what k_ee_parse
// (rfx_endext.hip; P/ReflexivDSDynamicKmerMapping.java :683-772) computes from that row: the walk over the CIGAR's operations (an
// operation is added when the next one is read, so the last never is; the sum starts at the first M that has been added, else at
// the first operation), the left contribution from first clip - start (so a left overhang of ONE base adds nothing), the right one from
// the last clip minus what the target still has behind the alignment, each side only where the name's suffix feeds it (-L: left only,
// -R: right only with a reference length of 200, none: both with the contig's length) and each capped at 300 bases.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define EH_INLINE __forceinline__
#else
#define EH_INLINE inline
#endif

#define EH_END 200                   /* bases of a contig end: MP_END (rfx_endmap.hip), EE_END (rfx_endext.hip)             */
#define EH_LONGEST 300               /* positions of a consensus: EE_LONGEST                                                */
#define EH_NEAR 10                   /* a start / a tail of 10 or more skips the row: EE_NEAR                               */

// the row of a hit: suf 0 = the whole contig is the target, 1 = "-L", 2 = "-R"; c0 S, c1 M, c2 S -- a part of 0 is not printed
struct EhRow { int suf, start, c0, c1, c2; };
// what the row adds, as positions of seq (the read in the orientation that matched, n bases): lcnt bases read DOWN from seq[lsrc] to the
// left table from j = 0, rcnt bases read UP from seq[rsrc] to the right one; bad: 1 = a CIGAR the parser refuses (an operation of 10
// digits), 2 = an overhang outside seq -- neither can come from a hit eh_row accepts, and both are kept as the parser has them
struct EhAdd { int lsrc, lcnt, rsrc, rcnt, bad; };

// side = end & 1, L = the contig's length (>= seed), n = the read's length.  false: rfx_dev_map_ends cannot have written (off, v)
__host__ __device__ EH_INLINE bool eh_row(int side, int L, int n, int off, int v, int seed, EhRow *r) {
    const int tlen = L < 2 * EH_END ? L : EH_END;
    int over, past;                                                 // the clips at this end and at the far end
    if (side == 0) {
        if (off < 1 || off > n - seed || v != (n - off < tlen ? n - off : tlen)) return false;
        over = off; past = n - off - v;
    } else {
        if (off < 0 || off > n - 1 - seed || v != (off + seed < tlen ? off + seed : tlen)) return false;
        over = n - off - seed; past = off + seed - v;
    }
    r->suf = L < 2 * EH_END ? 0 : 1 + side;
    r->start = side ? tlen - v + 1 : 1;
    r->c0 = side ? past : over; r->c1 = v; r->c2 = side ? over : past;
    return true;
}

__host__ __device__ EH_INLINE EhAdd eh_add(const EhRow &r, int n, int L) {
    EhAdd a{0, 0, 0, 0, 0};
    int64_t first_len = 0, pend_len = 0, sum_all = 0, sum_m = 0;
    char first_op = 0, pend_op = 0;
    bool seen_m = false;
    int nops = 0;
    for (int k = 0; k < 3; k++) {
        const int64_t v = k == 0 ? r.c0 : k == 1 ? r.c1 : r.c2;
        if (!v) continue;
        if (v >= 1000000000) { a.bad = 1; return a; }
        const char op = k == 1 ? 'M' : 'S';
        if (nops > 0) {
            if (pend_op == 'M') seen_m = true;
            sum_all += pend_len;                                    // (no I among the mapper's operations)
            if (seen_m) sum_m += pend_len;
        } else {
            first_len = v; first_op = op;
        }
        pend_len = v; pend_op = op; nops++;
    }
    const int64_t align = seen_m ? sum_m : sum_all;
    if (r.suf != 2 && first_op == 'S' && r.start < EH_NEAR) {
        const int64_t o = first_len - r.start;
        if (o > 0) {
            if (o >= n) a.bad = 2;
            else { a.lsrc = (int)o; a.lcnt = (int)(o + 1 < EH_LONGEST ? o + 1 : EH_LONGEST); }
        }
    }
    if (r.suf != 1 && pend_op == 'S') {
        const int64_t ref = r.suf == 2 ? EH_END : L, tail = ref - (align + r.start - 1);
        if (tail < EH_NEAR) {
            const int64_t o = pend_len - tail;
            if (o > 0) {
                if (o > n) a.bad = 2;
                else { a.rsrc = (int)(n - o); a.rcnt = (int)(o < EH_LONGEST ? o : EH_LONGEST); }
            }
        }
    }
    if (a.bad) { a.lcnt = 0; a.rcnt = 0; }
    return a;
}
