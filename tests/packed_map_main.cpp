// pk_mismatch32 and pk_rc_seg32 (reflexiv_amd/csrc/rfx_packed_words.h), the two word helpers of the end mapping (rfx_endmap.hip), as a
// host program: values written out by hand, then random segments against a naive loop over bases.  Built by
// tests/test_packed_map_host.py with the host compiler and -fsanitize=address,undefined: every segment lives in a heap buffer of exactly
// ceil(len / 32) words WITH JUNK behind its last base (a read of the read store has no zero padding), so a word read past the segment
// is reported and a junk bit that reaches a result is a difference.  Exit status 0: no difference.
#define __host__
#define __device__
#include "rfx_packed_words.h"

#include <cstdint>
#include <cstdio>
#include <vector>

static uint64_t z = 88172645463325252ull;
static uint64_t rnd() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; }

static uint64_t word_of(const char *s) {                           // up to 32 letters, the first in the two highest bits
    uint64_t x = 0;
    for (int j = 0; s[j]; j++) x |= pk_at(pk_code(s[j]), j);
    return x;
}

int main() {
    int failures = 0;
    // ---- by hand
    const struct { const char *a, *b; int m, want; } FIXED[] = {
        {"ACGT", "ACGT", 4, 0}, {"ACGT", "ACGA", 4, 1}, {"ACGT", "ACGA", 3, 0}, {"ACGT", "TGCA", 4, 4}, {"ACGT", "TGCA", 0, 0},
        {"AAAA", "CCCC", 4, 4},                                    // codes 0 and 1 differ in the low bit only
        {"AAAA", "GGGG", 2, 2},                                    // 0 and 2: the high bit only
        {"CCCC", "GGGG", 4, 4},                                    // 1 and 2: both bits, one position each
        {"ACGTACGTACGTACGTACGTACGTACGTACGT", "ACGTACGTACGTACGTACGTACGTACGTACGA", 32, 1},
        {"ACGTACGTACGTACGTACGTACGTACGTACGT", "ACGTACGTACGTACGTACGTACGTACGTACGA", 31, 0},
        {"ACGTACGTACGTACGTACGTACGTACGTACGT", "TCGTACGTACGTACGTACGTACGTACGTACGT", 40, 1},
    };
    for (const auto &f : FIXED) {
        const int got = pk_mismatch32(word_of(f.a), word_of(f.b), f.m);
        if (got != f.want) { fprintf(stderr, "pk_mismatch32(%s, %s, %d) = %d, want %d\n", f.a, f.b, f.m, got, f.want); failures++; }
    }
    {                                                              // the reverse complement of ACGGT is ACCGT; of AAC, GTT
        const uint64_t a[1] = {word_of("ACGGT") | 0xFFFFull}, b[1] = {word_of("AAC") | 0xFFFFFFFFull};
        if (pk_rc_seg32(a, 5, 0) != word_of("ACCGT")) { fprintf(stderr, "rc(ACGGT)\n"); failures++; }
        if (pk_rc_seg32(a, 5, 2) != word_of("CGT")) { fprintf(stderr, "rc(ACGGT) from 2\n"); failures++; }
        if (pk_rc_seg32(b, 3, 0) != word_of("GTT")) { fprintf(stderr, "rc(AAC)\n"); failures++; }
        if (pk_rc_seg32(b, 3, 2) != word_of("T")) { fprintf(stderr, "rc(AAC) from 2\n"); failures++; }
    }
    // ---- random segments of 1..200 bases with junk behind them, every window start
    for (int it = 0; it < 600 && failures < 20; it++) {
        const int len = 1 + (int)(rnd() % 200), nw = (len + 31) >> 5;
        std::vector<uint8_t> base((size_t)len);
        uint64_t *w = new uint64_t[(size_t)nw];                    // exactly nw words: one more read is a heap overflow
        for (int k = 0; k < nw; k++) w[k] = rnd();                 // junk everywhere ...
        for (int t = 0; t < len; t++) {                            // ... then the bases
            base[(size_t)t] = (uint8_t)(rnd() & 3);
            w[t >> 5] = (w[t >> 5] & ~pk_at(3, t)) | pk_at(base[(size_t)t], t);
        }
        for (int t = 0; t < len; t++) {
            uint64_t want = 0;
            for (int j = 0; j < 32 && t + j < len; j++) want |= pk_at(3u - base[(size_t)(len - 1 - (t + j))], j);
            const uint64_t got = pk_rc_seg32(w, len, t);
            if (got != want) { fprintf(stderr, "pk_rc_seg32(len %d, t %d) = %016llx, want %016llx\n", len, t, (unsigned long long)got, (unsigned long long)want); failures++; break; }
        }
        // the mismatch count of two windows of the same segment against the loop, at every length 0..32 and beyond
        const int t0 = (int)(rnd() % (unsigned)len), t1 = (int)(rnd() % (unsigned)len);
        for (int m = 0; m <= 34; m++) {
            int want = 0;
            for (int j = 0; j < m && j < 32; j++) {
                const int a = t0 + j < len ? 3 - base[(size_t)(len - 1 - (t0 + j))] : 0, b = t1 + j < len ? 3 - base[(size_t)(len - 1 - (t1 + j))] : 0;
                want += a != b;
            }
            const int got = pk_mismatch32(pk_rc_seg32(w, len, t0), pk_rc_seg32(w, len, t1), m);
            if (got != want) { fprintf(stderr, "pk_mismatch32(len %d, %d, %d, m %d) = %d, want %d\n", len, t0, t1, m, got, want); failures++; break; }
        }
        delete[] w;
    }
    if (failures) { fprintf(stderr, "%d differences\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
