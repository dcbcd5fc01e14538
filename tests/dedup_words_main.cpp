// The word helpers of the contig de-duplication (reflexiv_amd/csrc/rfx_dedup_words.h) against a byte model, as a host program:
// random contigs of every length 0..130 and a few of about 10^5 bases, every start from 0 to len + 16, both strands.  Built by
// tests/test_dedup_words_host.py with the host compiler and -fsanitize=address,undefined (the packed arrays are exactly as long
// as the layout says, so a word load past a contig's last word is reported).  Exit status 0: no difference.
#define __host__
#define __device__
#include "rfx_dedup_words.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

typedef std::vector<uint8_t> Bases;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                                           // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int failures = 0;
static void differ(const char *what, int64_t len, int64_t t, int rc, uint64_t got, uint64_t want) {
    if (failures++ < 20)
        fprintf(stderr, "%s: len %lld start %lld strand %d: got %016llx want %016llx\n", what, (long long)len, (long long)t, rc,
                (unsigned long long)got, (unsigned long long)want);
}

// the layout: 32 bases per word, the first in the two highest bits, 0 behind the last base; exactly (len + 31) / 32 words
static std::vector<uint64_t> pack(const Bases &b) {
    std::vector<uint64_t> w((b.size() + 31) / 32, 0ull);
    for (size_t i = 0; i < b.size(); i++) w[i / 32] |= (uint64_t)b[i] << (62 - 2 * (i % 32));
    return w;
}
static Bases strand(const Bases &b, int rc) {
    if (!rc) return b;
    Bases r(b.size());
    for (size_t i = 0; i < b.size(); i++) r[i] = (uint8_t)(3 - b[b.size() - 1 - i]);
    return r;
}
// the byte model of a window: base t + j of s in group j, 0 where s has none
static uint64_t window(const Bases &s, int64_t t) {
    uint64_t x = 0;
    for (int j = 0; j < 32; j++) {
        const int64_t q = t + j;
        x = (x << 2) | (q >= 0 && q < (int64_t)s.size() ? s[(size_t)q] : 0);
    }
    return x;
}
// the seed as the byte kernels read it: position n is C, everything behind it A
static uint32_t seed_model(const Bases &s, int64_t p) {
    const int64_t n = (int64_t)s.size();
    uint32_t x = 0;
    for (int j = 0; j < 15; j++) {
        const int64_t q = p + j;
        x = (x << 2) | (q < n ? s[(size_t)q] : q == n ? 1u : 0u);
    }
    return x;
}

static void check_contig(const Bases &b, bool cats) {
    const int64_t len = (int64_t)b.size();
    const std::vector<uint64_t> w = pack(b);
    const uint64_t *wp = w.empty() ? nullptr : w.data();
    for (int rc = 0; rc < 2; rc++) {
        const Bases s = strand(b, rc);
        for (int64_t t = 0; t <= len + 16; t++) {
            const uint64_t want = window(s, t);
            const uint64_t got = rc ? dd_seg32_rc(wp, len, t) : dd_seg32(wp, len, t);
            if (got != want) differ("seg32", len, t, rc, got, want);
            if (dd_strand32(wp, len, rc, t) != want) differ("strand32", len, t, rc, dd_strand32(wp, len, rc, t), want);
            const uint32_t sg = dd_seed15(wp, len, t, rc), sw = seed_model(s, t);
            if (sg != sw) differ("seed15", len, t, rc, sg, sw);
            if (t + 31 <= len) {
                const uint64_t m = (window(s, t) & ~3ull) | 1ull;
                if (!rc) {
                    if (dd_mer31(wp, len, t) != m) differ("mer31", len, t, 0, dd_mer31(wp, len, t), m);
                } else {
                    // the 31-mer at t of the reverse complement = the reverse complement of the forward 31-mer at len - 31 - t
                    const uint64_t g = dd_mer31_rc(dd_mer31(wp, len, len - 31 - t));
                    if (g != m) differ("mer31_rc", len, t, 1, g, m);
                }
            }
        }
        // the seed's past-end rule at p = n - 14 .. n, once more by name
        for (int64_t p = len - 14 > 0 ? len - 14 : 0; p <= len; p++)
            if (dd_seed15(wp, len, p, rc) != seed_model(s, p)) differ("seed15 past the end", len, p, rc, dd_seed15(wp, len, p, rc), seed_model(s, p));
    }
    for (int64_t t = -31; t < 0; t++)                             // a contig that begins inside the window (the second piece of a merge)
        if (dd_seg32(wp, len, t) != window(b, t)) differ("seg32 (negative start)", len, t, 0, dd_seg32(wp, len, t), window(b, t));
    if (!cats) return;
    // concatenations: a piece of this contig and a piece of a second one, each of either strand, in both orders
    Bases c((size_t)(rnd() % 131));
    for (auto &x : c) x = (uint8_t)(rnd() & 3);
    const std::vector<uint64_t> cw = pack(c);
    const int64_t clen = (int64_t)c.size();
    for (int combo = 0; combo < 8; combo++) {
        const int rca = combo & 1, rcb = (combo >> 1) & 1, order = combo >> 2;
        DdSeg a{wp, len, 0, 0, rca, 0}, d{cw.empty() ? nullptr : cw.data(), clen, 0, 0, rcb, 0};
        a.from = len ? (int64_t)(rnd() % (uint64_t)(len + 1)) : 0;
        a.n = (int64_t)(rnd() % (uint64_t)(len - a.from + 1));
        if (combo % 3 == 0) { a.from = 0; a.n = len; }            // (the whole contig: what a merge's long side and a copy are)
        d.from = clen ? (int64_t)(rnd() % (uint64_t)(clen + 1)) : 0;
        d.n = (int64_t)(rnd() % (uint64_t)(clen - d.from + 1));
        const Bases sa = strand(b, rca), sd = strand(c, rcb);
        Bases cat;
        const DdSeg &first = order ? d : a, &second = order ? a : d;
        const Bases &sf = order ? sd : sa, &ss = order ? sa : sd;
        cat.insert(cat.end(), sf.begin() + first.from, sf.begin() + first.from + first.n);
        cat.insert(cat.end(), ss.begin() + second.from, ss.begin() + second.from + second.n);
        for (int64_t t = 0; t <= (int64_t)cat.size() + 16; t++) {
            const uint64_t got = dd_cat32(first, second, t), want = window(cat, t);
            if (got != want) differ("cat32", (int64_t)cat.size(), t, combo, got, want);
        }
    }
}

int main() {
    for (int rep = 0; rep < 3; rep++)
        for (int64_t len = 0; len <= 130; len++) {
            Bases b((size_t)len);
            for (auto &x : b) x = (uint8_t)(rnd() & 3);
            check_contig(b, true);
        }
    // all T (the complement is all A: the zeros of the padding and the zeros of a base must not be confused) and all A
    for (int64_t len = 0; len <= 130; len++) { check_contig(Bases((size_t)len, 3), true); check_contig(Bases((size_t)len, 0), true); }
    const int64_t big[] = {99999, 100000, 100001, 100032};
    for (int64_t len : big) {
        Bases b((size_t)len);
        for (auto &x : b) x = (uint8_t)(rnd() & 3);
        check_contig(b, true);
    }
    if (failures) { fprintf(stderr, "%d differences\n", failures); return 1; }
    printf("dedup word helpers: ok\n");
    return 0;
}
