// The word helpers of the packed seams between the counter, the k-mer sorting stage, the reduction and the dynamic-k passes
// (reflexiv_amd/csrc/rfx_packed_words.h: pk_revcomp, pk_from_counter, pk_count_as_text, pk_int_as_text) against a plain restatement,
// base by base and digit by digit, as a host program.  Built by tests/test_packed_seams_host.py with the host compiler and
// -fsanitize=address,undefined: a counter key is exactly the words its format has, so a load past the last one is reported.
// Exit status 0: no difference.
#define __host__
#define __device__
#include "rfx_packed_words.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bases;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {                                           // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static int failures = 0;
static void differ(const char *what, long long a, long long b, unsigned long long got, unsigned long long want) {
    if (failures++ < 20) fprintf(stderr, "%s: (%lld, %lld): got %016llx want %016llx\n", what, a, b, got, want);
}
// 0: random, 1: all A, 2: all T, 3: its own reverse complement (even lengths; the middle base of an odd one cannot be)
static Bases bases_of(int n, int kind) {
    Bases b((size_t)n);
    for (auto &x : b) x = kind == 1 ? 0 : kind == 2 ? 3 : (uint8_t)(rnd() & 3);
    if (kind == 3) for (int i = 0; i < n / 2; i++) b[(size_t)(n - 1 - i)] = (uint8_t)(3 - b[(size_t)i]);
    return b;
}
// the key layout: 128 base slots in four words, the first base in the two highest bits, 0 behind the last base
static Pk4 pk4_of(const Bases &b) {
    uint64_t w[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < b.size(); i++) w[i / 32] |= (uint64_t)b[i] << (62 - 2 * (i % 32));
    return Pk4{w[0], w[1], w[2], w[3]};
}
static bool same(const Pk4 &a, const Pk4 &b) { return a.w0 == b.w0 && a.w1 == b.w1 && a.w2 == b.w2 && a.w3 == b.w3; }

// ---- pk_revcomp: base i of the result is 3 - base len - 1 - i ------------------------------------------------------------------------
static void check_revcomp() {
    for (int kind = 0; kind < 4; kind++)
        for (int len = 0; len <= 128; len++) {
            const Bases b = bases_of(len, kind);
            Bases rc((size_t)len);
            for (int i = 0; i < len; i++) rc[(size_t)i] = (uint8_t)(3 - b[(size_t)(len - 1 - i)]);
            const Pk4 got = pk_revcomp(pk4_of(b), len);
            if (!same(got, pk4_of(rc))) differ("pk_revcomp", kind, len, got.w0, pk4_of(rc).w0);
            if (kind == 3 && len % 2 == 0 && !same(got, pk4_of(b))) differ("pk_revcomp (palindrome)", kind, len, got.w0, pk4_of(b).w0);
            // what lies behind the first len bases of the input must not matter
            Pk4 dirty = pk4_of(b);
            const Pk4 junk{rnd(), rnd(), rnd(), rnd()}, kept = pk_keep4(junk, len);
            dirty.w0 |= junk.w0 ^ kept.w0; dirty.w1 |= junk.w1 ^ kept.w1; dirty.w2 |= junk.w2 ^ kept.w2; dirty.w3 |= junk.w3 ^ kept.w3;
            if (!same(pk_revcomp(dirty, len), pk4_of(rc))) differ("pk_revcomp (junk behind the bases)", kind, len, pk_revcomp(dirty, len).w0, pk4_of(rc).w0);
        }
}

// ---- pk_from_counter: the counter's words, written here base by base as DSBinaryKmerToString reads them ------------------------------
static void check_from_counter() {
    for (int kind = 0; kind < 4; kind++)
        for (int k = 1; k <= 127; k++) {
            const Bases b = bases_of(k, kind);
            const int full = k / 32, res = k % 32;
            std::vector<uint64_t> w((size_t)(full + (res ? 1 : 0)), 0ull);          // exactly the words that hold a base
            for (int i = 0; i < full * 32; i++) w[(size_t)(i / 32)] |= (uint64_t)b[(size_t)i] << (2 * (31 - i % 32));
            for (int i = full * 32; i < k; i++) w[(size_t)(i / 32)] |= (uint64_t)b[(size_t)i] << (2 * (res - 1 - i % 32));
            Pk4 got = pk_from_counter(w.data(), k);
            if (!same(got, pk4_of(b))) differ("pk_from_counter", kind, k, got.w0, pk4_of(b).w0);
            if (res) {                                                              // bits above the bases of the last word: dropped
                w[(size_t)full] |= rnd() << (2 * res);
                got = pk_from_counter(w.data(), k);
                if (!same(got, pk4_of(b))) differ("pk_from_counter (bits above the last word's bases)", kind, k, got.w0, pk4_of(b).w0);
            }
        }
}

// ---- the two "through the text" rules --------------------------------------------------------------------------------------------------
// DynamicKmerBinarizer as k_ks_bin_sizes states it: the digits of the count; ten or more of them are 1,000,000,000
static long long count_model(long long c) {
    char t[32];
    const int nd = snprintf(t, sizeof t, "%lld", c);
    return nd >= 10 ? 1000000000LL : atoll(t);
}
static void check_count(long long c) {
    if (pk_count_as_text(c) != count_model(c)) differ("pk_count_as_text", c, 0, (unsigned long long)pk_count_as_text(c), (unsigned long long)count_model(c));
}
// the text pk_int_char writes, read back by pk_parse_int -- and the same from snprintf and the rule spelled out (a sign, then the
// shortest run of leading digits that reaches 10^8, or all of them)
static void check_int(int v) {
    char t[16];
    const int n = pk_int_chars(v);
    for (int q = 0; q < n; q++) t[q] = pk_int_char(v, q);
    int64_t i = 0;
    const int back = pk_parse_int(t, i, n);
    if (pk_int_as_text(v) != back || i != n) differ("pk_int_as_text (print, parse)", v, i, (unsigned)pk_int_as_text(v), (unsigned)back);
    char s[16];
    snprintf(s, sizeof s, "%d", v);
    const char *d = s + (s[0] == '-');
    long long m = 0;
    for (size_t len = 1; len <= strlen(d); len++) {
        m = atoll(std::string(d, len).c_str());
        if (m >= 100000000LL) break;
    }
    const int want = (int)(s[0] == '-' ? -m : m);
    if (pk_int_as_text(v) != want) differ("pk_int_as_text (rule)", v, 0, (unsigned)pk_int_as_text(v), (unsigned)want);
    if (v > -1000000000 && v < 1000000000 && pk_int_as_text(v) != v) differ("pk_int_as_text (nine digits are themselves)", v, 0, (unsigned)pk_int_as_text(v), (unsigned)v);
}
static void check_text_rules() {
    const long long counts[] = {0, 1, 8, 9, 10, 30000, 30001, 10000000, 10000001, 999999999, 1000000000, 1000000001, 2147483647, 2147483648LL,
                                1LL << 40, LLONG_MAX};
    for (long long c : counts) check_count(c);
    for (int rep = 0; rep < 4000; rep++) { check_count((long long)(rnd() >> 1)); check_count((long long)(rnd() % 3000000000ull)); }
    const int ints[] = {0, 1, -1, 9, -9, 10, 29999, 30000, 30001, -29999, -30000, -30001, 99999999, 100000000, 999999999, -999999999,
                        1000000000, -1000000000, 1000000009, 2147483647, INT_MAX - 1, INT_MIN, INT_MIN + 1};
    for (int v : ints) check_int(v);
    for (int rep = 0; rep < 4000; rep++) { check_int((int)(uint32_t)rnd()); check_int((int)(rnd() % 60001) - 30000); }
}

int main() {
    check_revcomp();
    check_from_counter();
    check_text_rules();
    if (failures) { fprintf(stderr, "%d differences\n", failures); return 1; }
    printf("packed seam helpers: ok\n");
    return 0;
}
