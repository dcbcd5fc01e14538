// The word helpers of the stages on packed record sets (reflexiv_amd/csrc/rfx_packed_words.h) against a byte model, as a host
// program.  Built by tests/test_packed_words_host.py with the host compiler and -fsanitize=address,undefined: every packed array
// is exactly (len + 31) / 32 words long and every offset array exactly n entries, so a load past the last one is reported.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                                           // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static Bases random_bases(size_t n) {
    Bases b(n);
    for (auto &x : b) x = (uint8_t)(rnd() & 3);
    return b;
}

static int failures = 0;
static void differ(const char *what, long long a, long long b, unsigned long long got, unsigned long long want) {
    if (failures++ < 20) fprintf(stderr, "%s: (%lld, %lld): got %016llx want %016llx\n", what, a, b, got, want);
}

// the layout: 32 bases per word, the first in the two highest bits, 0 behind the last base; exactly (len + 31) / 32 words
static std::vector<uint64_t> pack(const Bases &b) {
    std::vector<uint64_t> w((b.size() + 31) / 32, 0ull);
    for (size_t i = 0; i < b.size(); i++) w[i / 32] |= (uint64_t)b[i] << (62 - 2 * (i % 32));
    return w;
}
// the byte model of a window: base t + j of s in group j, 0 where s has none
static uint64_t window(const Bases &s, int t) {
    uint64_t x = 0;
    for (int j = 0; j < 32; j++) {
        const int q = t + j;
        x = (x << 2) | (uint64_t)(q >= 0 && q < (int)s.size() ? s[(size_t)q] : 0);
    }
    return x;
}
static const uint64_t *ptr(const std::vector<uint64_t> &w) { return w.empty() ? nullptr : w.data(); }

// ---- one word, the lookups, the clamp ---------------------------------------------------------------------------------------------
static void check_words() {
    for (int rep = 0; rep < 200; rep++) {
        const uint64_t x = rep == 0 ? 0ull : rep == 1 ? ~0ull : rnd();
        for (int m = -3; m <= 35; m++) {
            uint64_t want = 0;
            for (int j = 0; j < 32; j++) if (j < m) want |= x & (3ull << (62 - 2 * j));
            if (pk_keep(x, m) != want) differ("pk_keep", m, rep, pk_keep(x, m), want);
        }
        uint64_t y = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
        y = ((y >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((y & 0x0F0F0F0F0F0F0F0Full) << 4);
        y = __builtin_bswap64(y);                                  // (two swaps and a byte swap)
        if (pk_rev2(x) != y) differ("pk_rev2", rep, 0, pk_rev2(x), y);
        uint64_t z = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);   // (five swaps, no byte swap)
        z = ((z >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((z & 0x0F0F0F0F0F0F0F0Full) << 4);
        z = ((z >> 8) & 0x00FF00FF00FF00FFull) | ((z & 0x00FF00FF00FF00FFull) << 8);
        z = ((z >> 16) & 0x0000FFFF0000FFFFull) | ((z & 0x0000FFFF0000FFFFull) << 16);
        z = (z >> 32) | (z << 32);
        if (pk_rev2(x) != z) differ("pk_rev2 (five swaps)", rep, 0, pk_rev2(x), z);
        z = 0;
        for (int j = 0; j < 32; j++) z |= ((x >> (2 * j)) & 3ull) << (62 - 2 * j);
        if (pk_rev2(x) != z) differ("pk_rev2 (group by group)", rep, 0, pk_rev2(x), z);
    }
    for (uint32_t c = 0; c < 4; c++) {
        if (pk_letter(c) != (uint32_t)"ACGT"[c]) differ("pk_letter", c, 0, pk_letter(c), (uint32_t)"ACGT"[c]);
        if (pk_code("ACGT"[c]) != c) differ("pk_code", c, 0, pk_code("ACGT"[c]), c);
    }
    for (int ch = 0; ch < 256; ch++)
        if (ch != 'A' && ch != 'C' && ch != 'G' && pk_code((char)ch) != 3) differ("pk_code (other)", ch, 0, pk_code((char)ch), 3);
    const int cv[][2] = {{29999, 29999}, {30000, 30000}, {30001, 30000}, {-29999, -29999}, {-30000, -30000}, {-30001, -30000},
                         {0, 0}, {INT_MAX, 30000}, {INT_MIN, -30000}};
    for (auto &c : cv) if (pk_clamp(c[0]) != c[1]) differ("pk_clamp", c[0], 0, (unsigned)pk_clamp(c[0]), (unsigned)c[1]);
}

// ---- pk_seg32, pk_base_of, fx_cat32 -----------------------------------------------------------------------------------------------
static void check_segment(const Bases &b) {
    const int len = (int)b.size();
    const std::vector<uint64_t> w = pack(b);
    for (int t = -40; t <= len + 16; t++)
        if (pk_seg32(ptr(w), len, t) != window(b, t)) differ("pk_seg32", len, t, pk_seg32(ptr(w), len, t), window(b, t));
    for (int t = 0; t < len; t++)
        if (pk_base_of(ptr(w), t) != b[(size_t)t]) differ("pk_base_of", len, t, pk_base_of(ptr(w), t), b[(size_t)t]);
}
// one record as the kernels see it (DynView's members): a key of PK_KW words, an extension of exactly its words
struct HostView { const uint64_t *key; const uint8_t *key_len; const uint64_t *ext; const int64_t *ext_off; const int32_t *ext_len, *marker; };
static void check_contig(int kl, int el) {
    const Bases k = random_bases((size_t)kl), e = random_bases((size_t)el);
    std::vector<uint64_t> kw = pack(k);
    kw.resize(PK_KW, 0ull);
    const std::vector<uint64_t> ew = pack(e);
    const uint8_t key_len = (uint8_t)kl;
    const int64_t ext_off = 0;
    const int32_t ext_len = el;
    for (int32_t marker = 1; marker <= 2; marker++) {
        const HostView v{kw.data(), &key_len, ptr(ew), &ext_off, &ext_len, &marker};
        const FxCat c = fx_contig(v, 0);
        Bases cat = marker == 1 ? k : e;
        const Bases &second = marker == 1 ? e : k;
        cat.insert(cat.end(), second.begin(), second.end());
        if (c.l0 + c.l1 != (int)cat.size()) differ("fx_contig (length)", kl, el, (unsigned)(c.l0 + c.l1), cat.size());
        for (int t = -40; t <= (int)cat.size() + 16; t++)
            if (fx_cat32(c, t) != window(cat, t)) differ(marker == 1 ? "fx_cat32 key+ext" : "fx_cat32 ext+key", kl * 1000 + el, t, fx_cat32(c, t), window(cat, t));
    }
}
static void check_segments() {
    for (int rep = 0; rep < 3; rep++)
        for (int len = 0; len <= 130; len++) check_segment(random_bases((size_t)len));
    // all T and all A: the zeros of the padding and the zeros of a base must not be confused
    for (int len = 0; len <= 130; len++) { check_segment(Bases((size_t)len, 3)); check_segment(Bases((size_t)len, 0)); }
    const int kls[] = {0, 1, 30, 31, 32, 33, 63, 64, 65, 95, 96, 97, 123, 124}, els[] = {0, 1, 31, 32, 33, 64, 65};
    for (int el = 0; el <= 130; el++) {
        for (int kl : kls) check_contig(kl, el);
        check_contig((int)(rnd() % 125), el);
    }
    for (int kl = 0; kl <= 124; kl++) {
        for (int el : els) check_contig(kl, el);
        check_contig(kl, (int)(rnd() % 131));
    }
}

// ---- Pk4 --------------------------------------------------------------------------------------------------------------------------
static Pk4 pk4_of(const Bases &b) {                                  // 128 base codes -> the four words
    uint64_t w[4] = {0, 0, 0, 0};
    for (int i = 0; i < 128; i++) w[i / 32] |= (uint64_t)b[(size_t)i] << (62 - 2 * (i % 32));
    return Pk4{w[0], w[1], w[2], w[3]};
}
static bool same(const Pk4 &a, const Pk4 &b) { return a.w0 == b.w0 && a.w1 == b.w1 && a.w2 == b.w2 && a.w3 == b.w3; }
static void check_pk4() {
    for (int rep = 0; rep < 6; rep++) {
        const Bases b = rep == 0 ? Bases(128, 3) : rep == 1 ? Bases(128, 0) : random_bases(128);
        const Pk4 a = pk4_of(b);
        for (int j = -1; j <= 5; j++) {
            const uint64_t want = j == 0 ? a.w0 : j == 1 ? a.w1 : j == 2 ? a.w2 : j == 3 ? a.w3 : 0ull;
            if (pk_word(a, j) != want) differ("pk_word", rep, j, pk_word(a, j), want);
        }
        for (int p = 0; p < 128; p++)
            if (pk_base(a, p) != b[(size_t)p]) differ("pk_base", rep, p, pk_base(a, p), b[(size_t)p]);
        for (int s = 0; s <= 127; s++) {
            Bases m(128, 0);
            for (int i = 0; i + s < 128; i++) m[(size_t)i] = b[(size_t)(i + s)];
            if (!same(pk_shl(a, s), pk4_of(m))) differ("pk_shl", rep, s, pk_shl(a, s).w0, pk4_of(m).w0);
        }
        for (int len = 0; len <= 128; len++) {
            Bases kept(128, 0), rev(128, 0);
            for (int i = 0; i < len; i++) { kept[(size_t)i] = b[(size_t)i]; rev[(size_t)i] = b[(size_t)(len - 1 - i)]; }
            if (!same(pk_keep4(a, len), pk4_of(kept))) differ("pk_keep4", rep, len, pk_keep4(a, len).w0, pk4_of(kept).w0);
            if (!same(pk_reverse(a, len), pk4_of(rev))) differ("pk_reverse", rep, len, pk_reverse(a, len).w0, pk4_of(rev).w0);
        }
        // a base code put in at every position of an empty word set comes back there and nowhere else
        for (int p = 0; p < 128; p++)
            for (uint64_t code = 1; code < 4; code++) {
                Pk4 z{0, 0, 0, 0};
                pk_or(z, p >> 5, pk_at(code, p));
                for (int q = 0; q < 128; q++)
                    if (pk_base(z, q) != (q == p ? code : 0ull)) differ("pk_at / pk_or / pk_base", p, q, pk_base(z, q), q == p ? code : 0ull);
            }
        // load / store at a record's index in an array of exactly its words
        std::vector<uint64_t> arr(3 * PK_KW, 0ull);
        pk_store(arr.data(), 2, a);
        if (!same(pk_load(arr.data(), 2), a) || arr[2 * PK_KW] != a.w0 || arr[3 * PK_KW - 1] != a.w3 || arr[2 * PK_KW - 1] != 0ull)
            differ("pk_load / pk_store", rep, 0, arr[2 * PK_KW], a.w0);
    }
    // dynamicSubKmerComparator on keys as the layout holds them (zeros behind the last base): every pair of lengths
    const Bases master = random_bases(128);
    for (int lx = 0; lx <= 124; lx++)
        for (int ly = 0; ly <= 124; ly++) {
            Bases x(128, 0), y(128, 0);
            for (int i = 0; i < lx; i++) x[(size_t)i] = master[(size_t)i];
            for (int i = 0; i < ly; i++) y[(size_t)i] = master[(size_t)i];
            const int m = lx < ly ? lx : ly;
            if (!pk_prefix(pk4_of(x), lx, pk4_of(y), ly)) differ("pk_prefix (equal or prefix)", lx, ly, 0, 1);
            if (m > 0) {
                y[(size_t)(m - 1)] ^= 1;                            // the two differ at the last base they share
                if (pk_prefix(pk4_of(x), lx, pk4_of(y), ly)) differ("pk_prefix (differs at the last shared base)", lx, ly, 1, 0);
                y[(size_t)(m - 1)] ^= 1;
            }
            if (ly > m) {
                y[(size_t)m] ^= 2;                                  // a difference behind the shorter key does not count
                if (!pk_prefix(pk4_of(x), lx, pk4_of(y), ly)) differ("pk_prefix (differs behind the shorter key)", lx, ly, 0, 1);
            }
        }
}

// ---- pk_find ----------------------------------------------------------------------------------------------------------------------
template <class T>
static void check_find_sizes(const std::vector<int> &sizes) {
    const int64_t n = (int64_t)sizes.size();
    std::vector<T> off((size_t)n);                                 // exactly n entries: off[n] must not be read
    int64_t run = 0;
    for (int64_t i = 0; i < n; i++) { off[(size_t)i] = (T)run; run += sizes[(size_t)i]; }
    for (int64_t i = 0; i < n; i++) {
        if (!sizes[(size_t)i]) continue;
        const int64_t first = (int64_t)off[(size_t)i], last = first + sizes[(size_t)i] - 1;
        if (pk_find(off.data(), n, first) != i) differ("pk_find (first item)", n, i, (uint64_t)pk_find(off.data(), n, first), (uint64_t)i);
        if (pk_find(off.data(), n, last) != i) differ("pk_find (last item)", n, i, (uint64_t)pk_find(off.data(), n, last), (uint64_t)i);
    }
}
static void check_find() {
    const std::vector<std::vector<int>> cases = {
        {1}, {7}, {1, 1}, {5, 3}, {0, 4}, {4, 0}, {0, 0, 0, 5, 2}, {3, 0, 0, 0, 2, 9}, {2, 6, 0, 0, 0}, {0, 0, 3, 0, 0, 1, 0, 0},
        {1, 0, 1, 0, 1, 0, 1}, {300, 1, 0, 0, 77, 0, 4096, 1, 1, 0}};
    for (auto &c : cases) { check_find_sizes<uint64_t>(c); check_find_sizes<int64_t>(c); }
    for (int rep = 0; rep < 200; rep++) {
        std::vector<int> c((size_t)(1 + rnd() % 40));
        for (auto &x : c) x = (rnd() & 3) ? (int)(rnd() % 50) : 0;
        check_find_sizes<uint64_t>(c); check_find_sizes<int64_t>(c);
    }
}

// ---- the decimal text of an int, an int out of text -----------------------------------------------------------------------------------
static void check_int_text_of(int v) {
    char want[16];
    const int n = snprintf(want, sizeof want, "%d", v);
    if (pk_int_chars(v) != n) differ("pk_int_chars", v, 0, (unsigned)pk_int_chars(v), (unsigned)n);
    for (int q = 0; q < n; q++)
        if (pk_int_char(v, q) != want[q]) differ("pk_int_char", v, q, (unsigned char)pk_int_char(v, q), (unsigned char)want[q]);
}
static void check_int_text() {
    const int vals[] = {0, 9, -9, 10, -10, 99, -99, 100, -100, 30000, -30000, INT_MAX, INT_MIN, INT_MAX - 1, INT_MIN + 1, 1000000000, -1000000000, 999999999};
    for (int v : vals) check_int_text_of(v);
    for (int rep = 0; rep < 4000; rep++) {
        check_int_text_of((int)(uint32_t)rnd());                   // the whole range
        check_int_text_of((int)(rnd() % 60001) - 30000);             // what the stages write
    }
}
// the rule, spelled out: an optional '-' or '+'; the digits that follow; the value is that of the shortest run of leading digits
// that reaches 10^8, or of all of them; no digits are 0; one '|' behind the digits is stepped over; nothing is read at or past e
static int parse_model(const std::string &t, int64_t &i, int64_t e) {
    bool neg = false;
    if (i < e && (t[(size_t)i] == '-' || t[(size_t)i] == '+')) { neg = t[(size_t)i] == '-'; i++; }
    std::string digits;
    while (i < e && t[(size_t)i] >= '0' && t[(size_t)i] <= '9') digits += t[(size_t)i++];
    long long v = 0;
    for (size_t n = 1; n <= digits.size(); n++) {
        v = atoll(digits.substr(0, n).c_str());
        if (v >= 100000000LL) break;
    }
    if (i < e && t[(size_t)i] == '|') i++;
    return (int)(neg ? -v : v);
}
static void check_parse() {
    struct Case { const char *text; int64_t e; };                  // e < 0: the end of the text
    const Case cases[] = {{"-12|7", -1}, {"+7|", -1}, {"7", -1}, {"", -1}, {"|", -1}, {"||5", -1}, {"-", -1}, {"-|4", -1}, {"+|", -1}, {"abc", -1},
                          {"12345", 3}, {"12|345", 1}, {"-12345|6", 4}, {"1|-2|+3", -1}, {"30000|-30000|0", -1}, {"1|-1|-1)", -1},
                          {"1234567890123|5", -1}, {"-999999999999|1", -1}, {"100000000|2", -1}, {"99999999|2", -1}, {"999999999|2", -1},
                          {"000000000123|4", -1}, {"5|||", -1}, {"2|x|3", -1}};
    for (auto &c : cases) {
        const std::string t = c.text;                                // (pk_parse_int gets a copy of exactly e bytes: a read at or past e is reported)
        const int64_t e = c.e < 0 ? (int64_t)t.size() : c.e;
        std::vector<char> exact(t.begin(), t.begin() + e);
        int64_t i = 0, j = 0;
        for (int field = 0; field < 3; field++) {                   // three fields in a row, as the binarizers read "m|l|r"
            const int got = pk_parse_int(exact.empty() ? nullptr : exact.data(), i, e), want = parse_model(t, j, e);
            if (got != want || i != j) differ(c.text, field, i * 100 + j, (unsigned)got, (unsigned)want);
        }
    }
}

int main() {
    check_words();
    check_segments();
    check_pk4();
    check_find();
    check_int_text();
    check_parse();
    if (failures) { fprintf(stderr, "%d differences\n", failures); return 1; }
    printf("packed word helpers: ok\n");
    return 0;
}
