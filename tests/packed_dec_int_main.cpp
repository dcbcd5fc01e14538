// pk_dec_int (reflexiv_amd/csrc/rfx_packed_words.h), the strict decimal parser of the row parsers of 07EndExtend and 08Extend, as a
// host program: a fixed list of texts with the results written out by hand, then random texts against strtoll.  Built by
// tests/test_packed_dec_int_host.py with the host compiler and -fsanitize=address,undefined: every text lives in a heap buffer of
// exactly its length, so a read at or past `e` is reported.  Exit status 0: no difference.
#define __host__
#define __device__
#include "rfx_packed_words.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

// what the parser must say of a text: an int and where it stops, or no int (then *out stays as it was)
struct Want { bool ok; int v; int p; };
#define Y(v, p) Want{true, v, p}
#define N Want{false, 0, 0}
// the four ways the parser is asked: as Integer.toString writes ('-' only, no leading zero, no "-0"); as Integer.parseInt reads ('-'
// and '+', any zeros); digits only; '+' only and canonical
static const struct { bool sign, plus, canon; } MODES[4] = {{true, false, true}, {true, true, false}, {false, false, false}, {false, true, true}};
static const struct { const char *s; Want m[4]; } FIXED[] = {
    {"", {N, N, N, N}},
    {"-", {N, N, N, N}},
    {"+", {N, N, N, N}},
    {"0", {Y(0, 1), Y(0, 1), Y(0, 1), Y(0, 1)}},
    {"-0", {N, Y(0, 2), N, N}},
    {"+0", {N, Y(0, 2), N, Y(0, 2)}},
    {"00", {N, Y(0, 2), Y(0, 2), N}},
    {"007", {N, Y(7, 3), Y(7, 3), N}},
    {"-007", {N, Y(-7, 4), N, N}},
    {"7", {Y(7, 1), Y(7, 1), Y(7, 1), Y(7, 1)}},
    {"-7", {Y(-7, 2), Y(-7, 2), N, N}},
    {"+7", {N, Y(7, 2), N, Y(7, 2)}},
    {"12_", {Y(12, 2), Y(12, 2), Y(12, 2), Y(12, 2)}},
    {"12,", {Y(12, 2), Y(12, 2), Y(12, 2), Y(12, 2)}},
    {"1x", {Y(1, 1), Y(1, 1), Y(1, 1), Y(1, 1)}},
    {"x1", {N, N, N, N}},
    {" 1", {N, N, N, N}},
    {"2147483647", {Y(2147483647, 10), Y(2147483647, 10), Y(2147483647, 10), Y(2147483647, 10)}},
    {"2147483648", {N, N, N, N}},
    {"-2147483648", {Y(INT32_MIN, 11), Y(INT32_MIN, 11), N, N}},
    {"-2147483649", {N, N, N, N}},
    {"4294967296", {N, N, N, N}},
    {"9999999999", {N, N, N, N}},
    {"10000000000", {N, N, N, N}},
    {"99999999999", {N, N, N, N}},
    {"-99999999999", {N, N, N, N}},
    {"123456789012345", {N, N, N, N}},
    {"1-2", {Y(1, 1), Y(1, 1), Y(1, 1), Y(1, 1)}},
    {"--1", {N, N, N, N}},
    {"+-1", {N, N, N, N}},
    {"-+1", {N, N, N, N}},
    {"30000_-30001", {Y(30000, 5), Y(30000, 5), Y(30000, 5), Y(30000, 5)}},
    {"303_", {Y(303, 3), Y(303, 3), Y(303, 3), Y(303, 3)}},
    {"-1l", {Y(-1, 2), Y(-1, 2), N, N}},
    {"r1-", {N, N, N, N}},
};

// the same of a random text, the scan and the value by strtoll (which takes either sign and any zeros, and saturates far outside int);
// more than ten digits are no int to the parser, whatever their value
static Want by_strtoll(const std::string &s, bool sign, bool plus, bool canon) {
    const bool minus = !s.empty() && s[0] == '-', signed_ = minus || (!s.empty() && s[0] == '+');
    if (signed_ && !(minus ? sign : plus)) return N;
    char *end = nullptr;
    const long long v = strtoll(s.c_str(), &end, 10);
    const int stop = (int)(end - s.c_str()), nd = stop - (signed_ ? 1 : 0);
    if (nd <= 0 || nd > 10 || v < INT32_MIN || v > INT32_MAX) return N;
    if (canon && ((nd > 1 && s[signed_ ? 1 : 0] == '0') || (minus && v == 0))) return N;
    return Y((int)v, stop);
}

static int check(const std::string &s, bool sign, bool plus, bool canon, const Want &w) {
    std::vector<char> buf(s.begin(), s.end());                    // exactly s.size() bytes: no terminator to run into
    int64_t p = 0;
    int v = -12345;
    const bool ok = pk_dec_int(buf.data(), p, (int64_t)buf.size(), sign, plus, canon, &v);
    if (ok == w.ok && (ok ? v == w.v && p == w.p : v == -12345) && p >= 0 && p <= (int64_t)buf.size()) return 0;
    fprintf(stderr, "pk_dec_int(\"%s\", sign %d, plus %d, canon %d): got %d %d at %lld, want %d %d at %d\n", s.c_str(), sign, plus, canon, ok, v, (long long)p, w.ok,
            w.v, w.p);
    return 1;
}

int main() {
    int failures = 0;
    for (const auto &f : FIXED)
        for (int m = 0; m < 4; m++) failures += check(f.s, MODES[m].sign, MODES[m].plus, MODES[m].canon, f.m[m]);
    uint64_t z = 88172645463325252ull;
    for (int i = 0; i < 4000 && failures < 20; i++) {             // random digits, signs and separators, up to 14 characters
        std::string s;
        z ^= z << 13; z ^= z >> 7; z ^= z << 17;
        const int len = (int)(z % 15);
        for (int j = 0; j < len; j++) {
            z ^= z << 13; z ^= z >> 7; z ^= z << 17;
            s += "0123456789012345-+_,"[z % 20];
        }
        for (int mode = 0; mode < 8; mode++) failures += check(s, mode & 1, mode & 2, mode & 4, by_strtoll(s, mode & 1, mode & 2, mode & 4));
    }
    if (failures) { fprintf(stderr, "%d differences\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
