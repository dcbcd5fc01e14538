// pk_letters16 (reflexiv_amd/csrc/rfx_packed_words.h), the sixteen-letter decode of the two text writers, against a byte model, as a
// host program.  Built by tests/test_packed_letters_host.py with the host compiler and -fsanitize=address,undefined: every packed
// array is exactly (len + 31) / 32 words long, so a load of a word behind the last base is reported.  Exit status 0: no difference.
#define __host__
#define __device__
#include "rfx_packed_words.h"

#include <cstdio>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {                                           // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main() {
    int failures = 0;
    // every length up to four words and a half, every start at which sixteen bases are left: the last sixteen of a sequence too
    for (int len = 16; len <= 150; len++) {
        std::vector<uint8_t> b((size_t)len);
        for (auto &x : b) x = (uint8_t)(rnd() & 3);
        std::vector<uint64_t> w(((size_t)len + 31) / 32, 0ull);
        for (int i = 0; i < len; i++) w[(size_t)i / 32] |= (uint64_t)b[(size_t)i] << (62 - 2 * (i % 32));
        for (int t = 0; t + 16 <= len; t++) {
            const Pk16 y = pk_letters16(w.data(), t);
            const uint32_t got[4] = {y.a, y.b, y.c, y.d};
            for (int j = 0; j < 16; j++) {
                const char want = "ACGT"[b[(size_t)(t + j)]], have = (char)(got[j >> 2] >> (8 * (j & 3)));
                if (want != have && failures++ < 20) fprintf(stderr, "pk_letters16: len %d, t %d, byte %d: got %c want %c\n", len, t, j, have, want);
            }
        }
    }
    if (failures) { fprintf(stderr, "%d differences\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
