// rfx_synth.hip -- the benchmark's input on the device: a random genome (k_synth_genome) and error-bearing paired reads
// drawn from it (k_synth_reads), both as 2-bit packed words and a pure function of the seed, so that bench.py never
// ships reads over PCIe.  Not part of the pipeline.
#include "rfx_internal.h"
#include "rfx_device.h"

using namespace rfxd;

namespace {

// ------------------------------------------------------------ synthetic reads

constexpr uint64_t TAG_GENOME = 0x47454E4F4D45ULL, TAG_PAIRS = 0x5041495253ULL, TAG_ERRORS = 0x4552524F5253ULL;

__global__ void k_synth_genome(uint64_t sg, int64_t nw, uint64_t *__restrict__ g) {
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nw) g[j] = splitmix64(sg + (uint64_t)j);
}

__device__ __forceinline__ unsigned genome_base(const uint64_t *__restrict__ g, int64_t i) {
    return (unsigned)((g[i >> 5] >> (62 - 2 * (i & 31))) & 3);
}

// one thread per output word of a read
__global__ void k_synth_reads(uint64_t sp, uint64_t se, const uint64_t *__restrict__ genome,
                              int64_t genome_len, int64_t first_read, int64_t n_reads, int read_len,
                              uint32_t err, int wpr, uint64_t *__restrict__ words) {
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_reads * wpr) return;
    int64_t rl = t / wpr;
    int w = (int)(t % wpr);
    int64_t r = first_read + rl;
    uint64_t pair = (uint64_t)r >> 1;
    int mate = (int)(r & 1);
    uint64_t u = splitmix64(sp + pair);
    int64_t s = (int64_t)(u & 0xFFFF) + (int64_t)((u >> 16) & 0xFFFF) + (int64_t)((u >> 32) & 0xFFFF) +
                (int64_t)((u >> 48) & 0xFFFF);
    int64_t frag = 350 + ((s - 131070) * 35) / 37837;
    if (frag < read_len) frag = read_len;
    if (frag > genome_len) frag = genome_len;
    uint64_t v = splitmix64(u);
    int64_t start = (int64_t)((v >> 1) % (uint64_t)(genome_len - frag + 1));
    int strand = (int)(v & 1);
    int is_rc = mate ^ strand;
    int64_t pos = is_rc ? start + frag - read_len : start;
    uint64_t x = 0;
    for (int jj = 0; jj < 32; jj++) {
        int j = w * 32 + jj;
        unsigned b = 0;
        if (j < read_len) {
            b = is_rc ? 3u - genome_base(genome, pos + read_len - 1 - j) : genome_base(genome, pos + j);
            uint64_t e = splitmix64(se + (uint64_t)r * (uint64_t)read_len + (uint64_t)j);
            if ((uint32_t)e < err) b = (b + 1u + (unsigned)((e >> 32) % 3u)) & 3u;
        }
        x = (x << 2) | b;
    }
    words[t] = x;
}

}  // namespace

namespace rfx {

int synth_genome(rfx_ctx *ctx, uint64_t seed, int64_t genome_len, uint64_t *d_genome) {
    int64_t nw = (genome_len + 31) / 32;
    if (nw <= 0) return RFX_E_ARG;
    RFX_LAUNCH(k_synth_genome, dim3((unsigned)ceil_div(nw, 256)), dim3(256), 0,
               splitmix64(seed ^ TAG_GENOME), nw, d_genome);
    return RFX_OK;
}

int synth_reads(rfx_ctx *ctx, uint64_t seed, const uint64_t *d_genome, int64_t genome_len,
                int64_t first_read, int64_t n_reads, int read_len, uint32_t err, int words_per_read,
                uint64_t *d_words) {
    if (read_len > genome_len || words_per_read * 32 < read_len) return RFX_E_ARG;
    int64_t total = n_reads * words_per_read;
    if (total <= 0) return RFX_OK;
    RFX_LAUNCH(k_synth_reads, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0,
               splitmix64(seed ^ TAG_PAIRS), splitmix64(seed ^ TAG_ERRORS), d_genome, genome_len,
               first_read, n_reads, read_len, err, words_per_read, d_words);
    return RFX_OK;
}

}  // namespace rfx
