// Host check of reflexiv_amd/csrc/rfx_reduce_fsm.h (tests/test_reduce_fsm_host.py compiles this under -fsanitize=address,undefined
// and runs it): the two window adjustments of the k-mer reduction stage, once as the sequential loop with two pending rows written
// the way the reference writes it (every branch spelled out, the header's window function NOT used), once as the formulation the
// kernels use -- a map per row, a blocked scan of the maps (reduce per block, scan of the block aggregates, apply), a count per row,
// a scan of the counts, the emission with the flush done by the row that ends a partition -- and the two must write the same rows.
//
// A row is (short or long, group, marker, extension, id): a short row's key is its group, a long row's key its group plus a tail,
// so a short key is a prefix of a long one exactly when the groups agree.  Inputs: every sequence of up to 4 rows over all 16
// (length, group, marker sign, extension) symbols; every sequence of 5 and 6 rows over the 8 (length, group, extension) symbols
// with the marker sign taken from the position (two patterns); every sequence of 7 rows over the 4 (length, group) symbols with
// extension and sign from the position (eight patterns); 40 seeded random sequences of 10,000 rows cut into partitions, empty
// ones included.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rfx_reduce_fsm.h"

struct Row { bool s; int g, mk, ext, id; };
struct Out { int id, ext, mk; bool operator==(const Out &o) const { return id == o.id && ext == o.ext && mk == o.mk; } };

static bool pre(const Row &x, const Row &y) { return x.s == y.s ? (x.g == y.g && x.id == y.id) : x.g == y.g; }
static Out plain(const Row &r) { return Out{r.id, r.ext, r.mk}; }
static Out edited(const Row &t, const Row &src) { return Out{t.id, src.ext, (src.mk < 0 && t.mk >= 0) ? -1 : t.mk}; }

// ---- the reference's loop, one partition ---------------------------------------------------------------------------------------------
static void sequential(bool right, const Row *r, int n, std::vector<Out> &out) {
    const Row *a = nullptr, *b = nullptr;
    for (int i = 0; i < n; i++) {
        const Row *c = r + i;
        if (!a) { a = c; continue; }
        if (!b) { b = c; continue; }
        if (a->s) {
            if (b->s) {
                if (c->s) { out.push_back(plain(*a)); out.push_back(plain(*b)); a = c; b = nullptr; }
                else if (pre(*c, *b)) { out.push_back(plain(*a)); a = b; b = c; }
                else { out.push_back(plain(*a)); out.push_back(plain(*b)); a = c; b = nullptr; }
            } else {
                if (c->s) {
                    if (pre(*b, *a)) { if (!right) out.push_back(plain(*a)); out.push_back(edited(*b, *a)); a = c; b = nullptr; }
                    else if (pre(*c, *b)) { out.push_back(plain(*a)); a = b; b = c; }
                    else { out.push_back(plain(*a)); out.push_back(plain(*b)); a = c; b = nullptr; }
                } else {
                    if (pre(*b, *a) && pre(*c, *a)) {
                        if (!(right && (a->ext == b->ext || a->ext == c->ext))) out.push_back(plain(*a));
                        out.push_back(plain(*b)); out.push_back(plain(*c)); a = b = nullptr;
                    } else if (pre(*b, *a)) { if (!right) out.push_back(plain(*a)); out.push_back(edited(*b, *a)); a = c; b = nullptr; }
                    else { out.push_back(plain(*a)); a = b; b = c; }
                }
            }
        } else {
            if (b->s) {
                if (c->s) {
                    if (pre(*a, *b)) { out.push_back(edited(*a, *b)); if (!right) out.push_back(plain(*b)); a = c; b = nullptr; }
                    else { out.push_back(plain(*a)); out.push_back(plain(*b)); a = c; b = nullptr; }
                } else {
                    if (pre(*a, *b) && pre(*c, *b)) {
                        out.push_back(plain(*a));
                        if (!(right && (a->ext == b->ext || b->ext == c->ext))) out.push_back(plain(*b));
                        out.push_back(plain(*c)); a = b = nullptr;
                    } else if (pre(*a, *b)) { out.push_back(edited(*a, *b)); if (!right) out.push_back(plain(*b)); a = c; b = nullptr; }
                    else if (pre(*c, *b)) { out.push_back(plain(*a)); a = b; b = c; }
                    else { out.push_back(plain(*a)); out.push_back(plain(*b)); a = c; b = nullptr; }
                }
            } else {
                if (c->s) {
                    if (pre(*a, *c) && pre(*c, *b)) {
                        out.push_back(plain(*a)); out.push_back(plain(*b));
                        if (!(right && (a->ext == c->ext || b->ext == c->ext))) out.push_back(plain(*c));
                        a = b = nullptr;
                    } else if (pre(*c, *b)) { out.push_back(plain(*a)); a = b; b = c; }
                    else { out.push_back(plain(*a)); out.push_back(plain(*b)); a = c; b = nullptr; }
                } else { out.push_back(plain(*a)); a = b; b = c; }
            }
        }
    }
    if (a && b) {
        if (a->s && !b->s && pre(*a, *b)) { if (!right) out.push_back(plain(*a)); out.push_back(edited(*b, *a)); }
        else if (!a->s && b->s) { if (pre(*a, *b)) { out.push_back(edited(*a, *b)); if (!right) out.push_back(plain(*b)); } }
        else { out.push_back(plain(*a)); out.push_back(plain(*b)); }
    } else if (a) out.push_back(plain(*a));
}

// ---- the kernels' formulation, all partitions at once ---------------------------------------------------------------------------------
static unsigned window_bits(const Row *r, int i) {           // rows i - 2, i - 1, i (i >= 2)
    const Row &a = r[i - 2], &b = r[i - 1], &c = r[i];
    return (a.s ? RFX_FSM_SA : 0) | (b.s ? RFX_FSM_SB : 0) | (c.s ? RFX_FSM_SC : 0) | (pre(a, b) ? RFX_FSM_PAB : 0) | (pre(b, c) ? RFX_FSM_PBC : 0) |
           (pre(a, c) ? RFX_FSM_PAC : 0) | (a.ext == b.ext ? RFX_FSM_EAB : 0) | (b.ext == c.ext ? RFX_FSM_EBC : 0) | (a.ext == c.ext ? RFX_FSM_EAC : 0);
}
static void put(const rfx_fsm_step &st, const Row *const rows[3], Out *dst) {
    int q = 0;
    for (int j = 0; j < 3; j++) {
        if (!(st.emit >> j & 1)) continue;
        if (st.edit == 1 && j == 0) dst[q++] = edited(*rows[0], *rows[1]);
        else if (st.edit == 2 && j == 1) dst[q++] = edited(*rows[1], *rows[0]);
        else dst[q++] = plain(*rows[j]);
    }
}
// agg[b] := the composite of the aggregates before b, as k_rd_scan_aggs computes it with one block of T threads
static void scan_aggs_as_the_kernel(std::vector<unsigned> &agg, int nb, int T) {
    const long per = ((long)nb + T - 1) / T;
    std::vector<unsigned> sh(T), x(T);
    auto b0_of = [&](int t) { return (long)t * per; };
    auto b1_of = [&](int t) { const long b0 = (long)t * per; return b0 + per < nb ? b0 + per : (long)nb; };
    for (int t = 0; t < T; t++) {
        unsigned m = RFX_FSM_IDENTITY;
        for (long b = b0_of(t); b < b1_of(t); b++) m = rfx_fsm_compose(m, agg[b]);
        sh[t] = m;
    }
    for (int d = 1; d < T; d <<= 1) {                                // rd_block_scan: every thread reads, then every thread writes
        for (int t = 0; t < T; t++) x[t] = t >= d ? rfx_fsm_compose(sh[t - d], sh[t]) : sh[t];
        sh = x;
    }
    for (int t = 0; t < T; t++) {
        unsigned run = t ? sh[t - 1] : RFX_FSM_IDENTITY;
        for (long b = b0_of(t); b < b1_of(t); b++) { const unsigned v = agg[b]; agg[b] = run; run = rfx_fsm_compose(run, v); }
    }
}
// T == 0: the aggregates are scanned by a running composite; T > 0: in the kernel's form with T threads
static void scanned(bool right, const Row *r, int n, const std::vector<int> &ps, int block, int T, std::vector<Out> &out) {
    static std::vector<unsigned char> start, end;
    start.assign(n, 0); end.assign(n, 0);
    for (size_t p = 0; p + 1 < ps.size(); p++) if (ps[p] < ps[p + 1]) { start[ps[p]] = 1; end[ps[p + 1] - 1] = 1; }
    static std::vector<unsigned> map, state, cnt, agg;
    static std::vector<size_t> off;
    map.resize(n); state.resize(n); cnt.resize(n);
    for (int i = 0; i < n; i++) map[i] = rfx_fsm_map(start[i], i >= 2 ? rfx_fsm_window(right, window_bits(r, i)).next : 0u);
    const int nb = (n + block - 1) / block;
    agg.assign(nb, RFX_FSM_IDENTITY);
    for (int b = 0; b < nb; b++) for (int i = b * block; i < n && i < (b + 1) * block; i++) agg[b] = rfx_fsm_compose(agg[b], map[i]);
    if (T > 0) scan_aggs_as_the_kernel(agg, nb, T);
    else {
        unsigned run = RFX_FSM_IDENTITY;
        for (int b = 0; b < nb; b++) { const unsigned t = agg[b]; agg[b] = run; run = rfx_fsm_compose(run, t); }
    }
    for (int b = 0; b < nb; b++) {
        unsigned m = agg[b];
        for (int i = b * block; i < n && i < (b + 1) * block; i++) { state[i] = rfx_fsm_apply(m, 0u); m = rfx_fsm_compose(m, map[i]); }
    }
    auto steps = [&](int i, rfx_fsm_step &w, rfx_fsm_step &f, bool &one) {      // what row i writes: its window, then its flush
        const unsigned s = start[i] ? 0u : state[i];
        w = rfx_fsm_step{s + 1, 0u, 0u}; f = rfx_fsm_step{0u, 0u, 0u}; one = false;
        if (s == 2) w = rfx_fsm_window(right, window_bits(r, i));
        if (end[i]) {
            if (w.next == 2) f = rfx_fsm_flush(right, (r[i - 1].s ? RFX_FSM_SA : 0) | (r[i].s ? RFX_FSM_SB : 0) | (pre(r[i - 1], r[i]) ? RFX_FSM_PAB : 0));
            else if (w.next == 1) one = true;
        }
    };
    for (int i = 0; i < n; i++) {
        rfx_fsm_step w, f; bool one;
        steps(i, w, f, one);
        cnt[i] = rfx_fsm_popcount3(w.emit) + rfx_fsm_popcount3(f.emit) + (one ? 1u : 0u);
        if (cnt[i] > 3) { std::printf("a row writes %u records\n", cnt[i]); std::exit(1); }
    }
    off.assign(n + 1, 0);
    for (int i = 0; i < n; i++) off[i + 1] = off[i] + cnt[i];
    out.assign(off[n], Out{-1, -1, -1});
    for (int i = 0; i < n; i++) {
        rfx_fsm_step w, f; bool one;
        steps(i, w, f, one);
        Out *dst = out.data() + off[i];
        if (w.emit) { const Row *rows[3] = {r + i - 2, r + i - 1, r + i}; put(w, rows, dst); dst += rfx_fsm_popcount3(w.emit); }
        if (f.emit) { const Row *rows[3] = {r + i - 1, r + i, nullptr}; put(f, rows, dst); }
        if (one) *dst = plain(r[i]);
    }
}

static long checked = 0;
static void check(const std::vector<Row> &rows, const std::vector<int> &ps, int block, int T) {
    for (int right = 0; right < 2; right++) {
        static std::vector<Out> a, b;
        a.clear();
        for (size_t p = 0; p + 1 < ps.size(); p++) sequential(right != 0, rows.data() + ps[p], ps[p + 1] - ps[p], a);
        for (int form = 0; form < (T > 0 ? 2 : 1); form++) {                     // the running composite, then (T > 0) the kernel's form
            b.clear();
            scanned(right != 0, rows.data(), (int)rows.size(), ps, block, form ? T : 0, b);
            if (!(a == b)) {
                std::printf("MISMATCH right=%d n=%zu partitions=%zu block=%d T=%d: %zu vs %zu rows\n", right, rows.size(), ps.size() - 1, block, form ? T : 0,
                            a.size(), b.size());
                if (rows.size() <= 64) for (const Row &r : rows) std::printf("  row %d: %c g%d mk%d e%d\n", r.id, r.s ? 'S' : 'L', r.g, r.mk, r.ext);
                std::exit(1);
            }
            checked++;
        }
    }
}
static Row symbol(int sym, int id) { return Row{(sym & 1) != 0, (sym >> 1) & 1, (sym >> 3) & 1 ? -1 : 5, (sym >> 2) & 1, id}; }

int main() {
    for (int n = 0; n <= 7; n++) {
        const int A = n <= 4 ? 16 : n <= 6 ? 8 : 4, patterns = n <= 4 ? 1 : n <= 6 ? 2 : 8;
        long total = 1;
        for (int i = 0; i < n; i++) total *= A;
        std::vector<Row> rows(n);
        for (long code = 0; code < total; code++) for (int pat = 0; pat < patterns; pat++) {
            long c = code;
            for (int i = 0; i < n; i++) {
                int sym = (int)(c % A);
                c /= A;
                if (A == 8) sym |= ((i + pat) & 1) ? 8 : 0;                     // the marker sign from the position
                if (A == 4) sym |= (((i * 5 + pat) >> 1) & 1 ? 4 : 0) | (((i + pat) & 1) ? 8 : 0);   // extension and sign from it
                rows[i] = symbol(sym, i);
            }
            check(rows, {0, n}, 3, n <= 5 || code % 8 == 0 ? 4 : 0);            // one partition, blocks of 3: aggregates from 4 rows on
            if (n >= 3 && code % 7 == 0) check(rows, {0, 0, n / 2, n / 2, n}, 2, 2);    // cut in two, empty partitions between
        }
    }
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    auto random_rows = [&](int t, int n) {
        std::vector<Row> rows(n);
        const int long_bias = t % 4;                                             // 3: mostly long rows, state 2 for long stretches
        for (int i = 0; i < n; i++) {
            int sym = (int)(rnd() & 15);
            if (long_bias == 3 && (rnd() & 7)) sym &= ~1;
            rows[i] = symbol(sym, i);
            if (long_bias >= 2) rows[i].g = 0;                                   // one group: every prefix test passes
        }
        return rows;
    };
    auto random_cuts = [&](int t, int n) {
        const int P = 1 + (int)(rnd() % 63);
        std::vector<int> ps(P + 1, 0);
        for (int p = 1; p < P; p++) ps[p] = (int)(rnd() % (n + 1));
        ps[P] = n;
        for (int p = 1; p < P; p++) for (int q = p + 1; q < P; q++) if (ps[q] < ps[p]) { const int s = ps[p]; ps[p] = ps[q]; ps[q] = s; }
        if (t % 5 == 0 && P > 3) ps[2] = ps[1];                                  // an empty partition
        return ps;
    };
    for (int t = 0; t < 40; t++) {
        const int n = 10000;
        const std::vector<Row> rows = random_rows(t, n);
        check(rows, random_cuts(t, n), 256, 256);
        check(rows, random_cuts(t, n), 4, 4);                                    // per = 625
        for (int m = 1; m <= 50; m++) {                                          // 1 .. 13 blocks of 4 on 4 threads: per = 1 .. 4
            const std::vector<Row> head(rows.begin(), rows.begin() + m);
            check(head, {0, m}, 4, 4);
            if (m >= 8) check(head, {0, 5, 5, m - 2, m}, 4, 4);
        }
    }
    for (int t = 0; t < 4; t++) for (int n : {65537, 131073}) {                  // 257 and 513 blocks on 256 threads: per = 2 and 3
        const std::vector<Row> rows = random_rows(t, n);
        check(rows, {0, n}, 256, 256);
        check(rows, random_cuts(t, n), 256, 256);
    }
    std::printf("ok %ld comparisons\n", checked);
    return 0;
}
