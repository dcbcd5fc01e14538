// rfx_count_tuning.h -- the count stage's environment knobs, parsed in one place.
//
// Host-only and free of HIP: a plain C++ program can include it (tests/count_tuning_main.cpp does).  The knobs exist so
// that the tests can force every path of the count stage at small shapes and tools/ can sweep a constant without a
// rebuild; none of them is needed in normal use.  count_tuning() reads the environment on EVERY call -- the tests change
// these variables between the cases of one process -- so call it where a knob is needed, never keep its result in a
// static.  DESIGN.md section 31 has the table of knobs, what each forces and which test uses it.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace rfxc {
#pragma GCC visibility push(hidden)   // internal to the library: none of this is among its exported symbols

constexpr int MAX_BITS = 10;          // widest radix digit of a level (1024 bins)

struct CountTuning {
    // RFX_LEVEL_BITS ("9,9"): the radix plan, level by level.  Entries outside 0..MAX_BITS are dropped; when none is left
    // the plan is computed as if the variable were unset -- except that plan_wide_record_levels keeps plan_levels' split
    // whenever the variable is set at all (level_bits_set).
    std::vector<int> level_bits;
    bool level_bits_set = false;
    double leaf_target = 0;           // RFX_LEAF_TARGET: instances per leaf the plan aims at (<= 0 or unset: the caller's)
    // RFX_HEAVY ("heavy,slice,pcap", in elements): the heavy-leaf thresholds; taken only when all three parse and are non-zero
    bool heavy_set = false;
    unsigned long long heavy = 0, heavy_slice = 0, heavy_pcap = 0;
    bool presplit_set = false;        // RFX_PRESPLIT: elements beyond which a leaf of k_leaf_count starts in parts
    uint32_t presplit_env = 0;
    bool wide_presplit_set = false;   // RFX_WIDE_PRESPLIT: the same for the k > 32 leaves
    uint32_t wide_presplit_env = 0;
    bool sk_desc = true;              // RFX_SK_DESC=0: level 1's two-pass form recomputes the runs instead of storing descriptors
    int sk_onesweep = 1;              // RFX_SK_ONESWEEP: level 1 in one sweep 0 never, 1 from 2^22 segments up, 2 at any size
    int sk_onesweep_cap = 100;        // RFX_SK_ONESWEEP_CAP: per cent of the planned region a bucket may take (>= 1)
    bool rec_onesweep_set = false;    // RFX_REC_ONESWEEP: a received array's first level without a histogram 0 never,
    int rec_onesweep_env = 0;         //   1 every element kind from 2^24 records up, 2 at any size
    bool l2_onesweep = true;          // RFX_L2_ONESWEEP=0: the last level always in the exact form
    int l2_squeeze = 100;             // RFX_L2_SQUEEZE: per cent of the sampled size a child's region gets (>= 1)
    bool wide_records = true;         // RFX_WIDE_RECORDS=0: uniform reads at k = 33..63 take the element path
    bool trace = false;               // RFX_TRACE (set to anything): one line per decision on stderr

    // the knobs whose default depends on who asks
    uint32_t presplit(bool record_leaves) const { return presplit_set ? presplit_env : record_leaves ? 8000u : 0u; }
    uint32_t wide_presplit(bool record_leaves) const { return wide_presplit_set ? wide_presplit_env : record_leaves ? 2600u : 0u; }
    // mode: the level kernels' element kind (LevelElem<MODE>); on by default for the super-k-mer records (0 and 3)
    int rec_onesweep(int mode) const { return rec_onesweep_set ? rec_onesweep_env : (mode == 0 || mode == 3 ? 1 : 0); }
    double leaf_target_or(double target) const { return leaf_target > 0 ? leaf_target : target; }
};

inline CountTuning count_tuning() {
    CountTuning t;
    if (const char *e = getenv("RFX_LEVEL_BITS")) {
        t.level_bits_set = true;
        for (const char *q = e; *q;) {
            int v = atoi(q);
            if (v >= 0 && v <= MAX_BITS) t.level_bits.push_back(v);
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
    }
    if (const char *e = getenv("RFX_LEAF_TARGET")) t.leaf_target = atof(e);
    if (const char *e = getenv("RFX_HEAVY")) {
        unsigned long long a = 0, b = 0, c = 0;
        if (sscanf(e, "%llu,%llu,%llu", &a, &b, &c) == 3 && a && b && c) {
            t.heavy_set = true; t.heavy = a; t.heavy_slice = b; t.heavy_pcap = c;
        }
    }
    if (const char *e = getenv("RFX_PRESPLIT")) { t.presplit_set = true; t.presplit_env = (uint32_t)atoi(e); }
    if (const char *e = getenv("RFX_WIDE_PRESPLIT")) { t.wide_presplit_set = true; t.wide_presplit_env = (uint32_t)atoi(e); }
    if (const char *e = getenv("RFX_SK_DESC")) t.sk_desc = atoi(e) != 0;
    if (const char *e = getenv("RFX_SK_ONESWEEP")) t.sk_onesweep = atoi(e);
    if (const char *e = getenv("RFX_SK_ONESWEEP_CAP")) { const int v = atoi(e); t.sk_onesweep_cap = v > 1 ? v : 1; }
    if (const char *e = getenv("RFX_REC_ONESWEEP")) { t.rec_onesweep_set = true; t.rec_onesweep_env = atoi(e); }
    if (const char *e = getenv("RFX_L2_ONESWEEP")) t.l2_onesweep = atoi(e) != 0;
    if (const char *e = getenv("RFX_L2_SQUEEZE")) { const int v = atoi(e); t.l2_squeeze = v > 1 ? v : 1; }
    if (const char *e = getenv("RFX_WIDE_RECORDS")) t.wide_records = atoi(e) != 0;
    t.trace = getenv("RFX_TRACE") != nullptr;
    return t;
}

// level 1 of a record path in one sweep (k_sk_onesweep): when the input is large enough for a sampled histogram to size
// the regions, or always under RFX_SK_ONESWEEP=2.  n_threads: the segments of the read set.
inline bool sweep_level1(const CountTuning &t, int64_t n_threads) {
    return t.sk_onesweep && (t.sk_onesweep == 2 || n_threads >= ((int64_t)1 << 22));
}

// uniform reads at k = 33..63 go through super-k-mer records (the default) or, under RFX_WIDE_RECORDS=0, the element path
inline bool wide_records_enabled(const CountTuning &t, int k) { return t.wide_records && k >= 33 && k <= 63; }

#pragma GCC visibility pop
}  // namespace rfxc
