// The count stage's knob parser (reflexiv_amd/csrc/rfx_count_tuning.h) as a host program.  Built by
// tests/test_count_tuning_host.py with the host compiler and -fsanitize=address,undefined.  It sets and unsets the RFX_*
// variables, calls count_tuning() and checks what comes back against the rules the count stage has always parsed them by.
// Exit status 0: no difference.
#include "rfx_count_tuning.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace rfxc;

static int failures = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { failures++; fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static const char *const KNOBS[] = {"RFX_LEVEL_BITS",  "RFX_LEAF_TARGET",     "RFX_HEAVY",        "RFX_PRESPLIT",  "RFX_WIDE_PRESPLIT",
                                    "RFX_SK_DESC",     "RFX_SK_ONESWEEP",     "RFX_SK_ONESWEEP_CAP", "RFX_REC_ONESWEEP", "RFX_L2_ONESWEEP",
                                    "RFX_L2_SQUEEZE",  "RFX_WIDE_RECORDS",    "RFX_TRACE"};
static void clear_env() {
    for (const char *k : KNOBS) unsetenv(k);
}
static CountTuning with(const char *name, const char *value) {
    clear_env();
    setenv(name, value, 1);
    return count_tuning();
}

static void check_defaults(const CountTuning &t) {
    CHECK(t.level_bits.empty());
    CHECK(!t.level_bits_set);
    CHECK(t.leaf_target_or(16384.0) == 16384.0);
    CHECK(t.leaf_target_or(6144.0) == 6144.0);
    CHECK(!t.heavy_set);
    CHECK(t.presplit(true) == 8000u);            // record leaves
    CHECK(t.presplit(false) == 0u);              // k-mer and pair leaves
    CHECK(t.wide_presplit(true) == 2600u);       // finish_wide_records
    CHECK(t.wide_presplit(false) == 0u);         // finish_wide
    CHECK(t.sk_desc);
    CHECK(t.sk_onesweep == 1);
    CHECK(t.sk_onesweep_cap == 100);
    CHECK(t.rec_onesweep(0) == 1 && t.rec_onesweep(3) == 1);                                   // the super-k-mer records
    CHECK(t.rec_onesweep(1) == 0 && t.rec_onesweep(2) == 0 && t.rec_onesweep(4) == 0 && t.rec_onesweep(5) == 0);
    CHECK(t.l2_onesweep);
    CHECK(t.l2_squeeze == 100);
    CHECK(t.wide_records);
    CHECK(!t.trace);
    CHECK(!sweep_level1(t, ((int64_t)1 << 22) - 1));
    CHECK(sweep_level1(t, (int64_t)1 << 22));
    for (int k : {33, 47, 63}) CHECK(wide_records_enabled(t, k));
    CHECK(!wide_records_enabled(t, 32) && !wide_records_enabled(t, 64));
}

int main() {
    typedef std::vector<int> V;
    clear_env();
    check_defaults(count_tuning());

    // RFX_LEVEL_BITS: entries outside 0..MAX_BITS are dropped; nothing valid left -> the plan (empty), but "set" is remembered
    {
        CountTuning t = with("RFX_LEVEL_BITS", "9,10");
        CHECK(t.level_bits == (V{9, 10}) && t.level_bits_set);
        t = with("RFX_LEVEL_BITS", "4,3,3");
        CHECK(t.level_bits == (V{4, 3, 3}) && t.level_bits_set);
        t = with("RFX_LEVEL_BITS", "9,,1");              // the empty entry reads as 0
        CHECK(t.level_bits == (V{9, 0, 1}) && t.level_bits_set);
        t = with("RFX_LEVEL_BITS", "11");                // out of range: the plan is used
        CHECK(t.level_bits.empty() && t.level_bits_set);
        t = with("RFX_LEVEL_BITS", "x");                 // atoi("x") = 0 is a valid width
        CHECK(t.level_bits == (V{0}) && t.level_bits_set);
        t = with("RFX_LEVEL_BITS", "");
        CHECK(t.level_bits.empty() && t.level_bits_set);
        t = with("RFX_LEVEL_BITS", "9,11,-1,10");
        CHECK(t.level_bits == (V{9, 10}));
    }
    // RFX_LEAF_TARGET: <= 0 is ignored
    {
        CountTuning t = with("RFX_LEAF_TARGET", "-5");
        CHECK(t.leaf_target_or(16384.0) == 16384.0);
        t = with("RFX_LEAF_TARGET", "0");
        CHECK(t.leaf_target_or(2048.0) == 2048.0);
        t = with("RFX_LEAF_TARGET", "4096");
        CHECK(t.leaf_target_or(16384.0) == 4096.0);
        t = with("RFX_LEAF_TARGET", "1500.5");
        CHECK(t.leaf_target_or(16384.0) == 1500.5);
    }
    // RFX_HEAVY: all three fields, all non-zero, or nothing
    {
        CountTuning t = with("RFX_HEAVY", "40,16,64");
        CHECK(t.heavy_set && t.heavy == 40 && t.heavy_slice == 16 && t.heavy_pcap == 64);
        for (const char *bad : {"40,16", "0,1,1", "a", "", "40,16,0"}) {
            t = with("RFX_HEAVY", bad);
            CHECK(!t.heavy_set);
        }
    }
    // RFX_SK_ONESWEEP against the size gate
    {
        const int64_t below = ((int64_t)1 << 22) - 1, at = (int64_t)1 << 22;
        CountTuning t = with("RFX_SK_ONESWEEP", "0");
        CHECK(t.sk_onesweep == 0 && !sweep_level1(t, below) && !sweep_level1(t, at));
        t = with("RFX_SK_ONESWEEP", "1");
        CHECK(t.sk_onesweep == 1 && !sweep_level1(t, below) && sweep_level1(t, at));
        t = with("RFX_SK_ONESWEEP", "2");
        CHECK(t.sk_onesweep == 2 && sweep_level1(t, below) && sweep_level1(t, at) && sweep_level1(t, 1));
    }
    // the clamped percentages
    {
        CountTuning t = with("RFX_SK_ONESWEEP_CAP", "0");
        CHECK(t.sk_onesweep_cap == 1);
        t = with("RFX_SK_ONESWEEP_CAP", "35");
        CHECK(t.sk_onesweep_cap == 35);
        t = with("RFX_L2_SQUEEZE", "85");
        CHECK(t.l2_squeeze == 85);
        t = with("RFX_L2_SQUEEZE", "-3");
        CHECK(t.l2_squeeze == 1);
    }
    // the pre-split thresholds: the variable wins over both callers' defaults
    {
        CountTuning t = with("RFX_PRESPLIT", "300");
        CHECK(t.presplit(true) == 300u && t.presplit(false) == 300u && t.wide_presplit(true) == 2600u);
        t = with("RFX_PRESPLIT", "0");
        CHECK(t.presplit(true) == 0u && t.presplit(false) == 0u);
        t = with("RFX_WIDE_PRESPLIT", "700");
        CHECK(t.wide_presplit(true) == 700u && t.wide_presplit(false) == 700u && t.presplit(true) == 8000u);
    }
    // RFX_REC_ONESWEEP: set, it holds for every element kind
    {
        for (int v : {0, 1, 2}) {
            const CountTuning t = with("RFX_REC_ONESWEEP", std::to_string(v).c_str());
            for (int mode = 0; mode <= 5; mode++) CHECK(t.rec_onesweep(mode) == v);
        }
    }
    // switches that are off only at "0" (atoi == 0)
    {
        CountTuning t = with("RFX_SK_DESC", "0");
        CHECK(!t.sk_desc);
        t = with("RFX_SK_DESC", "1");
        CHECK(t.sk_desc);
        t = with("RFX_L2_ONESWEEP", "0");
        CHECK(!t.l2_onesweep);
        t = with("RFX_L2_ONESWEEP", "1");
        CHECK(t.l2_onesweep);
    }
    // RFX_WIDE_RECORDS: unset and 1 take the records at k = 33..63, 0 the element path
    {
        clear_env();
        for (int k : {33, 47, 63}) CHECK(wide_records_enabled(count_tuning(), k));
        CountTuning t = with("RFX_WIDE_RECORDS", "0");
        for (int k : {33, 47, 63}) CHECK(!wide_records_enabled(t, k));
        t = with("RFX_WIDE_RECORDS", "1");
        for (int k : {33, 47, 63}) CHECK(wide_records_enabled(t, k));
        CHECK(!wide_records_enabled(t, 31) && !wide_records_enabled(t, 65));
    }
    // RFX_TRACE: set to anything
    {
        CHECK(with("RFX_TRACE", "1").trace);
        CHECK(with("RFX_TRACE", "0").trace);
        CHECK(with("RFX_TRACE", "").trace);
    }
    // nothing is cached: with every variable set and then unset again, the defaults are back
    {
        clear_env();
        setenv("RFX_LEVEL_BITS", "9,10", 1); setenv("RFX_LEAF_TARGET", "100", 1); setenv("RFX_HEAVY", "40,16,64", 1);
        setenv("RFX_PRESPLIT", "1", 1); setenv("RFX_WIDE_PRESPLIT", "1", 1); setenv("RFX_SK_DESC", "0", 1);
        setenv("RFX_SK_ONESWEEP", "2", 1); setenv("RFX_SK_ONESWEEP_CAP", "5", 1); setenv("RFX_REC_ONESWEEP", "2", 1);
        setenv("RFX_L2_ONESWEEP", "0", 1); setenv("RFX_L2_SQUEEZE", "85", 1); setenv("RFX_WIDE_RECORDS", "0", 1);
        setenv("RFX_TRACE", "1", 1);
        const CountTuning t = count_tuning();
        CHECK(t.level_bits == (V{9, 10}) && t.leaf_target_or(1.0) == 100.0 && t.heavy_set && t.presplit(true) == 1u &&
              t.wide_presplit(true) == 1u && !t.sk_desc && t.sk_onesweep == 2 && t.sk_onesweep_cap == 5 && t.rec_onesweep(1) == 2 &&
              !t.l2_onesweep && t.l2_squeeze == 85 && !t.wide_records && t.trace);
        clear_env();
        check_defaults(count_tuning());
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
