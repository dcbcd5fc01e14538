// reflexiv_cli.cpp -- `reflexiv_host <command> ...`: the launcher sub-commands of bin/reflexiv:252-271 that reach the hot path
// (M/Main.java:59-79, M/MainOfCounter.java:60-80) and the stages of the meta pipeline one by one, on one MI355X instead of spark-submit.
// COMMANDS below holds one row per command: its synopsis, what it requires, where its output goes and what it runs.
#include <zlib.h>

#include <algorithm>
#include <cstring>
#include <dirent.h>
#include <fstream>
#include <iostream>
#include <sys/stat.h>

#include "ReflexivMain.h"

using reflexiv::DefaultParam;
using reflexiv::ReflexivMain;

static std::string slurp(const std::string &path) {
    std::string out;
    gzFile f = gzopen(path.c_str(), "rb");          // reads plain text as well as .gz
    if (!f) throw std::runtime_error("cannot open " + path);
    char buf[1 << 16];
    int n;
    while ((n = gzread(f, buf, sizeof buf)) > 0) out.append(buf, (size_t)n);
    gzclose(f);
    return out;
}

// the text of a comma-separated list of files and Spark output directories
static std::string readAll(const std::string &paths) {
    std::string text;
    std::stringstream ss(paths);
    for (std::string one; std::getline(ss, one, ',');) {
        struct stat st;
        if (stat(one.c_str(), &st) == 0 && S_ISDIR(st.st_mode)) {      // a Spark output directory: every part-*
            DIR *d = opendir(one.c_str());
            std::vector<std::string> parts;
            for (dirent *e; d && (e = readdir(d));) if (strncmp(e->d_name, "part-", 5) == 0) parts.push_back(one + "/" + e->d_name);
            if (d) closedir(d);
            std::sort(parts.begin(), parts.end());
            for (auto &f : parts) text += slurp(f);
        } else {
            text += slurp(one);
        }
        if (!text.empty() && text.back() != '\n') text.push_back('\n');
    }
    return text;
}

// one run of one command: the driver, the parameters, -partition where the command takes it
struct Run {
    ReflexivMain &m;
    const DefaultParam &param;
    int P;
    std::string kmerc() const { return readAll(param.inputKmerPath); }
    std::string fastq() const { return readAll(param.inputFqPath); }
    // saveAsTextFile / csv: <-outfile>/<dir>/<file> and _SUCCESS beside it; dir may be empty or hold several levels
    void writePart(const std::string &dir, const std::string &file, const std::string &text) const {
        std::string d = param.outputPath;
        for (size_t b = 0, e; b < dir.size(); b = e + 1) {
            e = std::min(dir.find('/', b), dir.size());
            d += "/" + dir.substr(b, e - b);
            mkdir(d.c_str(), 0755);
        }
        std::ofstream(d + "/" + file, std::ios::binary) << text;
        std::ofstream(d + "/_SUCCESS", std::ios::binary);
    }
};

// M/Main.java:74-78 -> Pipelines.reflexivDSMainPipe(): -kmerc routes to assemblyFromKmer()
// k > 31: Pipelines.reflexivDSMainPipe64() -> ReflexivDSMain64.assemblyFromKmer(), output under Assemble_<k>
// (P/ReflexivDSMain64.java:820-824); only the from-counts route exists for k > 31 -- and --resident,
// which is that route (`counter`, then `run -kmerc`) fused into one call on the device (k = 33..100, not 64 or 96)
static std::string run(Run &r) {
    const DefaultParam &p = r.param;
    const bool counts = !p.inputKmerPath.empty(), sharded = p.gpus > 1 || getenv("RFX_HOST_FORCE_SHARDED");
    if (p.kmerSize > 31 && !counts && !p.resident)
        throw std::runtime_error("-kmer > 31 needs -kmerc (counter -> run -kmerc; the reference's run -fastq is inconsistent for k > 31)");
    std::string out = counts ? (p.kmerSize > 31 ? r.m.assemblyFromKmer64(r.kmerc()) : r.m.assemblyFromKmer(r.kmerc()))
                      : p.kmerSize <= 31 && !p.resident ? r.m.assembly(r.fastq())
                      : sharded ? r.m.assemblyResidentSharded(r.fastq(), p.gpus) : r.m.assemblyResident(r.fastq());
    if (p.dedup) out = r.m.dedupContigText(out);
    r.writePart(p.kmerSize > 31 ? "Assemble_" + std::to_string(p.kmerSize) : "", "part-00000", out);
    return "";
}

// Pipelines.reflexivDSDynamicKmerReductionPipe() (Pipelines.java:1343-1365 walks the pairs of the k list); the second output
// is Count_<k2>_reduced when k2 is the last k of the list, Count_<k2>_sorted otherwise (P/ReflexivDSDynamicKmerRuduction.java:257-283)
static std::string reduce(Run &r) {
    const DefaultParam &p = r.param;
    auto write = [&](const std::string &name, const std::string &text) { r.writePart(name, "part-00000.csv", text); };
    auto pair = [&](const std::string &s, const std::string &l, int k1, int k2) {
        if (k1 < 8 || k1 >= k2 || k2 > 124) throw std::runtime_error("reduce: the pair " + std::to_string(k1) + ", " + std::to_string(k2) + " is not supported (8 <= k1 < k2 <= 124)");
        std::string o1, o2;
        r.m.kmerReduction(s, l, k1, k2, r.P, &o1, &o2);
        write("Count_" + std::to_string(k1) + "_reduced", o1);
        write("Count_" + std::to_string(k2) + (k2 == r.m.lastKmerOfList() ? "_reduced" : "_sorted"), o2);
        return o2;
    };
    const bool fromReads = !p.inputFqPath.empty() && p.inputKmerPath.empty();
    if (!fromReads && !p.inputKmerPath2.empty()) {
        pair(r.kmerc(), readAll(p.inputKmerPath2), p.kmerSize, p.kmerSize2);
        return "";
    }
    const std::vector<int> ks = reflexiv::kmerListOf(p.kmerList);
    if (fromReads) {
        // Pipelines.reflexivDSDynamicReductionPipe() from the reads in one run: Count_<k>_reduced of every k of the list
        const std::vector<std::string> texts = r.m.kmerReductionFromReads(r.fastq(), ks, r.P);
        for (size_t i = 0; i < ks.size(); i++) write("Count_" + std::to_string(ks[i]) + "_reduced", texts[i]);
        return "";
    }
    // DIR/Count_<k> of every k of the list: each through `sort`, then the pairs in the list's order
    if (ks.size() < 2) throw std::runtime_error("reduce: -klist needs two k at least");
    auto sorted = [&](int k) {
        if (k < 8 || k > 124 || (k - 1) % 31 == 0) throw std::runtime_error("reduce: the sorting stage does not support k = " + std::to_string(k));
        r.m.param.setKmerSize(k);
        return r.m.kmerSorting(readAll(p.inputKmerPath + "/Count_" + std::to_string(k)));
    };
    std::string cur = sorted(ks[0]);
    for (size_t i = 1; i < ks.size(); i++) cur = pair(cur, sorted(ks[i]), ks[i - 1], ks[i]);
    return "";
}

// the step behind `fixing` (Pipelines.java:840-1291): the rows of 04Fixing -> 05FixingAgain (rows "ID,contig") and 06ContigEnds (the
// FASTA of contig ends an aligner reads)
static std::string fixing2(Run &r) {
    std::string contigRows, contigEnds;
    r.m.contigFixingRoundTwo(r.kmerc(), r.P, &contigRows, &contigEnds);
    r.writePart("Assembly_intermediate/05FixingAgain", "part-00000.csv", contigRows);
    r.writePart("Assembly_intermediate/06ContigEnds", "part-00000", contigEnds);
    return "";
}

// Pipelines.reflexivDSDynamicReductionPipe + reflexivDSDynamicAssemblyStepsPipe (Pipelines.java:1315-1737, :840-1291) in one
// resident run; the partition rule of the later stages is the library's (rfx_meta.hip).  -intermediate: one run a stage
static std::string meta(Run &r) {
    static const char *const NAMES[RFX_META_ASSEMBLY] = {"00firstFour", "01Iteration5_9", "01Iteration10_14", "01Iteration15_19", "01Iteration21_30",
        "01Iteration31_40", "01Iteration41_50", "01Iteration51_60", "01Iteration61_70", "04Fixing", "05FixingAgain", "06ContigEnds", "Mapping",
        "07EndExtend", "08Extend", "09ExtendAgain"};
    const std::vector<int> ks = reflexiv::kmerListOf(r.param.kmerList);
    const std::string fastq = r.fastq();
    for (int s = RFX_META_FIRST_FOUR; r.param.intermediate && s < RFX_META_ASSEMBLY; s++)
        // (06ContigEnds is a FASTA and the mapper's rows are a table: neither is a csv)
        r.writePart(std::string("Assembly_intermediate/") + NAMES[s],
                    s == RFX_META_CONTIG_ENDS ? "part-00000" : s == RFX_META_MAPPING ? "part-00000.tsv" : "part-00000.csv",
                    r.m.metaAssemblyFromReads(fastq, ks, r.P, s));
    return r.m.metaAssemblyFromReads(fastq, ks, r.P, RFX_META_ASSEMBLY);
}

enum : unsigned { FASTQ = 1, KMERC = 2, SAM = 4, EITHER = 8 };   // EITHER: -fastq or -kmerc
struct Command {
    const char *name;
    const char *synopsis;                    // what follows the name; one line per form.  The usage text and "<name> needs ..." are made of these
    unsigned needs;                          // the inputs that must be given, -outfile with them; 0: the two general messages of main()
    bool partition;                          // takes -partition (1..63)
    bool lastK;                              // maxKmerSize is the last k of -klist, which must be 31..124
    const char *dir, *file;                  // where the handler's text goes under -outfile ({k}, {start}, {end}: -kmer, -start, -end)
    std::string (*handler)(Run &);           // dir null: it writes its own files
    void (*check)(const DefaultParam &);     // a further argument check, or null
};
#define AI "Assembly_intermediate/"
static const Command COMMANDS[] = {
    {"run", "-fastq F[,F2...] | -kmerc COUNTS -outfile DIR [-kmer 31 -cover 2 ... --resident --gpus N --dedup]", 0, false, false, nullptr, nullptr, run, nullptr},
    // P/ReflexivCounter.java, rows under Count_<k> (P/ReflexivDataFrameCounter.java:222-233); --resident at k = 33..100 (not 64 or 96): the same
    // rows through the device count of the packed reads
    {"counter", "-fastq F[,F2...] -outfile DIR [-kmer 31 -cover 2 ... --resident]", 0, false, false, "Count_{k}", "part-00000.csv",
     [](Run &r) { return r.param.resident && r.param.kmerSize >= 33 && r.param.kmerSize % 32 != 0 ? r.m.counterResident(r.fastq()) : r.m.counter(r.fastq()); }, nullptr},
    // Pipelines.java:1385-1391 (-sensitive, behind the counter for every k <= 31): the rows "KMER,count" of Count_<k> and the reads
    // -> Count_<k>_mercy (P/ReflexivDSDynamicMercyKmer.java:307-318), which the sorter reads through the glob Count_<k>*/part*
    {"mercy", "-kmerc COUNTS -fastq F[,F2...] -kmer K [-clipf N -clipe N] -outfile DIR", KMERC | FASTQ, false, false, "Count_{k}_mercy", "part-00000.csv",
     [](Run &r) { return r.m.mercyKmers(r.kmerc(), r.fastq()); },
     [](const DefaultParam &p) {
         if (p.kmerSize < 8 || p.kmerSize > 31) throw std::runtime_error("mercy: -kmer " + std::to_string(p.kmerSize) + " is not supported (8..31)");
     }},
    // Pipelines.reflexivLeftAndRightSortingPipe(): rows "KMER,count" -> Count_<k>_sorted (P/ReflexivDSKmerLeftAndRightSorting.java:228-240);
    // `-kmerc O/Count_<K>,O/Count_<K>_mercy` reads both, in the order Spark lists them
    {"sort", "-kmerc COUNTS -kmer K [-klist 23,31,...] -outfile DIR", KMERC, false, false, "Count_{k}_sorted", "part-00000.csv",
     [](Run &r) { return r.m.kmerSorting(r.kmerc()); },
     [](const DefaultParam &p) {
         if (p.kmerSize < 8 || (p.kmerSize - 1) % 31 == 0)
             throw std::runtime_error("sort: -kmer " + std::to_string(p.kmerSize) + " is not supported (8..124 except 32, 63, 94)");
     }},
    {"reduce", "-kmerc SHORT -kmerc2 LONG -kmer K1 -kmer2 K2 [-klist ...] -partition P -outfile DIR\n-kmerc COUNTS_DIR -klist K1,K2,... -partition P -outfile DIR\n"
               "-fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive]", EITHER, true, false, nullptr, nullptr, reduce,
     [](const DefaultParam &p) {
         if (!p.inputKmerPath2.empty() && (p.kmerSize < 8 || p.kmerSize >= p.kmerSize2 || p.kmerSize2 > 124))
             throw std::runtime_error("reduce: the pair -kmer " + std::to_string(p.kmerSize) + " -kmer2 " + std::to_string(p.kmerSize2) +
                                      " is not supported (8 <= k1 < k2 <= 124)");
     }},
    // Pipelines.reflexivDSDynamicKmerFirstFourPipe(): rows "KMER,marker|left|right" of the reduction -> 00firstFour
    {"firstfour", "-kmerc REDUCED -outfile DIR [--logical-partitions P]", 0, false, false, AI "00firstFour", "part-00000.csv",
     [](Run &r) { return r.m.assemblyDynamicFirstFour(r.kmerc()); }, nullptr},
    // Pipelines.reflexivDSDynamicKmerIterationPipe(): -> 01Iteration<start>_<end>
    {"iteration", "-kmerc ROWS -start S -end E -outfile DIR [--logical-partitions P]", 0, false, false, AI "01Iteration{start}_{end}", "part-00000.csv",
     [](Run &r) { return r.m.assemblyDynamicIteration(r.kmerc(), r.param.startIteration, r.param.endIteration); }, nullptr},
    // Pipelines.reflexivDSDynamicAssemblyStepsPipe() behind the last iteration (Pipelines.java:840-1291): the rows of 01Iteration<start>_<end> -> 04Fixing
    {"fixing", "-kmerc ITERATION_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR", KMERC, true, true, AI "04Fixing", "part-00000.csv",
     [](Run &r) { return r.m.contigFixing(r.kmerc(), r.P); }, nullptr},
    {"fixing2", "-kmerc FIXING_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR", KMERC, true, true, nullptr, nullptr, fixing2, nullptr},
    // Pipelines.java:1065-1085 behind the aligner: the rows of 05FixingAgain and the alignment rows (contig, start, cigar, seq -- or full SAM lines) -> 07EndExtend
    {"endextend", "-kmerc FIXING_AGAIN_OUT -sam ROWS [-klist 23,31,...] -outfile DIR", KMERC | SAM, false, true, AI "07EndExtend", "part-00000.csv",
     [](Run &r) { return r.m.contigEndExtend(r.kmerc(), readAll(r.param.inputSamPath)); }, nullptr},
    // the whole Mapping stage (Pipelines.java:1065-1085) with no program outside this one: the rows of 05FixingAgain and the reads ->
    // the library's end-overhang mapper -> the end extension -> 07EndExtend
    {"mapping", "-kmerc FIXING_AGAIN_OUT -fastq F[,F2...] [-klist 23,31,...] -outfile DIR [-rowsout FILE]", KMERC | FASTQ, false, true, AI "07EndExtend", "part-00000.csv",
     [](Run &r) {
         std::string rows, out = r.m.contigMapping(r.kmerc(), r.fastq(), &rows);
         if (!r.param.rowsOutPath.empty()) std::ofstream(r.param.rowsOutPath, std::ios::binary) << rows;
         return out;
     }, nullptr},
    // the two steps behind it (Pipelines.java:840-1291): the rows of 07EndExtend -> 08Extend, the rows of 08Extend -> 09ExtendAgain, which the de-duplication reads
    {"extend", "-kmerc END_EXTEND_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR", KMERC, true, true, AI "08Extend", "part-00000.csv",
     [](Run &r) { return r.m.contigExtend(r.kmerc(), r.P); }, nullptr},
    {"extend2", "-kmerc EXTEND_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR", KMERC, true, true, AI "09ExtendAgain", "part-00000.csv",
     [](Run &r) { return r.m.contigExtendAgain(r.kmerc(), r.P); }, nullptr},
    // Pipelines.java:1230-1290: the rows of 09ExtendAgain -> Assembly
    {"dedup", "-kmerc EXTEND_AGAIN_OUT -outfile DIR [-mincontig N]", KMERC, false, false, "Assembly", "part-00000",
     [](Run &r) { return r.m.dedupContigRows(r.kmerc()); }, nullptr},
    // reads to contigs in one resident run: O/Assembly; with -intermediate every file of O/Assembly_intermediate/ under the reference's names too
    {"meta", "-fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive] [-intermediate]", FASTQ, true, false, "Assembly", "part-00000", meta, nullptr},
};
#undef AI

static std::string replaced(std::string s, const std::string &what, const std::string &with) {
    for (size_t at = 0; (at = s.find(what, at)) != std::string::npos; at += with.size()) s.replace(at, what.size(), with);
    return s;
}

static int partitionsOf(const DefaultParam &param, const std::string &cmd) {
    const int P = param.partitions > 0 ? param.partitions : param.logicalPartitions;
    if (P < 1 || P > 63) throw std::runtime_error(cmd + ": -partition must be 1..63");
    return P;
}

static void requireLastK(const DefaultParam &param, const std::string &cmd) {
    const int k = reflexiv::lastKmerOf(param.kmerList);
    if (k < 31 || k > 124) throw std::runtime_error(cmd + ": the last k of -klist must be 31..124");
}

int main(int argc, char **argv) {
    try {
        if (argc < 2) {
            for (const Command &c : COMMANDS)
                std::cerr << (&c == COMMANDS ? "usage: " : "       ") << "reflexiv_host " << c.name << " "
                          << replaced(c.synopsis, "\n", std::string("\n       reflexiv_host ") + c.name + " ") << "\n";
            return 2;
        }
        const std::string cmd = argv[1];
        const DefaultParam param = reflexiv::importCommandLine(std::vector<std::string>(argv + 2, argv + argc));
        const Command *c = std::find_if(std::begin(COMMANDS), std::end(COMMANDS), [&](const Command &x) { return cmd == x.name; });
        if (c == std::end(COMMANDS)) c = nullptr;
        const bool fastq = !param.inputFqPath.empty(), kmerc = !param.inputKmerPath.empty();
        if (c && c->needs && (param.outputPath.empty() || (c->needs & FASTQ && !fastq) || (c->needs & KMERC && !kmerc) ||
                              (c->needs & SAM && param.inputSamPath.empty()) || (c->needs & EITHER && !fastq && !kmerc)))
            throw std::runtime_error(cmd + " needs " + replaced(c->synopsis, "\n", ", or "));
        if (c && c->check) c->check(param);
        if (param.outputPath.empty()) throw std::runtime_error("-outfile is required");
        if (!fastq && !kmerc) throw std::runtime_error("-fastq or -kmerc is required");
        if (!c) throw std::runtime_error("unknown command " + cmd);
        const int P = c->partition ? partitionsOf(param, cmd) : 0;
        if (c->lastK) requireLastK(param, cmd);
        ReflexivMain m;
        m.setParam(param);
        mkdir(param.outputPath.c_str(), 0755);
        Run r{m, param, P};
        const std::string text = c->handler(r);
        if (c->dir) r.writePart(replaced(replaced(replaced(c->dir, "{k}", std::to_string(param.kmerSize)), "{start}", std::to_string(param.startIteration)),
                                         "{end}", std::to_string(param.endIteration)), c->file, text);
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "reflexiv_host: " << e.what() << "\n";
        return 1;
    }
}
