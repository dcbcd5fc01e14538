// reflexiv_cli.cpp -- `reflexiv_host run|counter -fastq F [-kmer K -cover C ...] -outfile O`,
// `reflexiv_host sort -kmerc COUNTS -kmer K [-klist 23,31,...] -outfile O` (Count_<K>_sorted), `firstfour`, `iteration`,
// `reflexiv_host mercy -kmerc O/Count_<K> -fastq F[,F2...] -kmer K [-clipf N -clipe N] -outfile O` (Count_<K>_mercy; `sort -kmerc
// O/Count_<K>,O/Count_<K>_mercy` then reads both, in the order Spark lists them),
// `reflexiv_host reduce -kmerc SHORT -kmerc2 LONG -kmer K1 -kmer2 K2 [-klist ...] -partition P -outfile O` (Count_<K1>_reduced and
// Count_<K2>_sorted, or Count_<K2>_reduced when K2 is the last k of the list), `reflexiv_host reduce -fastq F -klist ... -partition P
// -outfile O [-sensitive]` (Count_<k>_reduced of every k from the reads in one run), `reflexiv_host reduce -kmerc DIR -klist ... -partition P
// -outfile O` (DIR/Count_<k> of every k of the list: each through `sort`, then the pairs in the list's order),
// `reflexiv_host fixing -kmerc ITERATION_OUT [-klist ...] -partition P -outfile O` (O/Assembly_intermediate/04Fixing),
// `reflexiv_host fixing2 -kmerc O/Assembly_intermediate/04Fixing [-klist ...] -partition P -outfile O` (05FixingAgain and 06ContigEnds),
// `reflexiv_host endextend -kmerc O/Assembly_intermediate/05FixingAgain -sam ROWS [-klist ...] -outfile O` (07EndExtend),
// `reflexiv_host mapping -kmerc O/Assembly_intermediate/05FixingAgain -fastq F[,F2...] [-klist ...] -outfile O [-rowsout FILE]` (the whole
// Mapping stage: the library's own end-overhang mapper in the aligner's place, then the end extension -> 07EndExtend),
// `reflexiv_host extend -kmerc O/Assembly_intermediate/07EndExtend [-klist ...] -partition P [-maxiter M] -outfile O` (08Extend),
// `reflexiv_host extend2 -kmerc O/Assembly_intermediate/08Extend [-klist ...] -partition P [-maxiter M] -outfile O` (09ExtendAgain),
// `reflexiv_host meta -fastq F[,F2...] -klist K1,K2,... -partition P -outfile O [-sensitive] [-intermediate]` (reads to contigs in one
// resident run: O/Assembly; with -intermediate every file of O/Assembly_intermediate/ under the reference's names too, one run a stage),
// `reflexiv_host dedup -kmerc O/Assembly_intermediate/09ExtendAgain -outfile O [-mincontig N]` (the last stage alone: O/Assembly)
// the two launcher sub-commands of bin/reflexiv:252-271 that reach the hot path
// (M/Main.java:59-79, M/MainOfCounter.java:60-80), on one MI355X instead of spark-submit.
#include <zlib.h>

#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <sys/stat.h>
#include <dirent.h>
#include <cstring>
#include <algorithm>

#include "ReflexivMain.h"

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

int main(int argc, char **argv) {
    try {
        if (argc < 2) { std::cerr << "usage: reflexiv_host <run|counter|sort|firstfour|iteration> -fastq F[,F2...] -outfile DIR [-kmer 31 -cover 2 ...]\n"
                                   "       reflexiv_host sort -kmerc COUNTS[,MERCY] -kmer K [-klist 23,31,41,53,67,81,95] -outfile DIR\n"
                                   "       reflexiv_host mercy -kmerc COUNTS -fastq F[,F2...] -kmer K [-clipf N -clipe N] -outfile DIR\n"
                                   "       reflexiv_host reduce -kmerc SHORT -kmerc2 LONG -kmer K1 -kmer2 K2 [-klist ...] -partition P -outfile DIR\n"
                                   "       reflexiv_host reduce -kmerc COUNTS_DIR -klist K1,K2,... -partition P -outfile DIR\n"
                                   "       reflexiv_host reduce -fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive]\n"
                                   "       reflexiv_host fixing -kmerc ITERATION_OUT [-klist 23,31,...,95] -partition P -outfile DIR\n"
                                   "       reflexiv_host fixing2 -kmerc FIXING_OUT [-klist 23,31,...,95] -partition P -outfile DIR\n"
                                   "       reflexiv_host endextend -kmerc FIXING_AGAIN_OUT -sam ROWS [-klist 23,31,...,95] -outfile DIR\n"
                                   "       reflexiv_host mapping -kmerc FIXING_AGAIN_OUT -fastq F[,F2...] [-klist 23,31,...,95] -outfile DIR [-rowsout FILE]\n"
                                   "       reflexiv_host extend -kmerc END_EXTEND_OUT [-klist 23,31,...,95] -partition P -outfile DIR\n"
                                   "       reflexiv_host extend2 -kmerc EXTEND_OUT [-klist 23,31,...,95] -partition P -outfile DIR\n"
                                   "       reflexiv_host meta -fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive] [-intermediate]\n"
                                   "       reflexiv_host dedup -kmerc EXTEND_AGAIN_OUT -outfile DIR [-mincontig N]\n"; return 2; }
        std::string cmd = argv[1];
        std::vector<std::string> args(argv + 2, argv + argc);
        reflexiv::DefaultParam param = reflexiv::importCommandLine(args);
        if (cmd == "sort" && (param.inputKmerPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("sort needs -kmerc COUNTS -kmer K [-klist 23,31,...] -outfile DIR");
        if (cmd == "sort" && (param.kmerSize < 8 || (param.kmerSize - 1) % 31 == 0))
            throw std::runtime_error("sort: -kmer " + std::to_string(param.kmerSize) + " is not supported (8..124 except 32, 63, 94)");
        if (cmd == "mercy" && (param.inputKmerPath.empty() || param.inputFqPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("mercy needs -kmerc COUNTS -fastq F[,F2...] -kmer K [-clipf N -clipe N] -outfile DIR");
        if (cmd == "mercy" && (param.kmerSize < 8 || param.kmerSize > 31))
            throw std::runtime_error("mercy: -kmer " + std::to_string(param.kmerSize) + " is not supported (8..31)");
        if (cmd == "reduce" && !param.inputFqPath.empty() && param.inputKmerPath.empty() && param.outputPath.empty())
            throw std::runtime_error("reduce needs -fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive]");
        if (cmd == "reduce" && param.inputFqPath.empty() && (param.inputKmerPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("reduce needs -kmerc SHORT -kmerc2 LONG -kmer K1 -kmer2 K2 [-klist ...] -partition P -outfile DIR, or -kmerc COUNTS_DIR "
                                     "-klist K1,K2,... -partition P -outfile DIR");
        if (cmd == "reduce" && !param.inputKmerPath2.empty() && (param.kmerSize < 8 || param.kmerSize >= param.kmerSize2 || param.kmerSize2 > 124))
            throw std::runtime_error("reduce: the pair -kmer " + std::to_string(param.kmerSize) + " -kmer2 " + std::to_string(param.kmerSize2) +
                                     " is not supported (8 <= k1 < k2 <= 124)");
        if (cmd == "fixing" && (param.inputKmerPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("fixing needs -kmerc ITERATION_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR");
        if (cmd == "fixing2" && (param.inputKmerPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("fixing2 needs -kmerc FIXING_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR");
        if (cmd == "endextend" && (param.inputKmerPath.empty() || param.inputSamPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("endextend needs -kmerc FIXING_AGAIN_OUT -sam ROWS [-klist 23,31,...] -outfile DIR");
        if (cmd == "mapping" && (param.inputKmerPath.empty() || param.inputFqPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("mapping needs -kmerc FIXING_AGAIN_OUT -fastq F[,F2...] [-klist 23,31,...] -outfile DIR [-rowsout FILE]");
        if (cmd == "extend" && (param.inputKmerPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("extend needs -kmerc END_EXTEND_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR");
        if (cmd == "extend2" && (param.inputKmerPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("extend2 needs -kmerc EXTEND_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR");
        if (cmd == "meta" && (param.inputFqPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("meta needs -fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive] [-intermediate]");
        if (cmd == "dedup" && (param.inputKmerPath.empty() || param.outputPath.empty()))
            throw std::runtime_error("dedup needs -kmerc EXTEND_AGAIN_OUT -outfile DIR [-mincontig N]");
        if (param.outputPath.empty()) throw std::runtime_error("-outfile is required");
        if (param.inputFqPath.empty() && param.inputKmerPath.empty()) throw std::runtime_error("-fastq or -kmerc is required");
        auto read_all = [&](const std::string &paths) {
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
        };
        reflexiv::ReflexivMain m;
        m.setParam(param);
        std::string out, dir = param.outputPath;
        mkdir(dir.c_str(), 0755);
        if (cmd == "run") {
            // M/Main.java:74-78 -> Pipelines.reflexivDSMainPipe(): -kmerc routes to assemblyFromKmer()
            // k > 31: Pipelines.reflexivDSMainPipe64() -> ReflexivDSMain64.assemblyFromKmer(), output under Assemble_<k>
            // (P/ReflexivDSMain64.java:820-824); only the from-counts route exists for k > 31 -- and --resident,
            // which is that route (`counter`, then `run -kmerc`) fused into one call on the device (k = 33..100, not 64 or 96)
            if (param.kmerSize > 31) {
                if (param.inputKmerPath.empty() && !param.resident)
                    throw std::runtime_error("-kmer > 31 needs -kmerc (counter -> run -kmerc; the reference's run -fastq is inconsistent for k > 31)");
                out = !param.inputKmerPath.empty() ? m.assemblyFromKmer64(read_all(param.inputKmerPath))
                      : (param.gpus > 1 || getenv("RFX_HOST_FORCE_SHARDED")) ? m.assemblyResidentSharded(read_all(param.inputFqPath), param.gpus)
                                                                             : m.assemblyResident(read_all(param.inputFqPath));
                dir += "/Assemble_" + std::to_string(param.kmerSize);
                mkdir(dir.c_str(), 0755);
            } else
            out = !param.inputKmerPath.empty() ? m.assemblyFromKmer(read_all(param.inputKmerPath))
                  : param.resident && (param.gpus > 1 || getenv("RFX_HOST_FORCE_SHARDED")) ? m.assemblyResidentSharded(read_all(param.inputFqPath), param.gpus)
                  : param.resident          ? m.assemblyResident(read_all(param.inputFqPath))
                                            : m.assembly(read_all(param.inputFqPath));
            if (param.dedup) out = m.dedupContigText(out);
        } else if (cmd == "sort") {
            // Pipelines.reflexivLeftAndRightSortingPipe(): rows "KMER,count" -> Count_<k>_sorted
            // (P/ReflexivDSKmerLeftAndRightSorting.java:228-240)
            out = m.kmerSorting(read_all(param.inputKmerPath));
            dir += "/Count_" + std::to_string(param.kmerSize) + "_sorted"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "mercy") {
            // Pipelines.java:1385-1391 (-sensitive, behind the counter for every k <= 31): the rows "KMER,count" of Count_<k> and the reads
            // -> Count_<k>_mercy (P/ReflexivDSDynamicMercyKmer.java:307-318), which the sorter reads through the glob Count_<k>*/part*
            out = m.mercyKmers(read_all(param.inputKmerPath), read_all(param.inputFqPath));
            dir += "/Count_" + std::to_string(param.kmerSize) + "_mercy"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "reduce") {
            // Pipelines.reflexivDSDynamicKmerReductionPipe() (Pipelines.java:1343-1365 walks the pairs of the k list); the second output
            // is Count_<k2>_reduced when k2 is the last k of the list, Count_<k2>_sorted otherwise (P/ReflexivDSDynamicKmerRuduction.java:257-283)
            const int P = param.partitions > 0 ? param.partitions : param.logicalPartitions;
            if (P < 1 || P > 63) throw std::runtime_error("reduce: -partition must be 1..63");
            auto write = [&](const std::string &name, const std::string &text) {
                const std::string d = param.outputPath + "/" + name;
                mkdir(d.c_str(), 0755);
                std::ofstream(d + "/part-00000.csv", std::ios::binary) << text;
                std::ofstream(d + "/_SUCCESS", std::ios::binary);
            };
            auto pair = [&](const std::string &s, const std::string &l, int k1, int k2) {
                if (k1 < 8 || k1 >= k2 || k2 > 124) throw std::runtime_error("reduce: the pair " + std::to_string(k1) + ", " + std::to_string(k2) + " is not supported (8 <= k1 < k2 <= 124)");
                std::string o1, o2;
                m.kmerReduction(s, l, k1, k2, P, &o1, &o2);
                write("Count_" + std::to_string(k1) + "_reduced", o1);
                write("Count_" + std::to_string(k2) + (k2 == m.lastKmerOfList() ? "_reduced" : "_sorted"), o2);
                return o2;
            };
            if (!param.inputFqPath.empty() && param.inputKmerPath.empty()) {
                // Pipelines.reflexivDSDynamicReductionPipe() from the reads in one run: Count_<k>_reduced of every k of the list
                std::vector<int> ks;
                std::stringstream ss(param.kmerList);
                for (std::string one; std::getline(ss, one, ',');) ks.push_back(std::stoi(one));
                const std::vector<std::string> texts = m.kmerReductionFromReads(read_all(param.inputFqPath), ks, P);
                for (size_t i = 0; i < ks.size(); i++) write("Count_" + std::to_string(ks[i]) + "_reduced", texts[i]);
            } else if (!param.inputKmerPath2.empty()) {
                pair(read_all(param.inputKmerPath), read_all(param.inputKmerPath2), param.kmerSize, param.kmerSize2);
            } else {
                std::vector<int> ks;
                std::stringstream ss(param.kmerList);
                for (std::string one; std::getline(ss, one, ',');) ks.push_back(std::stoi(one));
                if (ks.size() < 2) throw std::runtime_error("reduce: -klist needs two k at least");
                auto sorted = [&](int k) {
                    if (k < 8 || k > 124 || (k - 1) % 31 == 0) throw std::runtime_error("reduce: the sorting stage does not support k = " + std::to_string(k));
                    m.param.setKmerSize(k);
                    return m.kmerSorting(read_all(param.inputKmerPath + "/Count_" + std::to_string(k)));
                };
                std::string cur = sorted(ks[0]);
                for (size_t i = 1; i < ks.size(); i++) cur = pair(cur, sorted(ks[i]), ks[i - 1], ks[i]);
            }
            return 0;
        } else if (cmd == "firstfour") {
            // Pipelines.reflexivDSDynamicKmerFirstFourPipe(): rows "KMER,marker|left|right" of the reduction -> 00firstFour
            out = m.assemblyDynamicFirstFour(read_all(param.inputKmerPath));
            dir += "/Assembly_intermediate"; mkdir(dir.c_str(), 0755);
            dir += "/00firstFour"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "iteration") {
            // Pipelines.reflexivDSDynamicKmerIterationPipe(): -> 01Iteration<start>_<end>
            out = m.assemblyDynamicIteration(read_all(param.inputKmerPath), param.startIteration, param.endIteration);
            dir += "/Assembly_intermediate"; mkdir(dir.c_str(), 0755);
            dir += "/01Iteration" + std::to_string(param.startIteration) + "_" + std::to_string(param.endIteration); mkdir(dir.c_str(), 0755);
        } else if (cmd == "fixing") {
            // Pipelines.reflexivDSDynamicAssemblyStepsPipe() behind the last iteration (Pipelines.java:840-1291): the rows of
            // 01Iteration<start>_<end> -> 04Fixing; maxKmerSize is the last k of the list
            const int P = param.partitions > 0 ? param.partitions : param.logicalPartitions;
            if (P < 1 || P > 63) throw std::runtime_error("fixing: -partition must be 1..63");
            if (m.lastKmerOfList() < 31 || m.lastKmerOfList() > 124) throw std::runtime_error("fixing: the last k of -klist must be 31..124");
            out = m.contigFixing(read_all(param.inputKmerPath), P);
            dir += "/Assembly_intermediate"; mkdir(dir.c_str(), 0755);
            dir += "/04Fixing"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "fixing2") {
            // the step behind it (Pipelines.java:840-1291): the rows of 04Fixing -> 05FixingAgain (rows "ID,contig") and 06ContigEnds (the
            // FASTA of contig ends an aligner reads); maxKmerSize is the last k of the list
            const int P = param.partitions > 0 ? param.partitions : param.logicalPartitions;
            if (P < 1 || P > 63) throw std::runtime_error("fixing2: -partition must be 1..63");
            if (m.lastKmerOfList() < 31 || m.lastKmerOfList() > 124) throw std::runtime_error("fixing2: the last k of -klist must be 31..124");
            std::string contigRows, contigEnds;
            m.contigFixingRoundTwo(read_all(param.inputKmerPath), P, &contigRows, &contigEnds);
            dir += "/Assembly_intermediate"; mkdir(dir.c_str(), 0755);
            for (int f = 0; f < 2; f++) {
                const std::string d = dir + (f ? "/06ContigEnds" : "/05FixingAgain");
                mkdir(d.c_str(), 0755);
                std::ofstream(d + (f ? "/part-00000" : "/part-00000.csv"), std::ios::binary) << (f ? contigEnds : contigRows);
                std::ofstream(d + "/_SUCCESS", std::ios::binary);
            }
            return 0;
        } else if (cmd == "endextend") {
            // Pipelines.java:1065-1085 behind the aligner: the rows of 05FixingAgain and the alignment rows (contig, start, cigar, seq -- or
            // full SAM lines) -> 07EndExtend; maxKmerSize is the last k of the list
            if (m.lastKmerOfList() < 31 || m.lastKmerOfList() > 124) throw std::runtime_error("endextend: the last k of -klist must be 31..124");
            out = m.contigEndExtend(read_all(param.inputKmerPath), read_all(param.inputSamPath));
            dir += "/Assembly_intermediate"; mkdir(dir.c_str(), 0755);
            dir += "/07EndExtend"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "mapping") {
            // the whole Mapping stage (Pipelines.java:1065-1085) with no program outside this one: the rows of 05FixingAgain and the reads ->
            // the library's end-overhang mapper -> the end extension -> 07EndExtend; maxKmerSize is the last k of the list
            if (m.lastKmerOfList() < 31 || m.lastKmerOfList() > 124) throw std::runtime_error("mapping: the last k of -klist must be 31..124");
            std::string rows;
            out = m.contigMapping(read_all(param.inputKmerPath), read_all(param.inputFqPath), &rows);
            if (!param.rowsOutPath.empty()) std::ofstream(param.rowsOutPath, std::ios::binary) << rows;
            dir += "/Assembly_intermediate"; mkdir(dir.c_str(), 0755);
            dir += "/07EndExtend"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "extend" || cmd == "extend2") {
            // the two steps behind it (Pipelines.java:840-1291): the rows of 07EndExtend -> 08Extend, the rows of 08Extend -> 09ExtendAgain,
            // which the de-duplication reads; maxKmerSize is the last k of the list
            const int P = param.partitions > 0 ? param.partitions : param.logicalPartitions;
            if (P < 1 || P > 63) throw std::runtime_error(cmd + ": -partition must be 1..63");
            if (m.lastKmerOfList() < 31 || m.lastKmerOfList() > 124) throw std::runtime_error(cmd + ": the last k of -klist must be 31..124");
            out = cmd == "extend" ? m.contigExtend(read_all(param.inputKmerPath), P) : m.contigExtendAgain(read_all(param.inputKmerPath), P);
            dir += "/Assembly_intermediate"; mkdir(dir.c_str(), 0755);
            dir += cmd == "extend" ? "/08Extend" : "/09ExtendAgain"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "meta") {
            // Pipelines.reflexivDSDynamicReductionPipe + reflexivDSDynamicAssemblyStepsPipe (Pipelines.java:1315-1737, :840-1291) in one
            // resident run; the partition rule of the later stages is the library's (rfx_meta.hip)
            const int P = param.partitions > 0 ? param.partitions : param.logicalPartitions;
            if (P < 1 || P > 63) throw std::runtime_error("meta: -partition must be 1..63");
            std::vector<int> ks;
            std::stringstream ss(param.kmerList);
            for (std::string one; std::getline(ss, one, ',');) ks.push_back(std::stoi(one));
            const std::string fastq = read_all(param.inputFqPath);
            if (param.intermediate) {
                static const char *const NAMES[RFX_META_ASSEMBLY] = {"00firstFour", "01Iteration5_9", "01Iteration10_14", "01Iteration15_19", "01Iteration21_30",
                    "01Iteration31_40", "01Iteration41_50", "01Iteration51_60", "01Iteration61_70", "04Fixing", "05FixingAgain", "06ContigEnds", "Mapping",
                    "07EndExtend", "08Extend", "09ExtendAgain"};
                const std::string ai = dir + "/Assembly_intermediate";
                mkdir(ai.c_str(), 0755);
                for (int s = RFX_META_FIRST_FOUR; s < RFX_META_ASSEMBLY; s++) {
                    const std::string d = ai + "/" + NAMES[s];
                    mkdir(d.c_str(), 0755);
                    // (06ContigEnds is a FASTA and the mapper's rows are a table: neither is a csv)
                    std::ofstream(d + (s == RFX_META_CONTIG_ENDS ? "/part-00000" : s == RFX_META_MAPPING ? "/part-00000.tsv" : "/part-00000.csv"), std::ios::binary)
                        << m.metaAssemblyFromReads(fastq, ks, P, s);
                    std::ofstream(d + "/_SUCCESS", std::ios::binary);
                }
            }
            out = m.metaAssemblyFromReads(fastq, ks, P, RFX_META_ASSEMBLY);
            dir += "/Assembly"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "dedup") {
            // Pipelines.java:1230-1290: the rows of 09ExtendAgain -> Assembly
            out = m.dedupContigRows(read_all(param.inputKmerPath));
            dir += "/Assembly"; mkdir(dir.c_str(), 0755);
        } else if (cmd == "counter") {
            // --resident at k = 33..100 (not 64 or 96): the same rows through the device count of the packed reads
            out = param.resident && param.kmerSize >= 33 && param.kmerSize % 32 != 0 ? m.counterResident(read_all(param.inputFqPath))
                                                                                   : m.counter(read_all(param.inputFqPath));
            dir += "/Count_" + std::to_string(param.kmerSize);               // P/ReflexivDataFrameCounter.java:222-233
            mkdir(dir.c_str(), 0755);
        } else throw std::runtime_error("unknown command " + cmd);
        std::ofstream(dir + (cmd == "counter" || cmd == "sort" || cmd == "mercy" || cmd == "firstfour" || cmd == "iteration" || cmd == "fixing" || cmd == "endextend" || cmd == "mapping" || cmd == "extend" || cmd == "extend2" ? "/part-00000.csv" : "/part-00000"), std::ios::binary) << out;   // saveAsTextFile / csv
        std::ofstream(dir + "/_SUCCESS", std::ios::binary);
        return 0;
    } catch (const std::exception &e) {
        std::cerr << "reflexiv_host: " << e.what() << "\n";
        return 1;
    }
}
