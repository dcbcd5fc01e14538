// Drives reflexiv_amd/csrc/host/HostText.h on the cases of tests/test_host_text_host.py: the file named on the command line holds one
// case a line, "op <TAB> argument ...", every text argument in hex; one result line a case goes to stdout, fields between tabs, texts
// escaped (\n \r \t \0 \\).  The cases and what they must give are stated there.
#include <stdio.h>

#include <algorithm>
#include <fstream>
#include <iostream>

#include "HostText.h"

using namespace reflexiv;

static std::string unhex(const std::string &h) {
    std::string s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
    return s;
}

static std::string esc(const std::string &s) {
    std::string o;
    for (char c : s) o += c == '\n' ? "\\n" : c == '\r' ? "\\r" : c == '\t' ? "\\t" : c == '\0' ? "\\0" : c == '\\' ? "\\\\" : std::string(1, c);
    return o;
}

static std::string joined(const std::vector<int64_t> &v) {
    std::string o;
    for (size_t i = 0; i < v.size(); i++) o += (i ? "," : "") + std::to_string(v[i]);
    return o;
}

static std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> f(1);
    for (char c : s) if (c == sep) f.emplace_back(); else f.back().push_back(c);
    return f;
}

static std::string showRows(const Rows &r) { return "rows\t" + joined(r.off) + "\t" + std::to_string(r.n()) + "\t" + esc(r.text); }

// grow <sizes a,b> <replies "status:len:len/status:len:len/...">: the buffers start full of 'x'; call i answers with reply i (the last
// one again after it): the lengths stored, and under status 0 buffer j filled with 'a' + j up to its length.  Every call notes what it
// found in the buffers.
static std::string grow(const std::string &sizes, const std::string &replies) {
    std::vector<std::string> bufs;
    for (const std::string &s : split(sizes, ',')) bufs.emplace_back((size_t)std::stoi(s), 'x');
    std::vector<int64_t> lens(bufs.size(), 0);
    const std::vector<std::string> rep = split(replies, '/');
    std::string seen;
    int calls = 0;
    auto call = [&] {
        const std::vector<std::string> f = split(rep[std::min<size_t>((size_t)calls, rep.size() - 1)], ':');
        calls++;
        const int st = std::stoi(f[0]);
        for (size_t j = 0; j < bufs.size(); j++) {
            seen += (j ? "," : (calls > 1 ? "/" : "")) + esc(bufs[j]);
            lens[j] = std::stoi(f[j + 1]);
            if (st == 0 && lens[j] > (int64_t)bufs[j].size()) throw std::runtime_error("the call was given a buffer shorter than it had asked for");
            if (st == 0) std::fill(bufs[j].begin(), bufs[j].begin() + lens[j], (char)('a' + j));
        }
        return st;
    };
    const int st = bufs.size() == 1 ? growCall({{bufs[0], lens[0]}}, call) : growCall({{bufs[0], lens[0]}, {bufs[1], lens[1]}}, call);
    std::string o = "grow\t" + std::to_string(st) + "\t" + std::to_string(calls) + "\t" + seen + "\t";
    for (size_t j = 0; j < bufs.size(); j++) o += (j ? "," : "") + esc(bufs[j]);
    return o;
}

static std::string one(const std::vector<std::string> &f) {
    const std::string &op = f[0];
    if (op == "lines") {
        const std::string text = unhex(f[1]);
        std::string o = "lines";
        forEachLine(text, [&](size_t pos, size_t len) { o += "\t" + esc(text.substr(pos, len)); });
        return o;
    }
    if (op == "rows") return showRows(f.size() > 2 ? rowsOf(unhex(f[1]), std::stoi(f[2]), f[3].c_str()) : rowsOf(unhex(f[1])));
    if (op == "sam") return showRows(samRows(unhex(f[1])));
    if (op == "count") {
        const KmerCount c = countRow(unhex(f[1]), std::stoi(f[2]));
        return "count\t" + c.kmer + "\t" + std::to_string(c.count);
    }
    if (op == "klist") {
        std::vector<int64_t> ks;
        for (int k : kmerListOf(unhex(f[1]))) ks.push_back(k);
        return "klist\t" + joined(ks);
    }
    if (op == "lastk") return "lastk\t" + std::to_string(lastKmerOf(unhex(f[1])));
    if (op == "fastq" || op == "seq") {
        std::vector<uint8_t> bases(3, 'Z');                        // (the filters clear what they are given)
        std::vector<int64_t> off(2, 7);
        if (op == "fastq") fastqFilterWithQual(unhex(f[1]), bases, off);
        else dsFastqFilterOnlySeq(unhex(f[1]), bases, off);
        return "reads\t" + joined(off) + "\t" + esc(std::string(bases.begin(), bases.end()));
    }
    if (op == "grow") return grow(f[1], f[2]);
    throw std::logic_error("no such op: " + op);
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    for (std::string line; std::getline(in, line);) {
        try {
            std::cout << one(split(line, '\t')) << "\n";
        } catch (const std::invalid_argument &) {
            std::cout << "invalid_argument\n";
        } catch (const std::runtime_error &e) {
            std::cout << "error\t" << esc(e.what()) << "\n";
        }
    }
    std::cout << "ok\n";
    return 0;
}
