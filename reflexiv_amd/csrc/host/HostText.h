// HostText.h -- the pure text steps of the host driver, and the capacity retry every text call of the library goes through.
// Plain C++17: neither HIP nor reflexiv_hip.h, so a stand-alone program drives it (tests/host_text_main.cpp).
#pragma once
#include <cstdint>
#include <initializer_list>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace reflexiv {

// The line scan: split at '\n', one trailing '\r' dropped, the last line needs no newline.  f(pos, len) sees every line, the empty
// ones too: the row scans skip those, the FASTQ filters do not.
template <class F> void forEachLine(const std::string &text, F &&f) {
    for (size_t pos = 0; pos < text.size();) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        f(pos, e - pos - (e > pos && text[e - 1] == '\r' ? 1 : 0));
        pos = e + 1;
    }
}

// the non-empty lines back to back, and their offsets
struct Rows {
    std::string text;
    std::vector<int64_t> off{0};
    int64_t n() const { return (int64_t)off.size() - 1; }
    std::string row(int64_t i) const { return text.substr((size_t)off[(size_t)i], (size_t)(off[(size_t)i + 1] - off[(size_t)i])); }
};

// minCommas: what a row must hold to be one of the stage's; stage: the word that a refused row's message begins with
inline Rows rowsOf(const std::string &text, int minCommas = 0, const char *stage = "") {
    Rows r;
    forEachLine(text, [&](size_t pos, size_t len) {
        if (!len) return;
        int commas = 0;
        for (size_t i = pos; i < pos + len; i++) commas += text[i] == ',';
        if (commas < minCommas) throw std::runtime_error(std::string(stage) + " row: " + text.substr(pos, len));
        r.text.append(text, pos, len);
        r.off.push_back((int64_t)r.text.size());
    });
    return r;
}

// FastqFilterWithQual.call + FastqUnitFilter.call  P/ReflexivMain.java:3080-3113: the 4-line state machine; emits the sequence
// line of every completed record.
inline void fastqFilterWithQual(const std::string &text, std::vector<uint8_t> &bases, std::vector<int64_t> &readOff) {
    int lineMark = 0;
    size_t seqOff = 0, seqLen = 0;
    bases.clear(); readOff.assign(1, 0);
    forEachLine(text, [&](size_t pos, size_t l) {
        if (lineMark == 2) lineMark++;                                  // :3093-3096
        else if (lineMark == 3) {                                       // :3097-3100
            lineMark++;
            bases.insert(bases.end(), text.begin() + seqOff, text.begin() + seqOff + seqLen);
            readOff.push_back((int64_t)bases.size());
        } else if (l > 0 && text[pos] == '@') lineMark = 1;             // :3101-3104
        else if (lineMark == 1) { seqOff = pos; seqLen = l; lineMark++; }   // :3105-3108
    });
}

// DSFastqFilterOnlySeq.call  P/ReflexivDataFrameCounter.java:238-290 (the counter's line filter)
inline void dsFastqFilterOnlySeq(const std::string &text, std::vector<uint8_t> &bases, std::vector<int64_t> &readOff) {
    auto checkSeq = [](char a) { return a == 'A' || a == 'T' || a == 'C' || a == 'G' || a == 'N'; };   // :268-289
    bases.clear(); readOff.assign(1, 0);
    forEachLine(text, [&](size_t pos, size_t l) {
        const char *s = text.data() + pos;
        if (l > 20 && s[0] != '@' && s[0] != '+' && checkSeq(s[0]) && checkSeq(s[4]) && checkSeq(s[9]) &&
            checkSeq(s[14]) && checkSeq(s[19])) {                      // :245-262
            bases.insert(bases.end(), s, s + l);
            readOff.push_back((int64_t)bases.size());
        }
    });
}

// KmerBinarizer.call  P/ReflexivDSMain.java:3883-3931 and P/ReflexivDSMain64.java:10772-10836: one row "KMER,count" or
// "(KMER,count)" of at least k bases; a count of ten or more digits saturates at 1,000,000,000.  The callers pack the bases.
struct KmerCount { std::string kmer; int count; };
inline KmerCount countRow(const std::string &line, int k) {
    const size_t comma = line.find(',');
    if (comma == std::string::npos) throw std::runtime_error("k-mer count row without a comma: " + line);
    std::string kmer = line.substr(0, comma), cnt = line.substr(comma + 1);
    if (!kmer.empty() && kmer[0] == '(') kmer = kmer.substr(1);                        // :3892-3894
    int cover;
    if (!cnt.empty() && cnt.back() == ')') cover = cnt.size() >= 11 ? 1000000000 : std::stoi(cnt.substr(0, cnt.size() - 1));   // :3896-3901
    else cover = cnt.size() >= 10 ? 1000000000 : std::stoi(cnt);                       // :3902-3908
    if ((int)kmer.size() < k) throw std::runtime_error("k-mer shorter than -kmer: " + kmer);
    return {kmer, cover};
}
inline unsigned baseCode(char c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : 3u; }   // :3912-3919

// -klist: every entry, and the last one alone (param.kmerListInt[length - 1]; the entries before it are not read, so "x,31" is 31)
inline std::vector<int> kmerListOf(const std::string &list) {
    std::vector<int> ks;
    std::stringstream ss(list);
    for (std::string one; std::getline(ss, one, ',');) ks.push_back(std::stoi(one));
    return ks;
}
inline int lastKmerOf(const std::string &list) {
    const size_t c = list.rfind(',');
    return std::stoi(list.substr(c == std::string::npos ? 0 : c + 1));
}

// The alignment rows of the end extension: "contig \t start \t cigar \t seq" passes through; a line of 10 tabs or more is a full
// SAM line: header and `*` lines are skipped, fields 3, 4, 6 and 10 taken (the commented awk of P/ReflexivDSDynamicKmerMapping.java:1189).
inline Rows samRows(const std::string &samText) {
    const Rows lines = rowsOf(samText);
    Rows r;
    for (int64_t i = 0; i < lines.n(); i++) {
        const std::string line = lines.row(i);
        std::vector<size_t> tabs;
        for (size_t p = 0; p < line.size(); p++) if (line[p] == '\t') tabs.push_back(p);
        if (tabs.size() >= 10) {
            auto field = [&](size_t f) { return line.substr(tabs[f - 1] + 1, tabs[f] - tabs[f - 1] - 1); };
            if (line[0] == '@' || field(2) == "*") continue;
            r.text += field(2) + "\t" + field(3) + "\t" + field(5) + "\t" + field(9);
        } else {
            r.text += line;
        }
        r.off.push_back((int64_t)r.text.size());
    }
    return r;
}

// The capacity retry.  call() makes the library call with every buffer's data() and size() and returns its status, having stored
// the length each buffer needs in its len.  On RFX_E_CAP the buffers whose length exceeds them grow to it -- those alone -- and the
// call is made again; RFX_E_CAP with no such buffer is an error, not a loop.  RFX_OK resizes every buffer to its length.  Returns
// the last status; the caller words the failure.
constexpr int GROW_OK = 0, GROW_E_CAP = -2;                   // RFX_OK, RFX_E_CAP (ReflexivMain.cpp holds them equal)
struct GrowBuf { std::string &buf; int64_t &len; };
template <class Call> int growCall(std::initializer_list<GrowBuf> bufs, Call &&call) {
    for (;;) {
        const int st = call();
        bool grew = false;
        if (st == GROW_E_CAP)
            for (const GrowBuf &b : bufs)
                if (b.len > (int64_t)b.buf.size()) { b.buf.assign((size_t)b.len, '\0'); grew = true; }
        if (grew) continue;
        if (st == GROW_OK) for (const GrowBuf &b : bufs) b.buf.resize((size_t)b.len);
        return st;
    }
}

}  // namespace reflexiv
