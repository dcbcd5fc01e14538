"""The pure text steps of the host driver and its capacity retry (reflexiv_amd/csrc/host/HostText.h) as HOST code:
tests/host_text_main.cpp drives the header on the cases below, compiled with the host compiler under -fsanitize=address,undefined
and run once as a child process.  Nothing is loaded into Python, and no GPU is needed.

What a case must give is written out by hand; the line scans are also held to a few-line statement of their rule in Python
(split at "\\n", no line behind a final newline, one trailing "\\r" dropped; the row scans skip the lines that are then empty)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, "..", "reflexiv_amd", "csrc", "host")
A20, A21 = "A" * 20, "A" * 21
NUL = "\\0"

# the smallest texts that can go wrong: empty, no final newline, \r\n ends, a line that is only \r, blank lines between rows, two \r
SCANS = ["", "a,b", "a,b\n", "a,b\r\nc,d\r\n", "\r", "\n", "a,1\n\n\r\nb,2\n", "a\r\r\nb", "\n\na,b"]

# (stage, commas a row needs, text, the whole message): a row one comma short for each stage string in use
REFUSALS = [
    ("dynamic-k", 1, "ACGT,1|2|3\nACGT\n", "dynamic-k row: ACGT"),
    ("dynamic-k", 2, "ACG,1|2|3,TT\nACG,1|2|3\n", "dynamic-k row: ACG,1|2|3"),
    ("fixing", 2, "ACG,1|2|3,TT\r\nACG,TT\r\n", "fixing row: ACG,TT"),
    ("extend", 1, ">c,ACGT\n\nACGT\nTTTT\n", "extend row: ACGT"),          # (the first such row)
    ("extend2", 2, "ACG,1|2|3,TT\nACG,1|2|3\n", "extend2 row: ACG,1|2|3"),
    ("fixing2", 2, "ACG,1|2|3,TT\nACG,1|2|3", "fixing2 row: ACG,1|2|3"),
]

# countRow at -kmer 5: both row forms; counts of 9, 10 and 11 characters in each form (the ")" is one of them); no comma; a base short
COUNTS = [
    ("ACGTA,7", "count\tACGTA\t7"),
    ("(ACGTA,7)", "count\tACGTA\t7"),
    ("ACGTAC,12", "count\tACGTAC\t12"),
    ("ACGTA,123456789", "count\tACGTA\t123456789"),
    ("ACGTA,1234567890", "count\tACGTA\t1000000000"),
    ("ACGTA,12345678901", "count\tACGTA\t1000000000"),
    ("(ACGTA,12345678)", "count\tACGTA\t12345678"),
    ("(ACGTA,123456789)", "count\tACGTA\t123456789"),
    ("(ACGTA,1234567890)", "count\tACGTA\t1000000000"),
    ("ACGTA", "error\tk-mer count row without a comma: ACGTA"),
    ("ACGT,3", "error\tk-mer shorter than -kmer: ACGT"),
    ("(ACGT,3)", "error\tk-mer shorter than -kmer: ACGT"),
    ("ACGTA,x", "invalid_argument"),
]

KLISTS = [("31", "klist\t31", "lastk\t31"), ("23,31,41", "klist\t23,31,41", "lastk\t41"), ("x,31", "invalid_argument", "lastk\t31")]

# the alignment rows: a four-column row, an 11-field line, an @ line with 10 tabs, a * line, a short @ line (fewer than 10 tabs: any other line)
SAM = ("c1\t5\t10M\tACGT\n" "r1\t0\tc2\t7\t60\t4M\t*\t0\t0\tGGCC\tIIII\r\n" "@HD\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10\n"
       "r2\t4\t*\t0\t0\t*\t*\t0\t0\tTTTT\tIIII\n" "\n" "@short\theader\n")
SAM_ROWS = ["c1\t5\t10M\tACGT", "c2\t7\t4M\tGGCC", "@short\theader"]

# FastqFilterWithQual: (text, the reads)
FASTQ = [
    ("@r1\nACGT\n+\n@III\n@r2\nGGCC\n+\nIIII\n", ["ACGT", "GGCC"]),      # a quality line that begins with @ is no header
    ("@r1\nACGT\n\nIIII\n@r2\nGG\n+\nII", ["ACGT", "GG"]),              # a blank line in the + line's place: the machine advances on it
    ("@r1\n\nACGT\n+\nIIII\n", [""]),                                   # a blank line in the sequence's place is the (empty) sequence
    ("@r1\r\nACGT\r\n+\r\nIIII\r\n@r2\r\nGG\r\n+\r\n", ["ACGT"]),        # \r\n ends; a record without its last line is not emitted
    ("", []),
]
# DSFastqFilterOnlySeq: a sequence line has more than 20 characters and A C G T N at 0, 4, 9, 14, 19
SEQ = [
    ("\n".join(["@" + A21, A20, "+" + A21, A21, "AAAAX" + "A" * 16, "NCGTNACGTNACGTNACGTNA", A21.lower(), ""]), [A21, "NCGTNACGTNACGTNACGTNA"]),
    (A20 + "\r\n" + A21 + "\r\n" + "C" * 30, [A21, "C" * 30]),
    ("", []),
]

# the retry under a fake call: (sizes, replies "status:length..."/..., status, calls, what each call found, the buffers behind it)
GROW = [
    ("8", "0:5", 0, 1, "xxxxxxxx", "aaaaa"),                                                       # success at once
    ("4", "-2:10/0:10", 0, 2, "xxxx/" + NUL * 10, "a" * 10),                                        # one growth
    ("4,16", "-2:9:6/0:9:6", 0, 2, "xxxx," + "x" * 16 + "/" + NUL * 9 + "," + "x" * 16, "a" * 9 + "," + "b" * 6),   # one of two short: the other untouched
    ("16,4", "-2:6:9/0:6:9", 0, 2, "x" * 16 + ",xxxx/" + "x" * 16 + "," + NUL * 9, "a" * 6 + "," + "b" * 9),
    ("4,4", "-2:9:6/0:9:6", 0, 2, "xxxx,xxxx/" + NUL * 9 + "," + NUL * 6, "a" * 9 + "," + "b" * 6),   # both short
    ("8", "-2:8", -2, 1, "xxxxxxxx", "xxxxxxxx"),                                                   # RFX_E_CAP, no length above its buffer: no loop
    ("8,8", "-2:3:8", -2, 1, "xxxxxxxx,xxxxxxxx", "xxxxxxxx,xxxxxxxx"),
    ("8", "-3:99", -3, 1, "xxxxxxxx", "xxxxxxxx"),                                                  # another failure: nothing grows
    ("2", "-2:5/-2:9/0:9", 0, 3, "xx/" + NUL * 5 + "/" + NUL * 9, "a" * 9),                          # a second growth
    ("2", "-2:5/-3:5", -3, 2, "xx/" + NUL * 5, NUL * 5),                                            # a failure behind a growth
]


def esc(s):
    return s.replace("\\", "\\\\").replace("\n", "\\n").replace("\r", "\\r").replace("\t", "\\t")


def model_lines(text):
    parts = text.split("\n")
    if parts[-1] == "":
        parts.pop()
    return [p[:-1] if p.endswith("\r") else p for p in parts]


def offsets(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r))
    return ",".join(map(str, off))


def rows_line(rows):
    return "rows\t%s\t%d\t%s" % (offsets(rows), len(rows), esc("".join(rows)))


def reads_line(reads):
    return "reads\t%s\t%s" % (offsets(reads), "".join(reads))


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("host_text")
    exe, script = str(tmp / "host_text"), str(tmp / "cases.txt")
    # (the sanitizer runtimes linked into the program itself: it depends on no load order)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or os.path.basename(cxx) == "c++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I" + HOST,
                    os.path.join(HERE, "host_text_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    hx = lambda s: s.encode().hex()
    cases = [("lines", hx(t)) for t in SCANS] + [("rows", hx(t)) for t in SCANS]
    cases += [("rows", hx(t), str(n), stage) for stage, n, t, _ in REFUSALS]
    cases += [("rows", hx("a,b\nc,d,e\n"), "1", "extend"), ("rows", hx("a,b\nc,d,e\n"), "2", "extend")]
    cases += [("count", hx(t), "5") for t, _ in COUNTS]
    cases += [(op, hx(t)) for t, _, _ in KLISTS for op in ("klist", "lastk")]
    cases += [("sam", hx(SAM)), ("sam", hx(""))]
    cases += [("fastq", hx(t)) for t, _ in FASTQ] + [("seq", hx(t)) for t, _ in SEQ]
    cases += [("grow", sizes, replies) for sizes, replies, *_ in GROW]
    with open(script, "w") as f:
        f.write("".join("\t".join(c) + "\n" for c in cases))
    r = subprocess.run([exe, script], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.split("\n")
    assert got[len(cases):] == ["ok", ""] and len(got) == len(cases) + 2
    return dict(zip(cases, got))


def test_the_line_scan_and_the_row_scan_on_the_smallest_texts(answers):
    hx = lambda s: s.encode().hex()
    for t in SCANS:
        lines = model_lines(t)
        assert answers[("lines", hx(t))] == "lines" + "".join("\t" + esc(x) for x in lines), repr(t)
        assert answers[("rows", hx(t))] == rows_line([x for x in lines if x]), repr(t)
    # by hand
    assert answers[("lines", hx(""))] == "lines" and answers[("rows", hx(""))] == "rows\t0\t0\t"
    assert answers[("lines", hx("\r"))] == "lines\t" and answers[("rows", hx("\r"))] == "rows\t0\t0\t"
    assert answers[("rows", hx("a,b"))] == "rows\t0,3\t1\ta,b"
    assert answers[("rows", hx("a,b\r\nc,d\r\n"))] == "rows\t0,3,6\t2\ta,bc,d"
    assert answers[("lines", hx("a,1\n\n\r\nb,2\n"))] == "lines\ta,1\t\t\tb,2"
    assert answers[("rows", hx("a,1\n\n\r\nb,2\n"))] == "rows\t0,3,6\t2\ta,1b,2"
    assert answers[("rows", hx("a\r\r\nb"))] == "rows\t0,2,3\t2\ta\\rb"               # one \r is dropped, not two


def test_a_row_one_comma_short_is_refused_with_the_stage_s_message(answers):
    hx = lambda s: s.encode().hex()
    for stage, n, t, message in REFUSALS:
        assert answers[("rows", hx(t), str(n), stage)] == "error\t" + message, stage
    assert answers[("rows", hx("a,b\nc,d,e\n"), "1", "extend")] == "rows\t0,3,8\t2\ta,bc,d,e"
    assert answers[("rows", hx("a,b\nc,d,e\n"), "2", "extend")] == "error\textend row: a,b"


def test_count_rows_in_both_forms_saturate_at_ten_digits(answers):
    for t, want in COUNTS:
        assert answers[("count", t.encode().hex(), "5")] == want, t


def test_the_k_list_and_its_last_entry(answers):
    for t, every, last in KLISTS:
        assert answers[("klist", t.encode().hex())] == every and answers[("lastk", t.encode().hex())] == last, t


def test_the_sam_projection(answers):
    assert answers[("sam", SAM.encode().hex())] == rows_line(SAM_ROWS) == "rows\t0,13,25,38\t3\t" + esc("".join(SAM_ROWS))
    assert answers[("sam", "")] == "rows\t0\t0\t"


def test_the_two_fastq_filters(answers):
    for t, reads in FASTQ:
        assert answers[("fastq", t.encode().hex())] == reads_line(reads), repr(t)
    for t, reads in SEQ:
        assert answers[("seq", t.encode().hex())] == reads_line(reads), repr(t)
    assert answers[("fastq", FASTQ[0][0].encode().hex())] == "reads\t0,4,8\tACGTGGCC"
    assert answers[("fastq", FASTQ[2][0].encode().hex())] == "reads\t0,0\t"
    assert answers[("seq", SEQ[1][0].encode().hex())] == "reads\t0,21,51\t" + A21 + "C" * 30


def test_the_retry_grows_the_short_buffers_alone_and_never_loops_on_a_refusal(answers):
    for sizes, replies, status, calls, seen, left in GROW:
        assert answers[("grow", sizes, replies)] == "grow\t%d\t%d\t%s\t%s" % (status, calls, seen, left), (sizes, replies)
