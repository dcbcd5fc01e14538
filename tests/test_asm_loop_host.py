"""The loop rule of the fixed-k extend driver (reflexiv_amd/csrc/rfx_asm_loop.h) as HOST code: tests/asm_loop_main.cpp drives the
header through an enumeration and writes, after every step, the decision and the whole state; the same enumeration runs here
through a model of the rule written from the reference's lines (P/ReflexivMain.java:232-296 for k <= 31,
P/ReflexivDSMain64.java:581-661 for k > 31 -- as tests/pymodel.py's assemble / assemble_w have it inline), and every record
must be equal.  Compiled with the host compiler under -fsanitize=address,undefined and run as a child process.  Needs no GPU.

The enumeration: both widths; coalesce 0 and 1; min_iter in {0, 1, 3, 4, 15} and max_iter in {0, 2, 5, 20} (values below the 4
iterations the passes before the loop have used included); partition_number pn in {1, 15, 16, 17, 64} with the count alphabet
{21 pn - 1, 21 pn, 0}: the two sides of `current / pn <= 20`, and the contig number a fresh driver starts with (at max_iter = 20
every pn only where the coalesce rule can act, k <= 31 with coalesce on; pn = 64 elsewhere).  Starting states: fresh (the five
passes before the loop run first), and resumed with scramble 3, a contig number out of the alphabet and 0..5 passes done.  From a
state with `room` head calls left before max_iter closes the loop, every count sequence over the alphabet is walked as a tree
when room <= 7 -- always at max_iter <= 5, and at max_iter = 20 from the state resumed with five passes done, which starts at
iteration 14 so that three checks lie ahead.  The other states at max_iter = 20 have 17 calls left; 3^17 sequences are out of
reach, so the first 3 and the last 4 calls (two checks among them) take every value and the calls between take counts that
fall by one (no repeat).  The walk goes one call past a stop by max_iter."""
import os
import shutil
import subprocess
from collections import Counter

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "reflexiv_amd", "csrc")
FILL = 1000000


class Loop:
    __slots__ = ("iterations", "contig_number", "scramble", "P", "partition_number", "passes_done", "nt", "flipped")

    def __init__(self, pn):
        self.iterations, self.contig_number, self.scramble = 0, 0, 2
        self.P = self.partition_number = pn
        self.passes_done = self.nt = 0
        self.flipped = False       # (not part of a record: this walk has seen the scramble step)

    def copy(self):
        t = Loop(0)
        for f in Loop.__slots__:
            setattr(t, f, getattr(self, f))
        return t

    def line(self, decision):
        return "%d %d %d %d %d %d %d %d" % (decision, self.iterations, self.contig_number, self.scramble, self.P,
                                            self.partition_number, self.passes_done, self.nt)


def before(s):
    """:221-254: the pass before the first sort, three with iterations 1..3, the first-array pass with iterations 4"""
    if s.passes_done >= 5:
        return -1
    if s.passes_done >= 1:
        s.iterations += 1          # :234, :249
    return 0 if s.passes_done < 4 else 1


def head(s, wide, coalesce, min_iter, max_iter, current, taken):
    """One turn of `while (iterations <= maximumIteration)`: 0 for a break, else the marker the pass starts with."""
    if not s.iterations <= max_iter:                                   # :265 / 64 :581
        taken["max_iter exhausted"] += 1
        return 0
    s.iterations += 1                                                  # :266 / 64 :582
    if not wide:
        if s.iterations >= min_iter and s.iterations % 3 == 0:         # :267-268
            if s.contig_number == current:                             # :271
                taken["stop"] += 1
                return 0                                               # :272
            s.contig_number = current                                  # :274
            if coalesce:
                if s.partition_number >= 16:                           # :277
                    if current // s.partition_number <= 20:            # :278
                        s.partition_number = s.partition_number // 4 + 1           # :279
                        s.P = s.partition_number                       # :280
                        taken["coalesce taken"] += 1
                    else:
                        taken["coalesce refused by the quotient"] += 1
                else:
                    taken["coalesce refused by < 16"] += 1
        return 2
    if s.iterations >= min_iter + 3 and s.iterations % 3 == 0:         # 64 :621-622
        if s.contig_number == current:                                 # 64 :639
            if s.scramble == 2:                                        # 64 :640
                s.scramble = 3                                         # 64 :641
                s.flipped = True
                taken["scramble step"] += 1
            else:
                taken["second repeat" if s.flipped else "stop"] += 1
                return 0                                               # 64 :644
        else:
            s.contig_number = current                                  # 64 :647
        # 64 :650-656 changes a partition number that no pass reads
    return 1 if s.scramble == 3 else 2                                 # the passes of :660-661 / :666-668 under param.scramble


def model_records(taken):
    out = []

    def walk(s, rule, alphabet, pos, room, head_free, tail_free):
        free = pos < room and (pos < head_free or pos >= room - tail_free)
        for current in (alphabet if free else (FILL - pos,)):
            t = s.copy()
            d = head(t, *rule, current, taken)
            if d:
                t.passes_done += 1
                t.nt += 1
            out.append(t.line(d))
            if d and pos <= rule[3] + 2:
                walk(t, rule, alphabet, pos + 1, room, head_free, tail_free)

    for wide in (0, 1):
        for coalesce in (0, 1):
            for min_iter in (0, 1, 3, 4, 15):
                for max_iter in (0, 2, 5, 20):
                    for pn in (1, 15, 16, 17, 64):
                        if max_iter == 20 and not (coalesce and not wide) and pn != 64:
                            continue
                        rule = (wide, coalesce, min_iter, max_iter)
                        alphabet = (21 * pn - 1, 21 * pn, 0)
                        for start in range(-1, 6):
                            out.append("C %d %d %d %d %d %d" % (wide, coalesce, min_iter, max_iter, pn, start))
                            s = Loop(pn)
                            if start >= 0:
                                s.scramble = 3
                                s.passes_done = s.nt = start
                                s.iterations = max(start - 1, 0) if start < 5 else max(max_iter - 6, 4)
                                s.contig_number = alphabet[start % 3]
                            while True:
                                stage = before(s)
                                if stage < 0:
                                    break
                                s.passes_done += 1
                                s.nt += 1
                                out.append(s.line(stage))
                            room = max(max_iter + 1 - s.iterations, 0)
                            walk(s, rule, alphabet, 0, room, room if room <= 7 else 3, 0 if room <= 7 else 4)
    return out


def test_the_loop_rule_equals_the_model_on_every_record_under_the_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    assert os.path.exists(os.path.join(CSRC, "rfx_asm_loop.h"))
    exe, log = str(tmp_path / "asm_loop"), str(tmp_path / "records.txt")
    # (the sanitizer runtimes linked into the program itself: it depends on no load order)
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) or os.path.basename(cxx) == "c++" else ["-static-libsan"]
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static, "-I" + CSRC,
                    os.path.join(HERE, "asm_loop_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe, log], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ok" in r.stdout
    taken = Counter()
    want = model_records(taken)
    with open(log) as f:
        got = f.read().splitlines()
    assert len(got) == len(want)
    config = None
    for i, (g, w) in enumerate(zip(got, want)):
        if w[0] == "C":
            config = w
        assert g == w, "record %d of configuration %r: the header gives %r, the model %r" % (i, config, g, w)
    for branch in ("stop", "scramble step", "second repeat", "coalesce taken", "coalesce refused by < 16",
                   "coalesce refused by the quotient", "max_iter exhausted"):
        assert taken[branch] > 0, branch
