"""What `reflexiv_host` answers to argument vectors that it refuses before a context is created: the exit status, nothing on stdout and the
whole line on stderr.  Needs no GPU.

The lines are those of the binary before the command table (reflexiv_amd/csrc/host/reflexiv_cli.cpp: one row a command), recorded from it on
these argument vectors, with three exceptions that the table brings, each a synopsis now written once:
  * `reduce` without its inputs names all three of its forms (it named the two -kmerc forms, or with -fastq alone the third);
  * the usage text is the table's synopses joined: `run`, `counter`, `firstfour` and `iteration` have a line each, and the -klist of every
    line reads as in the "needs" messages;
  * an unknown command with -outfile and an input is refused as such before the context is created, not behind it (same words)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REDUCE = ("reduce needs -kmerc SHORT -kmerc2 LONG -kmer K1 -kmer2 K2 [-klist ...] -partition P -outfile DIR, or -kmerc COUNTS_DIR -klist K1,K2,... "
          "-partition P -outfile DIR, or -fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive]")
SORT = "sort needs -kmerc COUNTS -kmer K [-klist 23,31,...] -outfile DIR"
MERCY = "mercy needs -kmerc COUNTS -fastq F[,F2...] -kmer K [-clipf N -clipe N] -outfile DIR"
REFUSED = [
    (["run"], "-outfile is required"),
    (["counter"], "-outfile is required"),
    (["sort"], SORT),
    (["mercy"], MERCY),
    (["reduce"], REDUCE),
    (["firstfour"], "-outfile is required"),
    (["iteration"], "-outfile is required"),
    (["fixing"], "fixing needs -kmerc ITERATION_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR"),
    (["fixing2"], "fixing2 needs -kmerc FIXING_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR"),
    (["endextend"], "endextend needs -kmerc FIXING_AGAIN_OUT -sam ROWS [-klist 23,31,...] -outfile DIR"),
    (["mapping"], "mapping needs -kmerc FIXING_AGAIN_OUT -fastq F[,F2...] [-klist 23,31,...] -outfile DIR [-rowsout FILE]"),
    (["extend"], "extend needs -kmerc END_EXTEND_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR"),
    (["extend2"], "extend2 needs -kmerc EXTEND_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR"),
    (["meta"], "meta needs -fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive] [-intermediate]"),
    (["dedup"], "dedup needs -kmerc EXTEND_AGAIN_OUT -outfile DIR [-mincontig N]"),
    (["sort", "-kmer", "32"], SORT),
    (["mercy", "-kmer", "32"], MERCY),
    (["reduce", "-kmer", "41", "-kmer2", "31"], REDUCE),
    (["assemble"], "-outfile is required"),                                   # an unknown command
    (["run", "-bogus"], "unknown parameter -bogus"),
    (["run", "-fastq"], "Parameter -fastq needs a value"),
    # with their inputs named (no file is opened before these checks)
    (["reduce", "-fastq", "F"], REDUCE),
    (["run", "-outfile", "/nonexistent/out"], "-fastq or -kmerc is required"),
    (["sort", "-kmerc", "C", "-outfile", "/nonexistent/out", "-kmer", "32"], "sort: -kmer 32 is not supported (8..124 except 32, 63, 94)"),
    (["mercy", "-kmerc", "C", "-fastq", "F", "-outfile", "/nonexistent/out", "-kmer", "32"], "mercy: -kmer 32 is not supported (8..31)"),
    (["reduce", "-kmerc", "S", "-kmerc2", "L", "-kmer", "41", "-kmer2", "31", "-outfile", "/nonexistent/out"],
     "reduce: the pair -kmer 41 -kmer2 31 is not supported (8 <= k1 < k2 <= 124)"),
    (["assemble", "-fastq", "F", "-outfile", "/nonexistent/out"], "unknown command assemble"),
]

USAGE = """usage: reflexiv_host run -fastq F[,F2...] | -kmerc COUNTS -outfile DIR [-kmer 31 -cover 2 ... --resident --gpus N --dedup]
       reflexiv_host counter -fastq F[,F2...] -outfile DIR [-kmer 31 -cover 2 ... --resident]
       reflexiv_host mercy -kmerc COUNTS -fastq F[,F2...] -kmer K [-clipf N -clipe N] -outfile DIR
       reflexiv_host sort -kmerc COUNTS -kmer K [-klist 23,31,...] -outfile DIR
       reflexiv_host reduce -kmerc SHORT -kmerc2 LONG -kmer K1 -kmer2 K2 [-klist ...] -partition P -outfile DIR
       reflexiv_host reduce -kmerc COUNTS_DIR -klist K1,K2,... -partition P -outfile DIR
       reflexiv_host reduce -fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive]
       reflexiv_host firstfour -kmerc REDUCED -outfile DIR [--logical-partitions P]
       reflexiv_host iteration -kmerc ROWS -start S -end E -outfile DIR [--logical-partitions P]
       reflexiv_host fixing -kmerc ITERATION_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR
       reflexiv_host fixing2 -kmerc FIXING_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR
       reflexiv_host endextend -kmerc FIXING_AGAIN_OUT -sam ROWS [-klist 23,31,...] -outfile DIR
       reflexiv_host mapping -kmerc FIXING_AGAIN_OUT -fastq F[,F2...] [-klist 23,31,...] -outfile DIR [-rowsout FILE]
       reflexiv_host extend -kmerc END_EXTEND_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR
       reflexiv_host extend2 -kmerc EXTEND_OUT [-klist 23,31,...] -partition P [-maxiter M -scramble S] -outfile DIR
       reflexiv_host dedup -kmerc EXTEND_AGAIN_OUT -outfile DIR [-mincontig N]
       reflexiv_host meta -fastq F[,F2...] -klist K1,K2,... -partition P -outfile DIR [-sensitive] [-intermediate]
"""


@pytest.fixture(scope="module")
def exe():
    from reflexiv_amd import _lib
    _lib.build()
    path = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    assert os.path.exists(path)
    return path


@pytest.mark.parametrize("args,line", REFUSED, ids=[" ".join(a) for a, _ in REFUSED])
def test_reflexiv_host_refuses_with_status_1_and_the_whole_line(exe, args, line):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "reflexiv_host: " + line + "\n")


def test_reflexiv_host_without_arguments_prints_the_usage_with_status_2(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", USAGE)
