"""The argument errors of `reflexiv_host` that the binary before the command table raised with a context in hand (so on a machine with a GPU
only), and that the table checks before it creates one: the -partition range and the last k of -klist.  The whole lines are those of that
binary, recorded from it on an MI355X on these argument vectors.  `-partition 0` is no error: it is "not given", the run goes on with
--logical-partitions and ends at the input that does not exist."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISSING = "/nonexistent/rows"
INPUTS = {
    "fixing": ["-kmerc", MISSING], "fixing2": ["-kmerc", MISSING], "extend": ["-kmerc", MISSING], "extend2": ["-kmerc", MISSING],
    "endextend": ["-kmerc", MISSING, "-sam", MISSING], "mapping": ["-kmerc", MISSING, "-fastq", MISSING],
    "reduce": ["-kmerc", MISSING, "-kmerc2", MISSING, "-kmer", "31", "-kmer2", "41"], "meta": ["-fastq", MISSING, "-klist", "23,31"],
}
CASES = [(cmd, ["-partition", p], line) for cmd in ("fixing", "fixing2", "extend", "extend2", "reduce", "meta")
         for p, line in (("0", "cannot open " + MISSING), ("64", cmd + ": -partition must be 1..63"))]
CASES += [(cmd, ["-klist", ks], cmd + ": the last k of -klist must be 31..124") for cmd in ("fixing", "fixing2", "endextend", "mapping", "extend", "extend2")
          for ks in ("23,30", "23,125")]


@pytest.mark.gpu
@pytest.mark.parametrize("cmd,flags,line", CASES, ids=[" ".join([c] + f) for c, f, _ in CASES])
def test_reflexiv_host_refuses_the_argument_with_the_line_it_had(tmp_path, cmd, flags, line):
    exe = os.path.join(ROOT, "reflexiv_amd", "reflexiv_host")
    r = subprocess.run([exe, cmd] + INPUTS[cmd] + flags + ["-outfile", str(tmp_path / "out")], capture_output=True, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (1, "", "reflexiv_host: " + line + "\n")
