"""Writes tests/golden/meta_vectors.npz: the read sets of tests/meta_model.py and, for each, every stage's text of the whole call from
reads to contigs as the independent model gives it (tests/meta_model.py: the models of every stage joined, each handing the next its
text, under the orchestrator's partition rule), the counts of the report and the facts test_meta_model.py asserts.  Run from the
repository root: python tests/golden/make_meta_vectors.py.  tests/test_meta_model.py regenerates the arrays and compares."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import meta_model as MM      # noqa: E402

if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "meta_vectors.npz")
    np.savez_compressed(out, **MM.build_vectors())
    print(out, os.path.getsize(out), "bytes")
