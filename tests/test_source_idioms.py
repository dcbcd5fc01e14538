"""The host code in reflexiv_amd/csrc launches kernels through RFX_LAUNCH / RFX_LAUNCH_N (rfx_internal.h: on the context's
stream, checked) and nowhere else, has no launch-shape helper of its own, and passes `x.as<T>()` to a `const T *` parameter
without a cast; the views of a packed contig set and the arrays of an int32 block are made by the named
makers of rfx_internal.h and nowhere else (section 27).  Text only: nothing is compiled, nothing else is checked."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reflexiv_amd", "csrc")
SUFFIXES = (".hip", ".h", ".cpp", ".hpp", ".c")


def sources():
    out = []
    for base, _, names in os.walk(CSRC):
        out += [os.path.join(base, n) for n in sorted(names) if n.endswith(SUFFIXES)]
    return sorted(out)


def hits(pattern, skip=()):
    found = []
    for path in sources():
        if os.path.basename(path) in skip:
            continue
        for no, line in enumerate(open(path, encoding="utf-8", errors="replace"), 1):
            if re.search(pattern, line):
                found.append(f"{os.path.relpath(path, CSRC)}:{no}: {line.strip()[:120]}")
    return found


def test_sources_found():
    assert any(p.endswith("rfx_internal.h") for p in sources()) and len(sources()) > 15


@pytest.mark.parametrize("pattern, skip", [
    (r"hipLaunchKernelGGL|<<<", ("rfx_internal.h",)),                    # a launch outside the two macros
    (r"\bgrid_for\s*\(|#\s*define\s+RFX_GRID\b|\bRFX_GRID\s*\(", ()),      # a launch-shape helper beside RFX_LAUNCH_N
    (r"\(\s*const\s+([^()*]+?)\s*\*\s*\)\s*[\w.\[\]>-]+\.as<\s*\1\s*>\(\)", ()),  # (const X *)y.as<X>()
    # a kernel-facing view of a packed contig set written out as a list of pointers, as a temporary or as a variable (DESIGN.md
    # section 27: the named makers in rfx_internal.h write them); `X{}` and `X v{}` stay legal, and so does MpHitsIn
    (r"\b(Fx2View|EeSetIn|EeSetOut|EeConsIn|EeConsOut|MpHits)\b(\s+\w+)?\s*\{\s*[^}\s]", ("rfx_internal.h",)),
    (r"\+\s*\d+\s*\*\s*[a-z]1\b", ("rfx_internal.h",)),                   # `a + 2 * m1`: the arrays of one int32 block carved by hand
], ids=["raw_launch", "launch_shape_helper", "const_cast_of_as", "contig_view_as_a_pointer_list", "int32_block_carved_by_hand"])
def test_idiom_absent(pattern, skip):
    found = hits(pattern, skip)
    assert not found, "\n".join(found)
