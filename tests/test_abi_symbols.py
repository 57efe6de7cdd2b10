"""The C ABI's link surface: the `shelfi_*` symbols libshelfi.so exports are exactly the `shelfi_*`
functions include/shelfi.h declares.  An entry point that loses its `extern "C"` (it is then exported
under a mangled name) or whose source file drops out of the link shows up as a declared function that
is not exported; an exported one the header does not declare is an undocumented entry point."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

LIB = os.path.join(ROOT, "fhe-fed_amd", "SHELFI_FHE", "libshelfi.so")
HEADER = os.path.join(ROOT, "include", "shelfi.h")


def _ensure_lib():
    if not os.path.exists(LIB):  # normally built by build() / make
        subprocess.run(["make", "-C", os.path.join(ROOT, "fhe-fed_amd", "csrc"), "../SHELFI_FHE/libshelfi.so"],
                       check=True, capture_output=True, timeout=1800)
    return LIB


def _declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)  # comments name functions too
    src = re.sub(r"//[^\n]*", " ", src)
    # a function declaration: a return type at the start of a line, the name, its parameter list, ';'
    return set(re.findall(r"^[A-Za-z_][\w \t\*]*?\b(shelfi_\w+)\s*\([^;{]*\)\s*;", src, flags=re.M))


def _exported():
    out = subprocess.run(["nm", "-D", "--defined-only", _ensure_lib()], check=True, capture_output=True,
                         text=True, timeout=60).stdout
    names = set()
    for line in out.splitlines():
        parts = line.split()
        if len(parts) == 3 and parts[2].startswith("shelfi_"):
            assert parts[1] == "T", "%s is exported as '%s', not as a function" % (parts[2], parts[1])
            names.add(parts[2])
    return names


@pytest.mark.skipif(shutil.which("nm") is None, reason="nm (binutils) not available")
def test_exported_symbols_match_the_header():
    declared, exported = _declared(), _exported()
    assert len(declared) > 50, "the header's declarations were not parsed"
    assert not declared - exported, "declared, not exported: %s" % sorted(declared - exported)
    assert not exported - declared, "exported, not declared: %s" % sorted(exported - declared)
