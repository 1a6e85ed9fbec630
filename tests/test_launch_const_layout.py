"""The launch block of the lane-per-read kernel (LaunchConst, mapper_amd/csrc/xm_defs.h) is written by the host side of libxmapper_hip.so and read by kernels
compiled in another unit, from the same header.  The product library's host side reports the layout it was compiled with (launchConstLayout); the same
function is compiled here from the header in the tree, the way the host simulation compiles these sources (g++, host build), and the two must agree: a skew
between the library and the header - a stale object, a define that reaches one unit only - fails here, without a GPU."""
import ctypes as C
import os
import subprocess

from mapper_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 10  # XM_LAUNCH_CONST_LAYOUT_WORDS
NAMES = ("sizeof(LaunchConst)", "offsetof ix", "offsetof params", "sizeof(IndexView)", "IndexView::contigStart", "IndexView::lines32", "IndexView::baLogStep",
         "sizeof(Params)", "Params::Max_PenaltySpan", "Params::StartingInsertionStartFree")
PROGRAM = """#include "xm_defs.h"
#include <cstdio>
int main() {
  static_assert(xm::XM_LAUNCH_CONST_LAYOUT_WORDS == %d, "the test's word count");
  int64_t out[xm::XM_LAUNCH_CONST_LAYOUT_WORDS];
  xm::launchConstLayout(out);
  for (int i = 0; i < xm::XM_LAUNCH_CONST_LAYOUT_WORDS; i++) printf("%%lld\\n", (long long)out[i]);
  return 0;
}
""" % WORDS


def library_layout():
    fn = _capi.lib().xm_test_launch_const_layout
    fn.argtypes = [C.POINTER(C.c_int64), C.c_int32]
    fn.restype = C.c_int
    out = (C.c_int64 * WORDS)()
    assert fn(out, WORDS) == WORDS
    assert fn(out, WORDS - 1) == -1, "a buffer too small is refused"
    return dict(zip(NAMES, (int(x) for x in out)))


def header_layout(tmp_path):
    src, exe = str(tmp_path / "layout.cpp"), str(tmp_path / "layout")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "mapper_amd", "csrc"), "-o", exe, src])
    words = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    assert len(words) == WORDS
    return dict(zip(NAMES, words))


def test_launch_const_layout_agrees_between_the_library_and_the_header(tmp_path):
    product = library_layout()
    assert product == header_layout(tmp_path)
    # what the kernels rely on: the view first, the parameters behind it on an 8-byte boundary, nothing behind them
    assert product["offsetof ix"] == 0 and product["offsetof params"] >= product["sizeof(IndexView)"] and product["offsetof params"] % 8 == 0
    assert product["sizeof(LaunchConst)"] == product["offsetof params"] + product["sizeof(Params)"]
    assert product["sizeof(LaunchConst)"] <= 4096
