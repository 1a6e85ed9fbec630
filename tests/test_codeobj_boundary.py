"""CPU tier: the library's device code is cut where the sources say it is.  The lane-per-read align kernel, the two test kernels behind it and the out-of-line
device functions of the per-read state machine are compiled by xm_align_kernel.hip alone; the host unit, xm_capi.hip, includes the same headers (it needs their
host-side pieces) with the out-of-line functions made inline, and must emit none of them for the device - an edit of the host side then cannot re-make or move the
kernel.  The test reads the symbol tables of the gfx950 code objects in the built objects (unbundled as scripts/codeobj_diff.sh does); it looks at names only."""
import os
import subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapper_amd", "_lib")
LLVM = "/opt/rocm/lib/llvm/bin"
KERNELS = ("xm_align_kernel", "xm_test_local_kernel", "xm_test_bound_kernel")
OUT_OF_LINE = ("alignRead", "innerChain", "pathSearchLds", "pathSearchHbm", "compStep", "boundRejects")


def device_symbols(obj, tmp):
    """names the gfx950 code object of `obj` defines"""
    fatbin, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fatbin, obj, os.devnull], check=True, capture_output=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fatbin, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co],
                   check=True, capture_output=True)
    table = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", co], check=True, capture_output=True, text=True).stdout
    return [f[-1] for f in (line.split() for line in table.splitlines()) if len(f) >= 5 and "*UND*" not in f]


def test_the_align_kernel_and_its_functions_are_in_their_own_object(tmp_path):
    objs = {n: os.path.join(LIB, n + ".o") for n in ("xm_align_kernel", "xm_capi")}
    tools = [os.path.join(LLVM, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")]
    if not all(os.path.exists(p) for p in list(objs.values()) + tools):
        pytest.skip("needs the product's object files beside the library (make -C mapper_amd/csrc) and the LLVM tools of ROCm")
    syms = {}
    for n, obj in objs.items():
        d = tmp_path / n
        d.mkdir()
        syms[n] = device_symbols(obj, str(d))
    for k in KERNELS:  # (kernels of an anonymous namespace: the mangled name holds the plain one)
        assert any(k in s for s in syms["xm_align_kernel"]), "%s is not defined in xm_align_kernel.o" % k
        assert not any(k in s for s in syms["xm_capi"]), "%s is defined in xm_capi.o" % k
    for f in OUT_OF_LINE:
        assert any(f in s for s in syms["xm_align_kernel"]), "%s is not defined in xm_align_kernel.o (the test's list is stale?)" % f
        assert not any(f in s for s in syms["xm_capi"]), "the host unit emits %s for the device: %s" % (f, [s for s in syms["xm_capi"] if f in s])
