"""Register budgets of the heavy-row kernels, read from the built library's kernel metadata (no GPU).

k_dense for 8192-column windows and k_bm_tiles run two 512-thread workgroups per CU, four waves per SIMD: at most 128
VGPRs.  The compiler holds a kernel to its launch bound by spilling, so for the dense STORE and DIGEST launches the
scratch size is pinned to 0 as well: their scan-out keeps a batch of sums in registers, and a spill there is a memory
round trip per cell.  Only resource figures are read, never the instruction stream."""
import re

import pytest

from scripts import kernel_resources

MODE = {0: "COUNT", 1: "STORE", 2: "DIGEST"}


@pytest.fixture(scope="module")
def kernels():
    from spsparse_amd import build
    return kernel_resources.library_kernels(build.build())


def instantiations(kernels, pattern):
    """{template arguments as a tuple of ints: figures} of the kernels whose mangled name matches."""
    out = {}
    for name, figures in kernels.items():
        m = re.match(pattern, name)
        if m:
            out[tuple(int(x) for x in m.groups())] = figures
    return out


def test_dense_8192_store_and_digest_fit_two_workgroups_per_cu(kernels):
    """k_dense<8192, 512, MODE, PAT, PLAIN>: STORE and DIGEST, plain and general (and EXACT_PATTERN)."""
    inst = instantiations(kernels, r"_ZN6spsamd7k_denseILi(\d+)ELi(\d+)ELi(\d)ELb([01])ELb([01])EE")
    small = {k[2:]: v for k, v in inst.items() if k[:2] == (8192, 512) and MODE[k[2]] != "COUNT"}
    for mode in (1, 2):
        assert (mode, 0, 1) in small and (mode, 0, 0) in small, "PLAIN and general instantiation of %s" % MODE[mode]
    for (mode, pat, plain), f in sorted(small.items()):
        what = "k_dense<8192, 512, %s, %s, %s>: %r" % (MODE[mode], bool(pat), bool(plain), f)
        assert f["vgpr"] + f["agpr"] <= 128, what
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, what


def test_bitmap_tiles_fit_two_workgroups_per_cu(kernels):
    """Every k_bm_tiles instantiation: at most 128 VGPRs."""
    inst = instantiations(kernels, r"_ZN6spsamd10k_bm_tilesILi(\d)ELb([01])ELb([01])EE")
    assert {k[0] for k in inst} == {0, 1, 2} and len(inst) >= 8
    for k, f in sorted(inst.items()):
        assert f["vgpr"] + f["agpr"] <= 128, "k_bm_tiles<%s, ...%r>: %r" % (MODE[k[0]], k[1:], f)
