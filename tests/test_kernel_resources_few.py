"""Register budgets of k_few, read from the built library's kernel metadata (no GPU).

k_few keeps the B tuples of the next cell in registers while it accumulates the current one: ceil(T / 2 / NT) tuples of
three words and an A value of two per thread, twice.  A spill there is a memory round trip per cell in front of the very
loads the kernel exists to issue early, so scratch is pinned to 0 for every instantiation.  The 256-thread T = 1024
kernels are meant to run at least four workgroups a CU and the 512-thread T = 4096 kernels two (53 KB to 71 KB of LDS):
four waves a SIMD, at most 128 VGPRs.  T = 8192 takes 104 KB of LDS and more, one workgroup a CU, which therefore has
1024 threads: four waves a SIMD again.
Only resource figures are read, never the instruction stream."""
import pytest

from scripts import kernel_resources
from tests.test_kernel_resources import MODE, instantiations

VGPR_MAX = {(1024, 256): 128, (4096, 512): 128, (8192, 1024): 128}


@pytest.fixture(scope="module")
def kernels():
    from spsparse_amd import build
    return kernel_resources.library_kernels(build.build())


def test_few_kernels_keep_their_tuples_in_registers(kernels):
    """k_few<T, NT, MODE>: every table class in every mode, no scratch, the VGPRs its workgroups per CU allow."""
    inst = instantiations(kernels, r"_ZN6spsamd5k_fewILi(\d+)ELi(\d+)ELi(\d)EE")
    assert set(inst) == {(t, nt, mode) for (t, nt) in VGPR_MAX for mode in MODE}
    for (t, nt, mode), f in sorted(inst.items()):
        what = "k_few<%d, %d, %s>: %r" % (t, nt, MODE[mode], f)
        assert f["scratch"] == 0 and f["vgpr_spill"] == 0, what
        assert f["vgpr"] + f["agpr"] <= VGPR_MAX[(t, nt)], what
