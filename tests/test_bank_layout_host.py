"""csrc/bank_layout.h on the host: the remaps k_dense and k_bm_tiles place their LDS addresses with are bijections.
A stand-alone g++ program includes the header; it runs plain and under AddressSanitizer + UBSan.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "bank_layout.h"
using namespace spsamd;

int main()
{
	int bad = 0;
	// tile_key / tile_rel: inverse bijections of [0, 2^17)
	const uint32_t n = 1u << 17;
	std::vector<uint8_t> hit(n, 0);
	for (uint32_t x = 0; x < n; ++x) {
		const uint32_t k = tile_key(x);
		if (k >= n) { printf("tile_key(%u) = %u out of range\n", x, k); return 1; }
		if (hit[k]++) { if (!bad++) printf("tile_key hits %u twice\n", k); }
		if (tile_rel(k) != x) { if (!bad++) printf("tile_rel(tile_key(%u)) = %u\n", x, tile_rel(k)); }
		if (tile_key(tile_rel(x)) != x) { if (!bad++) printf("tile_key(tile_rel(%u)) = %u\n", x, tile_key(tile_rel(x))); }
	}
	for (uint32_t k = 0; k < n; ++k) if (hit[k] != 1) { if (!bad++) printf("tile_key misses %u\n", k); }
	// the dense swizzle: a bijection of [0, W) that never leaves a 64-slot group, its value a function of the group below 64
	uint32_t lowmix = 0;
	for (uint32_t W : {8192u, 16384u}) {
		std::vector<uint8_t> seen(W, 0);
		for (uint32_t s = 0; s < W; ++s) {
			const uint32_t z = dense_swz(s >> 6);
			if (z > 63u) { if (!bad++) printf("dense_swz(%u) = %u\n", s >> 6, z); continue; }
			const uint32_t p = s ^ z;
			if (p != dense_phys(s)) { if (!bad++) printf("dense_phys(%u)\n", s); }
			if (p >= W || (p >> 6) != (s >> 6)) { if (!bad++) printf("slot %u leaves its group: %u\n", s, p); continue; }
			if (seen[p]++) { if (!bad++) printf("W %u: physical slot %u taken twice\n", W, p); }
			if (dense_phys(p) != s) { if (!bad++) printf("dense_phys is not its own inverse at %u\n", s); }
			lowmix |= z;
		}
		for (uint32_t p = 0; p < W; ++p) if (seen[p] != 1) { if (!bad++) printf("W %u: physical slot %u unused\n", W, p); }
	}
	if ((lowmix & 15u) != 15u) { ++bad; printf("the group bits do not reach all of the low four bits: %u\n", lowmix); }
	printf(bad ? "FAILED\n" : "ok\n");
	return bad ? 1 : 0;
}
"""


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_remaps_are_bijections(tmp_path, sanitize):
    src = tmp_path / "bank_layout_check.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "bank_layout_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "spsparse_amd", "csrc"), str(src), "-o", exe]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
