"""The pass plan of the stable radix sort (csrc/isf_sort.h: stable_sort_plan): how many passes a key of `key_bits` bits
takes and how many bits each pass sorts by.  The widths must sum to key_bits exactly -- a wider last pass would let bits
the caller said to ignore decide the order.  A small host program compiled with hipcc (no GPU needed) answers for every
key width."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SRC = r"""
#include <cstdio>
#include "isf_sort.h"
int main() {
  for (int kb = 1; kb <= 32; ++kb) {
    const isf::SortPlan pl = isf::stable_sort_plan(kb);
    printf("%d", pl.passes);
    for (int p = 0; p < pl.passes; ++p) printf(" %d", pl.bits[p]);
    printf("\n");
  }
  return 0;
}
"""

PINNED = {1: [1], 10: [10], 11: [6, 5], 21: [7, 7, 7], 22: [8, 8, 6], 31: [8, 8, 8, 7], 32: [8, 8, 8, 8]}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """one compile, one run: key_bits -> the bit count of every pass"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("sort_plan")
    src = d / "plan.hip"
    src.write_text(SRC)
    exe = d / "plan"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "is-fusion_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = {}
    for kb in range(1, 33):
        v = [int(x) for x in out[kb - 1].split()]
        assert v[0] == len(v) - 1
        got[kb] = v[1:]
    return got


@pytest.mark.parametrize("key_bits", range(1, 33))
def test_passes_cover_exactly_the_key_bits(plans, key_bits):
    bits = plans[key_bits]
    passes = -(-key_bits // 10)
    assert len(bits) == passes
    assert all(1 <= b <= 10 for b in bits)
    assert all(b == -(-key_bits // passes) for b in bits[:-1])
    assert sum(bits) == key_bits


@pytest.mark.parametrize("key_bits", sorted(PINNED))
def test_pinned_rows(plans, key_bits):
    assert plans[key_bits] == PINNED[key_bits]
