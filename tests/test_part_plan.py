"""Host logic of the equal-work parts of a sparse-conv launch of several rounds (csrc/isf_spconv16.h: conv16_part_cut /
conv16_part_firsts / conv16_class_bounds / conv16_part_slots): a small host program compiled with hipcc (no GPU needed) walks
the arithmetic the device kernel walks.  Every tile must be in exactly one part, the parts contiguous and ascending, none
above its cap, an unclamped part within one maximum tile weight of the even share, and the slots of a part a permutation of
its tiles with no work class lighter than a later one."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "isf_spconv16.h"
int main(int argc, char** argv) {   // parts raster w0 w1 ...
  const int parts = atoi(argv[1]);
  const bool raster = atoi(argv[2]) != 0;
  const int T = argc - 3;
  std::vector<int32_t> w(T), W(T);
  int32_t hist[256] = {0};
  long long run = 0;
  for (int i = 0; i < T; ++i) {
    w[i] = atoi(argv[3 + i]);
    run += w[i];
    W[i] = (int32_t)run;
    ++hist[w[i] < 255 ? w[i] : 255];
  }
  const int cap = isf::conv16_parts_cap(T, parts);
  printf("cap %d\n", cap);
  printf("cuts");
  for (int k = 0; k <= parts; ++k) printf(" %d", isf::conv16_part_cut(W.data(), T, parts, k));
  printf("\n");
  std::vector<int32_t> first(parts + 1), slots(cap);
  isf::conv16_part_firsts(W.data(), T, parts, cap, first.data());
  printf("first");
  for (int k = 0; k <= parts; ++k) printf(" %d", first[k]);
  printf("\n");
  int32_t bound[3];
  isf::conv16_class_bounds(hist, 256, bound);
  printf("bound %d %d %d\n", bound[0], bound[1], bound[2]);
  for (int k = 0; k < parts; ++k) {
    isf::conv16_part_slots(w.data(), first.data(), k, cap, bound, raster, slots.data());
    printf("slots");
    for (int j = 0; j < cap; ++j) printf(" %d", slots[j]);
    printf("\n");
  }
  printf("classes");
  for (int i = 0; i < T; ++i) printf(" %d", isf::conv16_work_class(w[i], bound));
  printf("\n");
  return 0;
}
"""


@pytest.fixture(scope="module")
def part_exe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("part_plan")
    src = d / "parts.hip"
    src.write_text(SRC)
    exe = d / "parts"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "is-fusion_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    return str(exe)


def plan_of(exe, weights, parts=8, raster=0):
    out = subprocess.run([exe, str(parts), str(raster)] + [str(int(v)) for v in weights], check=True, capture_output=True,
                         text=True).stdout.strip().split("\n")
    rec = {"slots": []}
    for ln in out:
        key, *vals = ln.split()
        vals = [int(v) for v in vals]
        if key == "slots":
            rec["slots"].append(vals)
        else:
            rec[key] = vals
    rec["cap"] = rec["cap"][0]
    return rec


def check_invariants(weights, parts, rec, raster=False):
    """the invariants of a part table; shared with the GPU test (tests/test_gpu_launch_balance.py imports it)"""
    T, cap, first = len(weights), rec["cap"], rec["first"]
    assert len(first) == parts + 1 and first[0] == 0 and first[-1] == T
    assert all(a <= b for a, b in zip(first, first[1:]))                  # contiguous, ascending: every tile in one part
    assert all(b - a <= cap for a, b in zip(first, first[1:]))            # no part above the cap
    assert parts * cap >= T
    total, wmax = sum(weights), max(weights)
    if "cuts" in rec:
        for k in range(parts):
            if first[k] == rec["cuts"][k] and first[k + 1] == rec["cuts"][k + 1]:    # neither end moved by the clamp
                share = sum(weights[first[k]:first[k + 1]])
                assert abs(share - total / parts) <= wmax, (k, share, total / parts, wmax)
    bound = rec["bound"]
    assert bound[0] <= bound[1] <= bound[2]

    def cls(w):
        return (w <= bound[2]) + (w <= bound[1]) + (w <= bound[0])
    for k in range(parts):
        slots = rec["slots"][k]
        assert len(slots) == cap
        n = first[k + 1] - first[k]
        live = slots[:n]
        assert sorted(live) == list(range(first[k], first[k + 1]))          # a permutation of the part's tiles
        assert all(s == -1 for s in slots[n:])
        if raster:
            assert live == list(range(first[k], first[k + 1]))
            continue
        c = [cls(weights[t]) for t in live]
        assert all(a <= b for a, b in zip(c, c[1:])), (k, c)               # heaviest class first, none lighter than a later one
        for a, b, ca, cb in zip(live, live[1:], c, c[1:]):
            assert ca != cb or a < b                                        # tile order inside a class


def _lcg(seed, n, lo, hi):
    out, x = [], seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7fffffff
        out.append(lo + (x >> 8) % (hi - lo + 1))
    return out


CASES = {
    "T < parts": [9, 30, 17],
    "T == 1": [21],
    "T == parts": [14, 35, 14, 20, 33, 9, 27, 16],
    "first eighth": [30] * 40 + [0] * 280,                    # the clamp engages, the excess is pushed on
    "last tile": [0] * 319 + [35],
    "random": _lcg(7, 2707, 14, 35),
    "dense middle": [14] * 900 + [35] * 500 + [14] * 1300,
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("parts", [8, 4])
@pytest.mark.parametrize("raster", [0, 1])
def test_part_table_invariants(part_exe, name, parts, raster):
    w = CASES[name]
    check_invariants(w, parts, plan_of(part_exe, w, parts, raster), bool(raster))


@pytest.mark.parametrize("T,parts", [(320, 8), (2707, 8), (5, 8), (322, 4)])
def test_equal_weights_give_the_even_cut(part_exe, T, parts):
    rec = plan_of(part_exe, [20] * T, parts)
    even = [(k * T + parts - 1) // parts for k in range(parts + 1)]
    assert rec["cuts"] == even and rec["first"] == even
    check_invariants([20] * T, parts, rec)


def test_clamp_pushes_the_excess_on(part_exe):
    """all the weight in the first eighth: the cuts crowd into it, so the last part would hold 7/8 of the tiles; every part
    takes what the parts behind it cannot hold"""
    w = CASES["first eighth"]
    rec = plan_of(part_exe, w)
    assert max(rec["cuts"][1:-1]) <= 40
    sizes = [b - a for a, b in zip(rec["first"], rec["first"][1:])]
    assert max(sizes) <= rec["cap"] and sum(sizes) == len(w) and sizes[-1] == rec["cap"]
    # all the weight in the last tile: every cut is behind it, the first part is clamped and hands the rest on
    rec = plan_of(part_exe, CASES["last tile"])
    sizes = [b - a for a, b in zip(rec["first"], rec["first"][1:])]
    assert sizes[0] == rec["cap"] and max(sizes) <= rec["cap"] and sum(sizes) == 320


def test_two_column_blocks_use_four_parts(part_exe):
    w = _lcg(3, 1400, 28, 62)
    rec = plan_of(part_exe, w, 4)
    assert len(rec["first"]) == 5 and rec["cap"] == 350 + 44 + 1
    check_invariants(w, 4, rec)
    shares = [sum(w[a:b]) for a, b in zip(rec["first"], rec["first"][1:])]
    assert max(shares) - min(shares) <= 2 * max(w)


GRID_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "isf_spconv16.h"
int main(int argc, char** argv) {   // n_out TM ncb seed: the launch's uniform plan, a part table over pseudo-random weights,
  const int n_out = atoi(argv[1]), TM = atoi(argv[2]), ncb = atoi(argv[3]);   // then every workgroup slot of the 8 x cap grid
  unsigned x = (unsigned)atoi(argv[4]);
  const int parts = ncb == 2 ? 4 : 8;
  const isf::Conv16Plan uni = isf::conv16_plan(n_out, TM, ncb, 6, 32, false);
  const int T = isf::conv16_parts_tiles(uni.full, parts), cap = isf::conv16_parts_cap(T, parts);
  std::vector<int32_t> w(T), W(T), table(isf::conv16_part_table_ints(parts, cap));
  int32_t hist[256] = {0};
  long long run = 0;
  for (int t = 0; t < T; ++t) {
    int r0, r1; bool h;
    x = x * 1103515245u + 12345u;
    w[t] = isf::conv16_tile_rows(uni, TM, n_out, t / uni.full, t % uni.full, r0, r1, h) ? 8 + (int)((x >> 8) % 40u) : 0;
    run += w[t];
    W[t] = (int32_t)run;
    ++hist[w[t]];
  }
  isf::conv16_part_firsts(W.data(), T, parts, cap, table.data());
  isf::conv16_class_bounds(hist, 256, table.data() + parts + 1);
  for (int k = 0; k < parts; ++k)
    isf::conv16_part_slots(w.data(), table.data(), k, cap, table.data() + parts + 1, false, table.data() + parts + 4 + k * cap);
  const isf::Conv16Plan plan{cap, isf::kPlanParts, uni.part_rows};
  printf("grid %d %d\n", 8 * cap, T);
  for (int part = 0; part < parts; ++part)
    for (int j = 0; j < cap; ++j) {
      int row0, row_end; bool half;
      if (isf::conv16_part_tile_rows(plan, TM, n_out, parts, table.data(), part, j, row0, row_end, half))
        printf("tile %d %d %d %d %d\n", part, j, row0, row0 + TM < row_end ? row0 + TM : row_end, (int)half);
    }
  for (int part = 0; part < parts; ++part)
    for (int j = 0; j < uni.full; ++j) {
      int row0, row_end; bool half;
      if (isf::conv16_tile_rows(uni, TM, n_out, part, j, row0, row_end, half))
        printf("plain %d %d %d %d %d\n", part, j, row0, row0 + TM < row_end ? row0 + TM : row_end, (int)half);
    }
  return 0;
}
"""


@pytest.fixture(scope="module")
def grid_exe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("part_grid")
    src = d / "grid.hip"
    src.write_text(GRID_SRC)
    exe = d / "grid"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "is-fusion_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    return str(exe)


@pytest.mark.parametrize("n_out", [1, 127, 1024, 1025, 1445, 5120, 346474, 358320])
@pytest.mark.parametrize("TM,ncb", [(128, 1), (256, 1), (128, 2)])
def test_the_grid_on_a_part_table_runs_the_plain_plan_s_tiles_once_each(grid_exe, n_out, TM, ncb):
    """what the kernels do with a part table (conv16_part_tile_rows over the 8 x cap grid): the same (first row, last row)
    tiles as the uniform plan, each exactly once, every part one contiguous ascending row range when read in tile order"""
    out = subprocess.run([grid_exe, str(n_out), str(TM), str(ncb), "5"], check=True, capture_output=True,
                         text=True).stdout.strip().split("\n")
    tiles = [tuple(int(v) for v in ln.split()[1:]) for ln in out if ln.startswith("tile")]
    plain = [tuple(int(v) for v in ln.split()[1:]) for ln in out if ln.startswith("plain")]
    assert sorted(t[2:] for t in tiles) == sorted(t[2:] for t in plain)
    assert len({t[2] for t in tiles}) == len(tiles)
    covered = sorted((t[2], t[3]) for t in tiles)
    assert covered[0][0] == 0 and covered[-1][1] == n_out
    assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
    parts = 4 if ncb == 2 else 8
    last = -1
    for p in range(parts):                                    # the parts own ascending, disjoint row ranges
        rows = sorted(t[2] for t in tiles if t[0] == p)
        if rows:
            assert rows[0] > last
            last = rows[-1]
