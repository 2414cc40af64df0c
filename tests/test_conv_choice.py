"""The instantiation choice of the f16x3 tile kernel (csrc/isf_spconv16.h: conv16_choose / conv16_choose_trace): which
spconv_f16x3_kernel<c_in, NT, RG, NW, MODE> -- or the deep kernel -- a launch of (c_in, c_out, n_out, mode) runs on.  A small
host program compiled with hipcc (no GPU needed) answers every row of the literal table below.  The table is the behaviour
of the cascade this function replaced (launch16_rows / dispatch16 / run16 / trace16), taken from that cascade itself with
its launches stubbed out -- not from conv16_choose -- so a change of a production shape shows up here as a changed row."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

SRC = r"""
#include <cstdio>
#include "isf_spconv16.h"
int main() {
  char kind;
  int c_in, c_out, n_out, mode, rowmap, cus;
  while (scanf(" %c %d %d %d %d %d %d", &kind, &c_in, &c_out, &n_out, &mode, &rowmap, &cus) == 7) {
    isf::Conv16Choice ch;
    int r = ISF_OK;
    if (kind == 't') ch = isf::conv16_choose_trace(c_in, c_out, n_out, mode);
    else r = isf::conv16_choose(c_in, c_out, n_out, mode, rowmap != 0, cus, &ch);
    if (r != ISF_OK) printf("%d\n", r);
    else if (ch.backend == isf::kConv16Deep) printf("0 1 %d %d\n", (int)ch.uniform_tiles, (int)ch.drop_order);
    else printf("0 0 %d %d %d %d %d %d\n", ch.nt, ch.rg, ch.nw, ch.kern, (int)ch.uniform_tiles, (int)ch.drop_order);
  }
  printf("rules %d %d %d %d %d %d\n", (int)isf::conv16_wide_shape(128, 2047), (int)isf::conv16_wide_shape(128, 2048),
         (int)isf::conv16_wide_shape(256, 400000), isf::conv16_small_rows_256(256), isf::conv16_small_rows_wide(256),
         isf::conv16_small_rows_256(32));
  return 0;
}
"""

# include/isf_hip.h (ISF_CONV_MODE_*) and csrc/isf_spconv16.h (the library's internal bits)
F16, NO_GATHER, NO_WEIGHTS, NO_LOOP, NO_SHARING, UNIFORM, F16_ROWS, F16_STORAGE = 1, 2, 4, 8, 16, 32, 256, 257
NARROW, TILE_TABLE, PART_TABLE = 64, 1024, 16384
OB4, OB8, DEEP, STAGGER, R4, TWO_AHEAD, CHUNK = 4096, 8192, 32768, 65536, 131072, 262144, 524288
TRACE, PHASE = 512, 2048            # kernel MODE bits of the trace instantiations; as runtime modes of a launch they are none
ARG, UNSUPPORTED = -1, -4           # ISF_ERR_ARG, ISF_ERR_UNSUPPORTED
TILE = 0
DEEP_KERNEL = (1, 0, 0)             # isf_spconv_deep.hip, the call unchanged

# ((c_in, c_out, n_out, mode, has_rowmap, cus), (TILE, NT, RG, NW, kernel MODE, uniform_tiles, drop_order) | DEEP_KERNEL | error)
# thresholds on 256 compute units: 8 waves from 2048 rows of 128 columns, one group per wave up to 65536 of them and up to
# 24576 rows of 256 columns; on 32: 8192 and 3072
CHOICES = [
    # mode 0: every production shape on each side of each threshold
    ((32, 32, 1, 0, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((32, 32, 400000, 0, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((32, 64, 1, 0, 0, 256), (TILE, 4, 2, 4, 0, 0, 0)),
    ((32, 64, 400000, 0, 0, 256), (TILE, 4, 2, 4, 0, 0, 0)),
    ((64, 64, 1, 0, 0, 256), (TILE, 4, 2, 4, 0, 0, 0)),
    ((64, 64, 400000, 0, 0, 256), (TILE, 4, 2, 4, 0, 0, 0)),
    ((64, 32, 1, 0, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 32, 400000, 0, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 128, 2047, 0, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((64, 128, 2048, 0, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((64, 128, 65536, 0, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((64, 128, 65537, 0, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),
    ((128, 128, 2047, 0, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 128, 2048, 0, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((128, 128, 65536, 0, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((128, 128, 65537, 0, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),
    ((128, 256, 1, 0, 0, 256), (TILE, 8, 1, 4, 0, 0, 0)),
    ((128, 256, 24576, 0, 0, 256), (TILE, 8, 1, 4, 0, 0, 0)),
    ((128, 256, 24577, 0, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 256, 400000, 0, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 1, 0, 0, 256), (TILE, 8, 1, 4, 0, 0, 0)),
    ((256, 256, 24576, 0, 0, 256), (TILE, 8, 1, 4, 0, 0, 0)),
    ((256, 256, 24577, 0, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 400000, 0, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((64, 256, 24576, 0, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),          # the one-group 256-column shape: >= 128 in only
    ((256, 128, 2048, 0, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((256, 128, 65537, 0, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),
    ((128, 128, 8192, 0, 0, 32), (TILE, 8, 1, 8, 0, 0, 0)),           # the bounds follow the compute units
    ((128, 128, 8193, 0, 0, 32), (TILE, 8, 2, 8, 0, 0, 0)),
    ((256, 256, 3072, 0, 0, 32), (TILE, 8, 1, 4, 0, 0, 0)),
    ((256, 256, 3073, 0, 0, 32), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 128, 100000, UNIFORM, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),  # the tile bits pick no shape
    ((256, 256, 3000, UNIFORM, 0, 256), (TILE, 8, 1, 4, 0, 0, 0)),
    ((128, 128, 100000, PART_TABLE, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),
    ((256, 256, 30000, TILE_TABLE, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    # every opt-in bit: alone on a large and a small 256 -> 256 launch, with UNIFORM_TILES, on 32 -> 32 and 64 -> 256, and on
    # 128 -> 128 above the 8-wave bound (large, small) and below it
    ((256, 256, 30000, STAGGER, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((256, 256, 3000, STAGGER, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((256, 256, 30000, UNIFORM | STAGGER, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((32, 32, 30000, STAGGER, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 256, 30000, STAGGER, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((128, 128, 100000, STAGGER, 0, 256), (TILE, 8, 2, 8, STAGGER, 0, 0)),
    ((128, 128, 3000, STAGGER, 0, 256), (TILE, 8, 2, 8, STAGGER, 0, 0)),
    ((128, 128, 1000, STAGGER, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((256, 256, 30000, R4, 0, 256), (TILE, 8, 2, 4, R4, 0, 0)),
    ((256, 256, 3000, R4, 0, 256), (TILE, 8, 2, 4, R4, 0, 0)),
    ((256, 256, 30000, UNIFORM | R4, 0, 256), (TILE, 8, 2, 4, R4, 0, 0)),
    ((32, 32, 30000, R4, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 256, 30000, R4, 0, 256), (TILE, 8, 2, 4, R4, 0, 0)),
    ((128, 128, 100000, R4, 0, 256), (TILE, 8, 2, 8, R4, 0, 0)),
    ((128, 128, 3000, R4, 0, 256), (TILE, 8, 2, 8, R4, 0, 0)),
    ((128, 128, 1000, R4, 0, 256), (TILE, 8, 2, 4, R4, 0, 0)),
    ((256, 256, 30000, TWO_AHEAD, 0, 256), (TILE, 8, 2, 4, TWO_AHEAD, 0, 0)),
    ((256, 256, 3000, TWO_AHEAD, 0, 256), (TILE, 8, 2, 4, TWO_AHEAD, 0, 0)),
    ((256, 256, 30000, UNIFORM | TWO_AHEAD, 0, 256), (TILE, 8, 2, 4, TWO_AHEAD, 0, 0)),
    ((128, 256, 30000, TWO_AHEAD, 0, 256), (TILE, 8, 2, 4, TWO_AHEAD, 0, 0)),
    ((32, 32, 30000, TWO_AHEAD, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 256, 30000, TWO_AHEAD, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 128, 100000, TWO_AHEAD, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),           # ignored on the 8-wave shape
    ((128, 128, 3000, TWO_AHEAD, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((128, 128, 1000, TWO_AHEAD, 0, 256), (TILE, 8, 2, 4, TWO_AHEAD, 0, 0)),
    ((256, 256, 30000, CHUNK, 0, 256), (TILE, 8, 2, 4, CHUNK, 0, 0)),
    ((256, 256, 3000, CHUNK, 0, 256), (TILE, 8, 1, 4, CHUNK, 0, 0)),             # follows the small-launch rule
    ((128, 256, 3000, CHUNK, 0, 256), (TILE, 8, 1, 4, CHUNK, 0, 0)),
    ((256, 256, 30000, UNIFORM | CHUNK, 0, 256), (TILE, 8, 2, 4, CHUNK, 0, 0)),
    ((256, 256, 30000, CHUNK, 1, 256), (TILE, 8, 2, 4, CHUNK, 0, 0)),
    ((32, 32, 30000, CHUNK, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 256, 30000, CHUNK, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 128, 100000, CHUNK, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),
    ((128, 128, 3000, CHUNK, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((128, 128, 1000, CHUNK, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 30000, OB4, 0, 256), (TILE, 16, 2, 4, 0, 0, 1)),                 # one column block: no tile order
    ((256, 256, 3000, OB4, 0, 256), (TILE, 16, 2, 4, 0, 0, 1)),
    ((256, 256, 30000, UNIFORM | OB4, 0, 256), (TILE, 16, 2, 4, 0, 0, 1)),
    ((256, 256, 30000, OB4, 1, 256), (TILE, 8, 2, 4, 0, 0, 0)),                  # ... and no row map
    ((32, 32, 30000, OB4, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 256, 30000, OB4, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 128, 100000, OB4, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),
    ((128, 128, 3000, OB4, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((128, 128, 1000, OB4, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 30000, OB8, 0, 256), (TILE, 16, 1, 8, 0, 1, 1)),                 # one group per wave: uniform tiles forced
    ((256, 256, 3000, OB8, 0, 256), (TILE, 16, 1, 8, 0, 1, 1)),
    ((256, 256, 30000, UNIFORM | OB8, 0, 256), (TILE, 16, 1, 8, 0, 1, 1)),
    ((256, 256, 30000, OB8, 1, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((32, 32, 30000, OB8, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 256, 30000, OB8, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 128, 100000, OB8, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),
    ((128, 128, 3000, OB8, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((128, 128, 1000, OB8, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 30000, DEEP, 0, 256), DEEP_KERNEL),
    ((256, 256, 30000, UNIFORM | DEEP, 0, 256), DEEP_KERNEL),
    ((256, 256, 30000, TILE_TABLE | DEEP, 0, 256), DEEP_KERNEL),
    ((128, 128, 1000, DEEP, 0, 256), DEEP_KERNEL),
    ((256, 256, 30000, DEEP, 1, 256), (TILE, 8, 2, 4, 0, 0, 0)),                 # no row map, no part table
    ((256, 256, 30000, PART_TABLE | DEEP, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 3000, DEEP, 0, 256), (TILE, 8, 1, 4, 0, 0, 0)),                  # behind the small-launch rules
    ((256, 256, 24576, DEEP, 0, 256), (TILE, 8, 1, 4, 0, 0, 0)),
    ((128, 128, 3000, DEEP, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),
    ((128, 128, 100000, DEEP, 0, 256), (TILE, 8, 2, 8, 0, 0, 0)),                # ... and the 8-wave rule
    ((32, 32, 30000, DEEP, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 256, 30000, DEEP, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 30000, DEEP | STAGGER, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((256, 256, 30000, F16 | DEEP, 0, 256), (TILE, 8, 2, 4, F16, 0, 0)),
    ((128, 128, 100000, NARROW, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 128, 100000, UNIFORM | NARROW, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((128, 128, 100000, NARROW | DEEP, 0, 256), DEEP_KERNEL),
    ((128, 128, 3000, NARROW, 0, 256), (TILE, 8, 1, 8, 0, 0, 0)),                # does not override the small launch
    ((128, 128, 1000, NARROW, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 30000, NARROW, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    ((256, 256, 3000, NARROW, 0, 256), (TILE, 8, 1, 4, 0, 0, 0)),
    ((32, 32, 30000, NARROW, 0, 256), (TILE, 2, 2, 4, 0, 0, 0)),
    ((64, 256, 30000, NARROW, 0, 256), (TILE, 8, 2, 4, 0, 0, 0)),
    # the base modes: f16 storage and no-sharing on the production shapes (8 waves, but two groups whatever the rows),
    # single-pass f16 and the knock-outs on 4 waves
    ((256, 256, 30000, F16, 0, 256), (TILE, 8, 2, 4, F16, 0, 0)),
    ((256, 256, 3000, F16, 0, 256), (TILE, 8, 2, 4, F16, 0, 0)),
    ((256, 256, 30000, F16 | UNIFORM, 0, 256), (TILE, 8, 2, 4, F16, 0, 0)),
    ((32, 32, 30000, F16, 0, 256), (TILE, 2, 2, 4, F16, 0, 0)),
    ((64, 256, 30000, F16, 0, 256), (TILE, 8, 2, 4, F16, 0, 0)),
    ((128, 128, 100000, F16, 0, 256), (TILE, 8, 2, 4, F16, 0, 0)),
    ((128, 128, 3000, F16, 0, 256), (TILE, 8, 2, 4, F16, 0, 0)),
    ((256, 256, 30000, NO_SHARING, 0, 256), (TILE, 8, 2, 4, NO_SHARING, 0, 0)),
    ((256, 256, 3000, NO_SHARING, 0, 256), (TILE, 8, 2, 4, NO_SHARING, 0, 0)),
    ((256, 256, 30000, NO_SHARING | UNIFORM, 0, 256), (TILE, 8, 2, 4, NO_SHARING, 0, 0)),
    ((32, 32, 30000, NO_SHARING, 0, 256), (TILE, 2, 2, 4, NO_SHARING, 0, 0)),
    ((64, 64, 30000, NO_SHARING, 0, 256), (TILE, 4, 2, 4, NO_SHARING, 0, 0)),
    ((128, 128, 100000, NO_SHARING, 0, 256), (TILE, 8, 2, 8, NO_SHARING, 0, 0)),
    ((128, 128, 3000, NO_SHARING, 0, 256), (TILE, 8, 2, 8, NO_SHARING, 0, 0)),
    ((128, 128, 1000, NO_SHARING, 0, 256), (TILE, 8, 2, 4, NO_SHARING, 0, 0)),
    ((256, 256, 30000, F16_STORAGE, 0, 256), (TILE, 8, 2, 4, F16_STORAGE, 0, 0)),
    ((256, 256, 3000, F16_STORAGE, 0, 256), (TILE, 8, 2, 4, F16_STORAGE, 0, 0)),
    ((256, 256, 30000, F16_STORAGE | UNIFORM, 0, 256), (TILE, 8, 2, 4, F16_STORAGE, 0, 0)),
    ((32, 32, 30000, F16_STORAGE, 0, 256), (TILE, 2, 2, 4, F16_STORAGE, 0, 0)),
    ((64, 256, 30000, F16_STORAGE, 0, 256), (TILE, 8, 2, 4, F16_STORAGE, 0, 0)),
    ((128, 128, 100000, F16_STORAGE, 0, 256), (TILE, 8, 2, 8, F16_STORAGE, 0, 0)),
    ((128, 128, 3000, F16_STORAGE, 0, 256), (TILE, 8, 2, 8, F16_STORAGE, 0, 0)),
    ((128, 128, 1000, F16_STORAGE, 0, 256), (TILE, 8, 2, 4, F16_STORAGE, 0, 0)),
    ((256, 256, 30000, NO_GATHER, 0, 256), (TILE, 8, 2, 4, NO_GATHER, 0, 0)),
    ((256, 256, 30000, NO_GATHER | UNIFORM, 0, 256), (TILE, 8, 2, 4, NO_GATHER, 0, 0)),
    ((32, 32, 30000, NO_GATHER, 0, 256), (TILE, 2, 2, 4, NO_GATHER, 0, 0)),
    ((128, 128, 100000, NO_GATHER, 0, 256), (TILE, 8, 2, 4, NO_GATHER, 0, 0)),
    ((256, 256, 30000, NO_WEIGHTS, 0, 256), (TILE, 8, 2, 4, NO_WEIGHTS, 0, 0)),
    ((256, 256, 30000, NO_WEIGHTS | UNIFORM, 0, 256), (TILE, 8, 2, 4, NO_WEIGHTS, 0, 0)),
    ((32, 32, 30000, NO_WEIGHTS, 0, 256), (TILE, 2, 2, 4, NO_WEIGHTS, 0, 0)),
    ((128, 128, 100000, NO_WEIGHTS, 0, 256), (TILE, 8, 2, 4, NO_WEIGHTS, 0, 0)),
    ((256, 256, 30000, NO_GATHER | NO_WEIGHTS, 0, 256), (TILE, 8, 2, 4, NO_GATHER | NO_WEIGHTS, 0, 0)),
    ((256, 256, 30000, NO_GATHER | NO_WEIGHTS | UNIFORM, 0, 256), (TILE, 8, 2, 4, NO_GATHER | NO_WEIGHTS, 0, 0)),
    ((32, 32, 30000, NO_GATHER | NO_WEIGHTS, 0, 256), (TILE, 2, 2, 4, NO_GATHER | NO_WEIGHTS, 0, 0)),
    ((128, 128, 100000, NO_GATHER | NO_WEIGHTS, 0, 256), (TILE, 8, 2, 4, NO_GATHER | NO_WEIGHTS, 0, 0)),
    ((256, 256, 30000, NO_LOOP, 0, 256), (TILE, 8, 2, 4, NO_LOOP, 0, 0)),
    ((256, 256, 30000, NO_LOOP | UNIFORM, 0, 256), (TILE, 8, 2, 4, NO_LOOP, 0, 0)),
    ((32, 32, 30000, NO_LOOP, 0, 256), (TILE, 2, 2, 4, NO_LOOP, 0, 0)),
    ((128, 128, 100000, NO_LOOP, 0, 256), (TILE, 8, 2, 4, NO_LOOP, 0, 0)),
    # pairs: a variant takes the launch only when nothing else is left of the mode; the later one in the order wins
    ((256, 256, 30000, STAGGER | R4, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((128, 128, 100000, STAGGER | R4, 0, 256), (TILE, 8, 2, 8, STAGGER, 0, 0)),
    ((256, 256, 30000, STAGGER | TWO_AHEAD, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((256, 256, 30000, R4 | TWO_AHEAD, 0, 256), (TILE, 8, 2, 4, R4, 0, 0)),
    ((256, 256, 30000, STAGGER | CHUNK, 0, 256), (TILE, 8, 2, 4, STAGGER, 0, 0)),
    ((256, 256, 30000, OB8 | CHUNK, 0, 256), (TILE, 16, 1, 8, 0, 1, 1)),
    ((256, 256, 30000, OB4 | OB8, 0, 256), (TILE, 16, 1, 8, 0, 1, 1)),
    ((256, 256, 30000, F16 | STAGGER, 0, 256), (TILE, 8, 2, 4, F16, 0, 0)),
    ((256, 256, 30000, F16_STORAGE | OB8, 0, 256), (TILE, 8, 2, 4, F16_STORAGE, 0, 0)),
    ((256, 256, 30000, NO_SHARING | CHUNK, 0, 256), (TILE, 8, 2, 4, NO_SHARING, 0, 0)),
    # what is left is no base mode: single-pass precision and the knock-outs do not combine
    ((256, 256, 30000, F16 | NO_GATHER, 0, 256), ARG),
    ((256, 256, 30000, F16 | NO_SHARING, 0, 256), ARG),
    ((256, 256, 30000, NO_GATHER | NO_SHARING, 0, 256), ARG),
    ((256, 256, 30000, NO_GATHER | NO_LOOP, 0, 256), ARG),
    ((256, 256, 30000, F16_ROWS, 0, 256), ARG),
    ((256, 256, 30000, F16_STORAGE | NO_SHARING, 0, 256), ARG),
    ((256, 256, 30000, F16_STORAGE | NO_GATHER, 0, 256), ARG),
    ((256, 256, 30000, F16 | NO_GATHER | STAGGER, 0, 256), ARG),
    ((256, 256, 30000, TRACE, 0, 256), ARG),
    ((256, 256, 30000, PHASE, 0, 256), ARG),
    ((32, 32, 1000, F16 | NO_LOOP, 0, 256), ARG),
    ((128, 128, 100000, NO_LOOP | NO_SHARING | NARROW, 0, 256), ARG),
    ((16, 32, 1000, 0, 0, 256), UNSUPPORTED),
    ((32, 48, 1000, 0, 0, 256), UNSUPPORTED),
    ((512, 256, 1000, 0, 0, 256), UNSUPPORTED),
]

# (c_in, c_out, n_out, mode) -> the trace instantiation: the production shape of 128 -> 128 and 256 -> 256; the kernels
# exist for 128 and 256 input channels, and any other width is answered with 128's
TRACES = [
    ((256, 256, 30000, TRACE), (TILE, 8, 2, 4, TRACE, 0, 0)),
    ((256, 256, 3000, TRACE), (TILE, 8, 2, 4, TRACE, 0, 0)),
    ((256, 256, 30000, TRACE | PHASE), (TILE, 8, 2, 4, TRACE | PHASE, 0, 0)),
    ((128, 128, 2047, TRACE), (TILE, 8, 2, 4, TRACE, 0, 0)),
    ((128, 128, 2048, TRACE), (TILE, 8, 2, 8, TRACE, 0, 0)),
    ((128, 128, 100000, TRACE | PHASE), (TILE, 8, 2, 8, TRACE | PHASE, 0, 0)),
    ((128, 128, 2047, TRACE | PHASE), (TILE, 8, 2, 4, TRACE | PHASE, 0, 0)),
    ((128, 128, 100000, TRACE | UNIFORM), (TILE, 8, 2, 8, TRACE, 0, 0)),
    ((256, 128, 100000, TRACE), (TILE, 8, 2, 4, TRACE, 0, 0)),
    ((64, 128, 100000, TRACE), (TILE, 8, 2, 8, TRACE, 0, 0)),
    ((128, 256, 100000, TRACE), (TILE, 8, 2, 4, TRACE, 0, 0)),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """one compile, one run: the program's answer to every row of both tables, and the named rules"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("conv_choice")
    src = d / "choice.hip"
    src.write_text(SRC)
    exe = d / "choice"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "is-fusion_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    rows = [("c",) + q for q, _ in CHOICES] + [("t",) + q + (0, 256) for q, _ in TRACES]
    out = subprocess.run([str(exe)], input="".join(" ".join(map(str, r)) + "\n" for r in rows), check=True,
                         capture_output=True, text=True).stdout.split("\n")
    assert len(out) >= len(rows) + 1
    got = {}
    for r, ln in zip(rows, out):
        v = tuple(int(x) for x in ln.split())
        got[r] = v[0] if v[0] != 0 else v[1:]
    got["rules"] = tuple(int(x) for x in out[len(rows)].split()[1:])
    return got


def test_the_tables_hold_no_row_twice():
    assert len({q for q, _ in CHOICES}) == len(CHOICES) and len({q for q, _ in TRACES}) == len(TRACES)


@pytest.mark.parametrize("query,expected", CHOICES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_launch_runs_on_the_instantiation_the_cascade_chose(answers, query, expected):
    assert answers[("c",) + query] == expected


@pytest.mark.parametrize("query,expected", TRACES, ids=lambda v: "-".join(map(str, v)))
def test_trace_runs_on_the_production_shape_of_the_two_deep_widths(answers, query, expected):
    assert answers[("t",) + query + (0, 256)] == expected


def test_named_rules_are_the_thresholds_of_the_table(answers):
    """8 waves: exactly 128 columns from 8 x 256 rows; one group per wave: <= 96 x CUs rows of 256 columns (3 workgroups
    x 4 groups x 16 rows / 2 column blocks), <= 256 x CUs of the 8-wave shape (2 x 8 x 16) -- where tests/test_tile_plan.py
    shows the plan to stop being all half tiles"""
    assert answers["rules"] == (0, 1, 0, 96 * 256, 256 * 256, 96 * 32)
