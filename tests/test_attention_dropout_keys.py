"""CPU tests of the attention-probability dropout beyond 512 keys (the head's 200 x 32400 cross-attention in training):

  * isf_attention_forward_dropout / isf_attention_backward_dropout take any number of keys for head_dim 16 and refuse, before
    any HIP call (so none of these calls needs a GPU), what the mask hash cannot index: another head_dim, queries or keys
    from 2^24, batch * heads from 2^16;
  * csrc/isf_attention_plan.h (attention_forward_plan / attention_backward_plan): which kernels a shape runs on.  A small
    host program compiled with hipcc answers the literal tables below.  The rows of the shapes that existed before the
    key-split route are the arithmetic that stood inline in attention_forward_impl / attention_backward_impl (worked out by
    hand from those formulas, not from the new functions), so a shape that changes its route shows up as a changed row;
  * attn_keep (isf_common.h, __host__ __device__) from the same program against fusion_ops.attention_keep_mask."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ISF_OK, ISF_ERR_ARG, ISF_ERR_UNSUPPORTED = 0, -1, -4


# ------------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture(scope="module")
def lib():
    from isfusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _calls(lib):
    """(name, call(B, Lq, Lk, E, heads, p)) for the two entries; pointers that are never dereferenced"""
    buf = (ctypes.c_float * 4)()
    p = ctypes.addressof(buf)

    def fwd(B, Lq, Lk, E, heads, drop):
        return lib.isf_attention_forward_dropout(p, E, p, p, E, B, Lq, Lk, E, heads, drop, 7, p, E, None)

    def bwd(B, Lq, Lk, E, heads, drop):
        return lib.isf_attention_backward_dropout(p, E, p, p, E, p, p, E, B, Lq, Lk, E, heads, drop, 7, p, E, p, p, E, None)
    return (("forward", fwd), ("backward", bwd))


def test_dropout_entries_take_any_number_of_keys(lib):
    """the feature's front door: refused (ISF_ERR_UNSUPPORTED) above 512 keys before this change"""
    for name, call in _calls(lib):
        for Lk in (200, 512, 513, 1296, 32400, (1 << 24) - 1):
            assert call(0, 200, Lk, 128, 8, 0.1) == ISF_OK, (name, Lk)
            assert call(0, (1 << 24) - 1, Lk, 128, 8, 0.1) == ISF_OK, (name, Lk)


def test_dropout_entries_refuse_other_head_dims_and_say_which(lib):
    for name, call in _calls(lib):
        for Lk in (200, 32400):
            assert call(0, 200, Lk, 256, 8, 0.1) == ISF_ERR_UNSUPPORTED, (name, Lk)
            msg = lib.isf_last_error().decode()
            assert "head_dim 16" in msg and "32" in msg and "256" in msg, msg
        assert call(0, 200, 200, 64, 8, 0.1) == ISF_ERR_UNSUPPORTED
        assert "got 8" in lib.isf_last_error().decode()
        assert call(0, 200, 200, 128, 8, 1.0) == ISF_ERR_ARG           # the probability's own check comes first


def test_dropout_entries_refuse_indices_the_hash_would_alias(lib):
    """attn_keep packs bh << 48 | query << 24 | key: 24 bits each for query and key, 16 for sample * heads + head"""
    for name, call in _calls(lib):
        assert call(0, 200, 1 << 24, 128, 8, 0.1) == ISF_ERR_UNSUPPORTED, name
        msg = lib.isf_last_error().decode()
        assert "num_keys" in msg and str(1 << 24) in msg, msg
        assert call(0, 1 << 24, 200, 128, 8, 0.1) == ISF_ERR_UNSUPPORTED, name
        msg = lib.isf_last_error().decode()
        assert "num_queries" in msg and str(1 << 24) in msg, msg
        assert call(8192, 200, 200, 128, 8, 0.1) == ISF_ERR_UNSUPPORTED, name          # 8192 * 8 = 2^16
        msg = lib.isf_last_error().decode()
        assert "batch_size * num_heads" in msg and str(1 << 16) in msg, msg
        assert call(1 << 12, 200, 200, 256, 16, 0.1) == ISF_ERR_UNSUPPORTED, name       # 4096 * 16 = 2^16
        # without dropout nothing is hashed: the same sizes pass (no samples: the call returns before it looks further)
        assert call(0, 200, 1 << 24, 128, 8, 0.0) == ISF_OK, name
        assert call(0, 1 << 24, 200, 128, 8, 0.0) == ISF_OK, name
    # batch * heads = 2^16 without dropout: only the forward can answer without a device (no queries: nothing to do)
    assert _calls(lib)[0][1](8192, 0, 200, 128, 8, 0.0) == ISF_OK
    assert _calls(lib)[0][1](8192, 0, 200, 128, 8, 0.1) == ISF_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------- the plan and the hash
SRC = r"""
#include <cstdio>
#include "isf_attention_plan.h"
#include "isf_common.h"
int main() {
  char kind;
  long long a, b, c, d, e;
  while (scanf(" %c %lld %lld %lld %lld %lld", &kind, &a, &b, &c, &d, &e) == 6) {
    if (kind == 'f') {
      const isf::AttnForwardPlan p = isf::attention_forward_plan((int)a, (int)b, (int)c, 8, (int)d);
      printf("%d %d %zu\n", p.keys_per_split, p.splits, p.workspace_floats);
    } else if (kind == 'b') {
      const isf::AttnBackwardPlan p = isf::attention_backward_plan((int)a, (int)b, (int)c, 8, d != 0);
      printf("%d %d %d %zu\n", p.route, p.chunks, p.key_splits, p.workspace_floats);
    } else {
      printf("%d\n", (int)isf::attn_keep((unsigned long long)a, (unsigned)b, (unsigned)c, (unsigned)d, (unsigned)e));
    }
  }
  return 0;
}
"""

WAVE, LANES, KEYSPLIT = 0, 1, 2
HEADS = 8

# (B, Lq, Lk, dropout) -> (route, query chunks, key splits, workspace floats), 8 heads of 16.
# stat = B * 8 * Lq * 2 floats everywhere; LANES adds 2 * chunks * B * Lk * 128 of partial dK / dV with
# chunks = min(2048 / (ceil(Lk / 256) * 8 * B), Lq / 256); WAVE below 2048 queries has Lq / 1024 < 2: one chunk, no partials.
BACKWARD_BEFORE = [
    ((2, 32400, 200, 0), (LANES, 126, 1, 1036800 + 2 * 126 * 400 * 128)),     # min(2048 / 16 = 128, 32400 / 256 = 126)
    ((2, 32400, 200, 1), (LANES, 126, 1, 1036800 + 2 * 126 * 400 * 128)),
    ((2, 200, 200, 0), (WAVE, 1, 1, 6400)),
    ((2, 200, 200, 1), (WAVE, 1, 1, 6400)),
    ((2, 200, 32400, 0), (WAVE, 1, 1, 6400)),
    ((1, 2047, 37, 0), (WAVE, 1, 1, 32752)),
    ((1, 2047, 37, 1), (WAVE, 1, 1, 32752)),
    ((1, 2048, 37, 0), (LANES, 8, 1, 32768 + 2 * 8 * 37 * 128)),              # min(2048 / 8 = 256, 2048 / 256 = 8)
    ((1, 2048, 37, 1), (LANES, 8, 1, 32768 + 2 * 8 * 37 * 128)),
    ((1, 4100, 37, 0), (LANES, 16, 1, 65600 + 2 * 16 * 37 * 128)),            # min(256, 4100 / 256 = 16)
    ((1, 4100, 37, 1), (LANES, 16, 1, 65600 + 2 * 16 * 37 * 128)),
    ((2, 300, 200, 1), (WAVE, 1, 1, 9600)),
    ((1, 256, 512, 1), (WAVE, 1, 1, 4096)),                                   # 512 keys with dropout ran before: as before
]
# the route that exists for dropout_p > 0, more than 512 keys, at most 256 queries -- calls that were refused before:
# ceil(Lk / 512) splits, + B * 8 * splits * Lq * 18 floats of partial rows; everything else on the kernels above
BACKWARD_NEW = [
    ((2, 200, 32400, 1), (KEYSPLIT, 1, 64, 6400 + 2 * 8 * 64 * 200 * 18)),
    ((2, 20, 1296, 1), (KEYSPLIT, 1, 3, 640 + 2 * 8 * 3 * 20 * 18)),
    ((1, 256, 513, 1), (KEYSPLIT, 1, 2, 4096 + 8 * 2 * 256 * 18)),
    ((1, 257, 513, 1), (WAVE, 1, 1, 4112)),
    ((1, 2100, 600, 1), (LANES, 8, 1, 33600 + 2 * 8 * 600 * 128)),            # min(2048 / (3 * 8) = 85, 2100 / 256 = 8)
    ((1, 256, 513, 0), (WAVE, 1, 1, 4096)),                                   # without dropout: never
    ((1, 16, 32400, 1), (KEYSPLIT, 1, 64, 256 + 8 * 64 * 16 * 18)),
]
# (B, Lq, Lk, head_dim) -> (keys per split, splits, workspace floats): one resident set up to 512 keys, else 512-key splits
# with B * 8 * splits * Lq * (head_dim + 2) floats of partial rows
FORWARD = [
    ((2, 200, 32400, 16), (512, 64, 2 * 8 * 64 * 200 * 18)),
    ((2, 32400, 200, 16), (200, 1, 0)),
    ((2, 200, 200, 16), (200, 1, 0)),
    ((1, 16, 512, 16), (512, 1, 0)),
    ((1, 16, 513, 16), (512, 2, 8 * 2 * 16 * 18)),
    ((2, 20, 1296, 16), (512, 3, 2 * 8 * 3 * 20 * 18)),
    ((1, 37, 1040, 32), (512, 3, 8 * 3 * 37 * 34)),
    ((1, 37, 300, 32), (300, 1, 0)),
]

SEEDS = (0x1234567890ABCDEF, 0, (1 << 62) - 1, (1 << 64) - 1)
P_KEEP = 0.3


def _thresh(p):
    t = float(p) * 4294967296.0
    return 4294967295 if t >= 4294967295.0 else int(t)


def _triples():
    """(bh, i, j): the head's largest indices, the largest legal value of each field, and a seeded few hundred"""
    top_i, top_bh = (1 << 24) - 1, (1 << 16) - 1
    t = [(15, 199, 32399), (0, 0, 0), (top_bh, 0, 0), (0, top_i, 0), (0, 0, top_i), (top_bh, top_i, top_i),
         (15, 199, 32398), (15, 198, 32399), (14, 199, 32399), (1, 0, 512), (1, 255, 513)]
    g = torch.Generator().manual_seed(5)
    bh = torch.randint(0, 1 << 16, (300,), generator=g).tolist()
    i = torch.randint(0, 1 << 24, (300,), generator=g).tolist()
    j = torch.randint(0, 1 << 24, (300,), generator=g).tolist()
    return t + list(zip(bh, i, j))


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """one compile, one run: the program's answer to every plan row and every hash triple"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("attention_plan")
    src = d / "plan.hip"
    src.write_text(SRC)
    exe = d / "plan"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "is-fusion_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    # seeds travel as signed 64-bit numbers (scanf %lld): the same bits
    signed = lambda s: s - (1 << 64) if s >= (1 << 63) else s
    rows = [("b",) + q + (0,) for q, _ in BACKWARD_BEFORE + BACKWARD_NEW] + [("f",) + q + (0,) for q, _ in FORWARD]
    rows += [("k", signed(s)) + t + (_thresh(P_KEEP),) for s in SEEDS for t in _triples()]
    out = subprocess.run([str(exe)], input="".join(" ".join(map(str, r)) + "\n" for r in rows), check=True,
                         capture_output=True, text=True).stdout.split("\n")
    assert len(out) >= len(rows)
    return {r: tuple(int(x) for x in ln.split()) for r, ln in zip(rows, out)}


def test_the_tables_hold_no_row_twice():
    for table in (BACKWARD_BEFORE + BACKWARD_NEW, FORWARD):
        assert len({q for q, _ in table}) == len(table)


_ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("query,expected", BACKWARD_BEFORE, ids=_ids)
def test_backward_of_an_existing_shape_keeps_its_kernels(answers, query, expected):
    assert answers[("b",) + query + (0,)] == expected


@pytest.mark.parametrize("query,expected", BACKWARD_NEW, ids=_ids)
def test_backward_takes_the_key_split_route_only_where_dropout_was_refused(answers, query, expected):
    assert answers[("b",) + query + (0,)] == expected


@pytest.mark.parametrize("query,expected", FORWARD, ids=_ids)
def test_forward_splits_keys_above_512(answers, query, expected):
    assert answers[("f",) + query + (0,)] == expected


def test_attn_keep_is_what_attention_keep_mask_restates(answers, monkeypatch):
    """the C++ hash, run on the host, against the torch restatement the GPU tests build their float64 masks from: the
    head's last (bh, query, key) = (15, 199, 32399), the largest legal value of every field, 300 seeded triples; four seeds"""
    from isfusion_amd import fusion_ops as ops
    signed = lambda s: s - (1 << 64) if s >= (1 << 63) else s
    kept = 0
    for s in SEEDS:
        small = ops.attention_keep_mask(s, 2, HEADS, 256, 514, P_KEEP)          # read directly where the triple lies inside
        for bh, i, j in _triples():
            got = answers[("k", signed(s), bh, i, j, _thresh(P_KEEP))][0]
            if bh < 2 * HEADS and i < 256 and j < 514:
                want = small[bh // HEADS, bh % HEADS, i, j].item()
            else:
                want = _one(ops, monkeypatch, s, bh, i, j)
            assert bool(got) == bool(want), (hex(s), bh, i, j)
            kept += got
    rate = kept / (len(SEEDS) * len(_triples()))
    assert abs(rate - (1 - P_KEEP)) < 0.05, rate


def _one(ops, monkeypatch, seed, bh, i, j):
    """attention_keep_mask at one large (bh, i, j) without a [.., i + 1, j + 1] tensor: the function takes its three index
    ranges from torch.arange, in the order bh, query, key -- hand it ranges of the one index each"""
    want = iter((bh, i, j))
    with monkeypatch.context() as mp:
        mp.setattr(torch, "arange", lambda n, **kw: torch.tensor([next(want)], **kw))
        return ops.attention_keep_mask(seed, 1, 1, 1, 1, P_KEEP).item()
