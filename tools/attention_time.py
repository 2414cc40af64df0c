"""Time of the detection head's cross attention (200 queries x 32400 keys, 8 heads of 16, B = 2) through the attention
cores, and the forward's error against a float64 softmax attention on a few queries.

    python tools/attention_time.py [--dropout P] [--backward] [--lib path/to/libisf_hip.so] [--batch 2] [--queries 200] [--keys 32400]

  --dropout P   isf_attention_forward_dropout / isf_attention_backward_dropout with probability P (the head's decoder
                layer: 0.1) instead of the plain entries; the float64 check then applies fusion_ops.attention_keep_mask
  --backward    also time the backward alone (torch.autograd.grad on a retained graph)
  --lib         another build of the library (tools/probes/build_side_lib.sh), e.g. one without the key-split backward route

Every figure is the median of 30 single calls between device events after 5 untimed ones, three runs in this one
process.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

E, HEADS, CALLS, WARMUP, RUNS = 128, 8, 30, 5, 3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3            # us


def median_us(fn):
    for _ in range(WARMUP):
        fn()
    return round(statistics.median(timed(fn) for _ in range(CALLS)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dropout", type=float, default=0.0)
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--lib", default="")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--queries", type=int, default=200)
    ap.add_argument("--keys", type=int, default=32400)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attention_time.py measures on the GPU: no device found")
    from isfusion_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from isfusion_amd import fusion_ops as ops
    dev = torch.device("cuda", 0)
    B, P, HW, p, seed = a.batch, a.queries, a.keys, a.dropout, 0x1234567890ABCDEF
    g = torch.Generator().manual_seed(0)
    q = torch.randn((B * P, E), generator=g).to(dev).requires_grad_()
    k = torch.randn((B * HW, E), generator=g).to(dev).requires_grad_()
    v = torch.randn((B * HW, E), generator=g).to(dev).requires_grad_()
    go = torch.randn((B * P, E), generator=g).to(dev)
    forward = lambda: ops.AttentionFunction.apply(q, k, v, B, P, HW, E, HEADS, p, seed)
    res = dict(device=torch.cuda.get_device_name(0), lib=a.lib or "in-tree", batch=B, queries=P, keys=HW, dropout=p,
               calls=CALLS, runs=RUNS)
    with torch.no_grad():
        res["forward_us"] = [median_us(forward) for _ in range(RUNS)]
        out = forward()
    if a.backward:
        kept = forward()
        backward = lambda: torch.autograd.grad(kept, (q, k, v), go, retain_graph=True)
        res["backward_us"] = [median_us(backward) for _ in range(RUNS)]
    # fp64 reference on a few queries
    n = min(8, P)
    qd = q.detach().double().view(B, P, HEADS, 16)[:, :n]
    kd, vd = k.detach().double().view(B, HW, HEADS, 16), v.detach().double().view(B, HW, HEADS, 16)
    prob = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", qd, kd) / 4.0, -1)
    if p > 0.0:
        prob = prob * ops.attention_keep_mask(seed, B, HEADS, n, HW, p, device=dev).double() / (1.0 - p)
    o = torch.einsum("bhqk,bkhd->bqhd", prob, vd).reshape(B, n, E)
    res["forward_max_err_vs_fp64"] = (out.view(B, P, E)[:, :n].double() - o).abs().max().item()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
