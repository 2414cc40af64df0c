"""ChannelAttentionFunction (A14, training) with its two backwards, in one process on one GPU:

    python tools/channel_attention_bench.py [--calls 30] [--warmup 5] [--batches 2 4]

  hip    isf_channel_attention_backward (isf_channel_attn_bwd.hip: two launches, probabilities recomputed on the matrix cores)
  torch  fusion_train.channel_attention_backward_reference (five rocBLAS batched GEMMs + elementwise passes), the backward
         the Function had before the kernels: here a subclass of the Function with that backward

Per batch size B (B * 128 maps of 180 x 180, seeded randn * 0.3 inputs and randn output gradient) and per backward:
  fwd_bwd_ms       forward + backward of ChannelAttentionFunction, device-event time per call
  bwd_ms           the backward alone (torch.autograd.grad on a retained graph), device-event time per call
                   both: median of `calls` single calls after `warmup` untimed ones; the two backwards ALTERNATE call by
                   call, so clock and neighbour effects fall on both
  bwd_peak_mb      torch.cuda.max_memory_allocated during one backward over what was resident before it (inputs, saved
                   tensors, output gradient): the torch allocator's temporaries AND the two gradients
  workspace_mb     the library's own stream workspace after the calls (isf_workspace_bytes: whole arena blocks, not torch's
                   allocator) -- the hip backward's P / gS scratch lives there; nothing else in this process uses it
and max_abs_diff: the largest difference between the two backwards' gradients (same inputs).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHANNELS, SIZE = 128, 180
MODES = ("hip", "torch")


def workspace_bytes():
    from isfusion_amd import _lib
    n = ctypes.c_size_t(0)
    _lib.check(_lib.load().isf_workspace_bytes(ctypes.byref(n)), "isf_workspace_bytes")
    return n.value


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(B, calls, warmup):
    from isfusion_amd import fusion_train as tr
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(B)
    shape = (B, CHANNELS, SIZE, SIZE)
    qs = (torch.randn(shape, generator=gen, device=dev) * 0.3).requires_grad_()
    qi = (torch.randn(shape, generator=gen, device=dev) * 0.3).requires_grad_()
    g = torch.randn(shape, generator=gen, device=dev)

    class TorchBackward(tr.ChannelAttentionFunction):        # the same forward and saved tensors
        @staticmethod
        @tr._amp_bwd
        def backward(ctx, go):
            return tr.channel_attention_backward_reference(*ctx.saved_tensors, go.contiguous().float())

    functions = dict(hip=tr.ChannelAttentionFunction, torch=TorchBackward)

    def forward(mode):
        return functions[mode].apply(qs, qi)

    def fwd_bwd(mode):
        forward(mode).backward(g)
        qs.grad = qi.grad = None

    outs = {m: forward(m) for m in MODES}                    # retained graphs for the backward-alone timing
    bwd = lambda mode: torch.autograd.grad(outs[mode], (qs, qi), g, retain_graph=True)
    res = {m: {} for m in MODES}
    for key, fn in (("bwd_ms", bwd), ("fwd_bwd_ms", fwd_bwd)):
        samples = {m: [] for m in MODES}
        for i in range(warmup + calls):
            for m in MODES:
                ms = timed(lambda: fn(m))
                if i >= warmup:
                    samples[m].append(ms)
        for m in MODES:
            res[m][key] = round(statistics.median(samples[m]), 4)
            res[m][key + "_min"] = round(min(samples[m]), 4)
    grads = {}
    for m in MODES:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        resident = torch.cuda.memory_allocated()
        grads[m] = bwd(m)
        torch.cuda.synchronize()
        res[m]["bwd_peak_mb"] = round((torch.cuda.max_memory_allocated() - resident) / 2 ** 20, 1)
        res[m]["workspace_mb"] = round(workspace_bytes() / 2 ** 20, 1) if m == "hip" else 0.0
    diff = max((a - b).abs().max().item() for a, b in zip(grads["hip"], grads["torch"]))
    return dict(maps=B * CHANNELS, size=SIZE, max_abs_diff=diff, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 4])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("channel_attention_bench.py measures on the GPU: no device found")
    out = dict(device=torch.cuda.get_device_name(0), calls=a.calls, warmup=a.warmup)
    for B in a.batches:
        out[f"B{B}"] = measure(B, a.calls, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
