"""One clipped optimizer step on the real ISFusionPtsPath parameter set (312 tensors, 19.2 M fp32 parameters), the
reference's recipe (mmcv per-parameter groups: 312 groups; AdamW; global L2 clip at 0.01):

    python tools/optim_bench.py [--steps 50] [--warmup 5]

  fused        isfusion_amd.optim.FusedAdamW.step(grad_clip=...)        (2 HIP launches)
  torch        torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW(foreach=True) on the same 312 groups
  torch_fused  the same with AdamW(fused=True), if this torch build runs it

Per setup: device ms per step (events around `steps` back-to-back steps), host ms per step (wall time of the calls
alone, before the synchronize), GPU operations per step (torch.profiler, one step) and the achieved bandwidth of the
32 B / parameter model (read g for the norm; read p, g, m, v; write p, m, v) against the 6.29 TB/s measured copy rate.
Gradients are kept between steps (DDP bucket views are).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_TBPS = 6.29
CFG = dict(type="AdamW", lr=0.0001, weight_decay=0.01, paramwise_cfg=dict(custom_keys={"img_backbone": dict(lr_mult=0.1)}))
CLIP = dict(max_norm=0.01, norm_type=2)


def measure(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    host = (time.perf_counter() - t0) / steps
    e1.record()
    torch.cuda.synchronize()
    dev = e0.elapsed_time(e1) / steps
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
           and not e.name.startswith("Optimizer.")]                    # the step's annotation on the GPU timeline
    copies = [e for e in evs if "memcpy" in e.name.lower()]
    kernels = [e for e in evs if "memcpy" not in e.name.lower()]
    busy = sum(e.time_range.elapsed_us() for e in evs) / 1e3
    names = sorted({e.name[:60] for e in kernels})
    return dict(device_ms=round(dev, 4), host_ms=round(host * 1e3, 4), kernels=len(kernels), copies=len(copies),
                kernel_ms=round(busy, 4), kernel_names=names[:6])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from isfusion_amd import optim
    from isfusion_amd.detector import ISFusionPtsPath
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = ISFusionPtsPath().to(dev)
    n_params = sum(p.numel() for p in net.parameters())
    gen = torch.Generator(device=dev).manual_seed(1)
    out = dict(tensors=len(list(net.parameters())), parameters=n_params, bytes_per_param=32, copy_tbps=COPY_TBPS)

    def fresh():
        ps = [p.detach().clone().requires_grad_() for p in net.parameters()]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen, device=dev)
        return ps

    def groups(ps):
        proto = optim.build_optimizer(net, CFG)
        return [dict(params=[q], lr=g["lr"], weight_decay=g["weight_decay"]) for g, q in zip(proto.param_groups, ps)]

    ps = fresh()
    fused = optim.FusedAdamW(groups(ps), lr=1e-4, weight_decay=0.01)
    out["fused"] = measure(lambda: fused.step(grad_clip=CLIP), a.steps, a.warmup)
    out["groups"] = len(fused.param_groups)
    del fused, ps
    for name, kw in (("torch", dict(foreach=True)), ("torch_fused", dict(fused=True))):
        ps = fresh()
        try:
            opt = torch.optim.AdamW(groups(ps), lr=1e-4, weight_decay=0.01, **kw)

            def step():
                torch.nn.utils.clip_grad_norm_(ps, CLIP["max_norm"])
                opt.step()
            out[name] = measure(step, a.steps, a.warmup)
        except Exception as e:                                   # fused=True may not be built for this ROCm
            out[name] = dict(error=f"{type(e).__name__}: {str(e)[:200]}")
        del ps
    for name in ("fused", "torch", "torch_fused"):
        r = out[name]
        if "device_ms" in r:
            r["achieved_tbps"] = round(32 * n_params / (min(r["device_ms"], r["kernel_ms"]) * 1e-3) / 1e12, 3)
            r["fraction_of_copy_rate"] = round(r["achieved_tbps"] / COPY_TBPS, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
