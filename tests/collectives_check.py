"""Three-rank check of the deterministic mode across ranks (run by tests/test_gpu_collectives.py under
torch.distributed.run, gloo backend, every rank on cuda:0).  Linear(16, 64) -> NaiveSyncBatchNorm1d through norm.bn1d_relu
(the fused path; the row count differs per data index) -> Linear(64, 8) in DistributedDataParallel, three SGD steps:

  mode on   forward under ddp.no_sync(), exact_all_reduce_gradients after backward, the sync-BN sums through the exact
            all_reduce_sum_;
  mode off  DDP's own bucketed all-reduce and dist.all_reduce, as before;

each with the data dealt to the ranks in the order 0,1,2 and in the order 2,0,1.  Rank 0 prints per (mode, order) one
digest of parameters, BN buffers and the last step's reduced gradients, and per mode the largest gradient error against a
float64 single-process restatement of the three ranks' steps."""
import hashlib
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORLD, STEPS, LR, EPS, MOM = 3, 3, 0.05, 1e-3, 0.01
ORDERS = ((0, 1, 2), (2, 0, 1))


def data(index, step):
    """the share of data index `index` at `step`: x [n, 16], target [n, 8]; n differs per index"""
    g = torch.Generator().manual_seed(1000 + 10 * step + index)
    n = 37 + 13 * index
    scale = torch.exp2(torch.randint(-6, 3, (n, 1), generator=g).float())           # rows of mixed magnitude
    return torch.randn(n, 16, generator=g) * scale + 0.25, torch.randn(n, 8, generator=g)


def initial_state():
    g = torch.Generator().manual_seed(5)
    return {"fc1.weight": torch.randn(64, 16, generator=g) * 0.25, "fc1.bias": torch.randn(64, generator=g) * 0.1,
            "bn.weight": torch.rand(64, generator=g) + 0.5, "bn.bias": torch.randn(64, generator=g) * 0.1,
            "fc2.weight": torch.randn(8, 64, generator=g) * 0.125, "fc2.bias": torch.randn(8, generator=g) * 0.1}


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from isfusion_amd import norm
        self.fc1 = torch.nn.Linear(16, 64)
        self.bn = norm.NaiveSyncBatchNorm1d(64, eps=EPS, momentum=MOM)
        self.fc2 = torch.nn.Linear(64, 8)
        self.load_state_dict(initial_state(), strict=False)

    def forward(self, x):
        from isfusion_amd import norm
        return self.fc2(norm.bn1d_relu(self.bn, self.fc1(x)))


def reference_gradients():
    """float64, one process: the three ranks' rows through the same net -- sync-BN statistics = the equal-weight average of
    the per-rank mean / mean of squares (the reference's naiveSyncBN1d), gradient = the mean over the ranks of the
    gradients of the per-rank mean-square losses -- with the same SGD steps.  -> per step {name: gradient}"""
    p = {k: v.double().requires_grad_() for k, v in initial_state().items()}
    out = []
    for step in range(STEPS):
        hs, ts = [], []
        for index in range(WORLD):
            x, t = data(index, step)
            hs.append(x.double() @ p["fc1.weight"].T + p["fc1.bias"])
            ts.append(t.double())
        mean = sum(h.mean(0) for h in hs) / WORLD
        meansqr = sum((h * h).mean(0) for h in hs) / WORLD
        scale = p["bn.weight"] * torch.rsqrt(meansqr - mean * mean + EPS)
        loss = 0.0
        for h, t in zip(hs, ts):
            y = torch.relu((h - mean) * scale + p["bn.bias"]) @ p["fc2.weight"].T + p["fc2.bias"]
            loss = loss + ((y - t) ** 2).mean()
        grads = torch.autograd.grad(loss / WORLD, list(p.values()))
        out.append({k: g for k, g in zip(p, grads)})
        with torch.no_grad():
            for v, g in zip(p.values(), grads):
                v -= LR * g
    return out


def run(rank, dev, exact, order):
    """three steps with rank r on the data of index order[r] -> (digest, per step {name: reduced gradient})"""
    import isfusion_amd
    from isfusion_amd.collectives import exact_all_reduce_gradients
    import contextlib
    isfusion_amd.set_deterministic(exact)
    net = Net().to(dev).train()
    ddp = torch.nn.parallel.DistributedDataParallel(net, device_ids=[0], gradient_as_bucket_view=True)
    opt = torch.optim.SGD(net.parameters(), lr=LR)
    steps = []
    for step in range(STEPS):
        x, t = (v.to(dev) for v in data(order[rank], step))
        with ddp.no_sync() if exact else contextlib.nullcontext():
            loss = ((ddp(x) - t) ** 2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if exact:
            exact_all_reduce_gradients(net)
        steps.append({k: p.grad.detach().clone() for k, p in net.named_parameters()})
        opt.step()
    isfusion_amd.set_deterministic(False)
    h = hashlib.sha256()
    for k, v in list(net.state_dict().items()) + sorted(steps[-1].items()):
        h.update(k.encode())
        h.update(v.detach().cpu().numpy().tobytes())
    return h.hexdigest(), steps


def refusals(dev):
    """what must raise in a multi-rank job: a listed parameter without a gradient (named), a CPU tensor in the exact sum"""
    from isfusion_amd.collectives import all_reduce_sum_, exact_all_reduce_gradients
    from isfusion_amd._lib import IsfError
    p = torch.nn.Parameter(torch.zeros(4, device=dev))
    try:
        exact_all_reduce_gradients([("lonely.weight", p)])
        return False
    except IsfError as e:
        if "lonely.weight" not in str(e):
            return False
    try:
        all_reduce_sum_(torch.zeros(4), True)
        return False
    except IsfError:
        return True


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert world == WORLD
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    ref = reference_gradients() if rank == 0 else None
    refused = refusals(dev)
    for exact in (True, False):
        mode, worst = "on" if exact else "off", 0.0
        for order in ORDERS:
            digest, steps = run(rank, dev, exact, order)
            same = torch.tensor([1], dtype=torch.int32)                   # every rank holds the same reduced gradients
            for k, g in sorted(steps[-1].items()):
                rows = [torch.empty_like(g) for _ in range(world)]
                dist.all_gather(rows, g)
                if not all(torch.equal(r, rows[0]) for r in rows):
                    same[0] = 0
            dist.all_reduce(same, op=dist.ReduceOp.MIN)
            if rank == 0:
                for got, want in zip(steps, ref):
                    for k, g in got.items():
                        worst = max(worst, float((g.double().cpu() - want[k]).abs().max()))
                print(f"COLLECTIVES_DIGEST {mode} {','.join(map(str, order))} {digest} ranks_agree {int(same[0])}")
        if rank == 0:
            top = max(float(g.abs().max()) for step in ref for g in step.values())
            print(f"COLLECTIVES_GRAD_ERR {mode} {worst:.6e} max_ref {top:.6e}")
    if rank == 0:
        print(f"COLLECTIVES_REFUSALS {int(refused)}")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
