"""Worker of tests/test_gpu_optim_shard_module.py: one rank of a process group whose ranks ALL drive cuda:0 (the GPU box has one
GPU: two ranks over gloo, or one rank over nccl so that RCCL's reduce_scatter_tensor / all_gather_into_tensor run once).  Every
rank can compute every rank's gradients from (rank, step), so what the reduce-scatter must deliver needs no second collective.

    RANK=r WORLD_SIZE=W MASTER_ADDR=... MASTER_PORT=... python tests/optim_shard_worker.py gloo|nccl

Exit code 0 and a last line "rank r: sharded optimizer OK" = every check held."""
import datetime
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import optim_ref as R  # noqa: E402

SHAPES = ((33,), (8, 16), (4097,), (3, 4096), (64,))          # a shard boundary falls inside the fourth tensor at W = 2
LR, WDS = 1e-3, (0.1, 0.0)
HYPER = R.Hyper(0.9, 0.999, 1e-8, 1.0)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def make_params(dev):
    g = torch.Generator().manual_seed(11)
    return [torch.nn.Parameter((0.02 * torch.randn(s, generator=g)).to(device=dev, dtype=torch.bfloat16)) for s in SHAPES]


def groups_of(params):
    return [{"params": [p for p in params if p.dim() >= 2], "weight_decay": WDS[0]},
            {"params": [p for p in params if p.dim() < 2], "weight_decay": WDS[1]}]


def grads_of(rank, step, dev):
    g = torch.Generator().manual_seed(1000 * step + 17 * rank + 5)
    return [(0.1 * torch.randn(s, generator=g)).to(dev) for s in SHAPES]


def before_of(opt, params, sd, summed):
    """The state a step starts from, per tensor in the optimizer's (group) order, for tests/optim_ref.py."""
    out = []
    order = [p for group in opt.param_groups for p in group["params"]]
    for i, p in enumerate(order):
        k = [id(q) for q in params].index(id(p))
        st = sd["state"][i]
        group = opt.param_groups[0 if p.dim() >= 2 else 1]
        out.append({"p": st["master"].flatten().clone(), "m": st["exp_avg"].flatten().clone(), "v": st["exp_avg_sq"].flatten().clone(),
                    "g": summed[k].flatten().clone(), "lr": group["lr"], "wd": group["weight_decay"], "param": p})
    return out


def check_against(ref, bounds, sd, before, what, scale=1.0):
    for i, (t, (p2, m2, v2), (ep, em, ev)) in enumerate(zip(before, ref["out"], bounds)):
        st = sd["state"][i]
        for name, a, b, e in (("master", st["master"], p2, ep), ("exp_avg", st["exp_avg"], m2, em), ("exp_avg_sq", st["exp_avg_sq"], v2, ev)):
            r = R.worst_ratio(a.flatten(), b, scale * e)
            assert r <= 1.0, f"{what} tensor {i} {name}: |got - ref| / bound = {r:.3f}"
        assert torch.equal(bits(t["param"].detach()), bits(R.cast_ref(st["master"], torch.bfloat16))), f"{what} tensor {i}: param != cast(master)"


def main():
    from tokenpacker_amd import ShardedMainGradAdamW
    backend = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    kw = {"device_id": dev} if backend == "nccl" else {}
    dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60), **kw)
    solo = [dist.new_group([r]) for r in range(world)][rank]           # (every rank creates every group, and keeps its own)
    scale = 1.0 / world

    params = make_params(dev)
    opt = ShardedMainGradAdamW(groups_of(params), lr=LR)
    assert (opt.world, opt.rank) == (world, rank)
    lay, S = opt.layout, opt.layout["shard"]
    for p in params:
        assert p.main_grad.untyped_storage().data_ptr() == opt.flat_grad.untyped_storage().data_ptr()
        assert p.untyped_storage().data_ptr() == opt.flat_param.untyped_storage().data_ptr()
    order = [p for group in opt.param_groups for p in group["params"]]          # the layout's tensor order
    pos = {id(p): k for k, p in enumerate(params)}

    def one_step(step, poison=None):
        every = [grads_of(r, step, dev) for r in range(world)]
        if poison is not None:
            every[world - 1][2][7] = poison                          # the LAST rank's gradient only
        for p, g in zip(params, every[rank]):
            p.main_grad.copy_(g)
        summed = [sum((every[r][k] for r in range(1, world)), every[0][k]) for k in range(len(params))]      # fp32, rank order
        opt.step()
        if poison is None:                                           # (a NaN's payload is nobody's contract)
            flat = torch.zeros(lay["total"], dtype=torch.float32, device=dev)
            for p, off in zip(order, lay["offsets"]):
                flat[off:off + p.numel()] = summed[pos[id(p)]].flatten()
            assert torch.equal(bits(opt.grad_shard), bits(flat[rank * S:(rank + 1) * S])), \
                f"rank {rank} step {step}: grad_shard is not the fp32 sum of the ranks' gradients"
        assert not bool(opt.flat_grad.any()), "flat_grad is zeroed behind the step"
        return summed

    def same_on_every_rank(what):
        mine = int(bits(opt.flat_param).long().sum())
        seen = [None] * world
        dist.all_gather_object(seen, mine)
        assert all(v == mine for v in seen), f"{what}: the ranks hold different parameters"

    # 1. two clean steps against the reference on the reduced gradient, scale 1 / W
    for step in range(2):
        sd = opt.consolidated_state_dict()
        every = [grads_of(r, step, dev) for r in range(world)]
        summed = [sum((every[r][k] for r in range(1, world)), every[0][k]) for k in range(len(params))]
        before = before_of(opt, params, sd, summed)
        one_step(step)
        ref = R.step_ref(before, HYPER, step, scale)
        assert int(opt.found_inf) == 0 and int(opt.steps_applied) == step + 1
        norm = float(opt.grad_norm.double())
        assert abs(norm ** 2 - ref["norm"] ** 2) <= R.SUMSQ_REL * ref["norm"] ** 2
        assert float(opt.clip_coef) < 1.0
        check_against(ref, R.bounds(before, HYPER, step, ref, scale), opt.consolidated_state_dict(), before, f"rank {rank} step {step}")
        same_on_every_rank(f"step {step}")

    # 2. a NaN in ONE rank's gradient skips the step on all
    sd = opt.consolidated_state_dict()
    params_before = opt.flat_param.clone()
    one_step(2, poison=float("nan"))
    assert (int(opt.found_inf), int(opt.steps_applied), int(opt.steps_skipped)) == (1, 2, 1), f"rank {rank}: the step was not skipped"
    after = opt.consolidated_state_dict()
    assert torch.equal(bits(opt.flat_param), bits(params_before))
    for i in sd["state"]:
        for k in ("master", "exp_avg", "exp_avg_sq"):
            assert torch.equal(bits(sd["state"][i][k]), bits(after["state"][i][k])), f"{k} of a skipped step changed"

    # 3. the consolidated state into a fresh ONE-rank optimizer: one more step with the summed gradient (inv_scale = 1 / W takes
    #    the average) against the W ranks continuing
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in params]
    solo_opt = ShardedMainGradAdamW(groups_of(fresh), lr=7.0, process_group=solo)
    assert solo_opt.world == 1
    solo_opt.load_state_dict(after)
    assert int(solo_opt.steps_applied) == 2 and int(solo_opt.steps_skipped) == 1 and solo_opt.param_groups[0]["lr"] == LR
    step = 3
    every = [grads_of(r, step, dev) for r in range(world)]
    summed = [sum((every[r][k] for r in range(1, world)), every[0][k]) for k in range(len(params))]
    before = before_of(opt, params, after, summed)
    one_step(step)
    for p, g in zip(fresh, summed):
        p.main_grad.copy_(g)
    solo_opt.step(inv_scale=torch.tensor([scale], dtype=torch.float32, device=dev))
    ref = R.step_ref(before, HYPER, 2, scale)
    bounds = R.bounds(before, HYPER, 2, ref, scale)
    many, one = opt.consolidated_state_dict(), solo_opt.consolidated_state_dict()
    assert int(opt.steps_applied) == int(solo_opt.steps_applied) == 3
    check_against(ref, bounds, many, before, f"rank {rank}: {world} ranks continuing")
    check_against(ref, bounds, one, [dict(t, param=q) for t, q in zip(before, [f for group in solo_opt.param_groups for f in group["params"]])],
                  f"rank {rank}: one rank resumed")
    for i, (ep, em, ev) in enumerate(bounds):                          # ... and against each other
        for k, e in (("master", ep), ("exp_avg", em), ("exp_avg_sq", ev)):
            r = R.worst_ratio(one["state"][i][k].flatten(), many["state"][i][k].flatten().double(), e)
            assert r <= 1.0, f"rank {rank}: resumed on one rank vs {world} ranks, tensor {i} {k}: {r:.3f}"
    # a sharded state dict is for its own layout only
    if world > 1:
        try:
            solo_opt.load_state_dict(opt.state_dict())
            raise SystemExit("a two-rank sharded state dict loaded into a one-rank optimizer")
        except ValueError as e:
            assert "world" in str(e), e
    opt.load_state_dict(opt.state_dict())                              # ... and round-trips into it
    same_on_every_rank("the end")
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()
    print(f"rank {rank}: sharded optimizer OK", flush=True)


if __name__ == "__main__":
    main()
