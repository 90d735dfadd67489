"""tp_optim_sumsq / tp_optim_apply on the GPU, through the C ABI: ONE process plays the W ranks of a sharded optimizer in turn, with
no collective — the flat buffers of every array hold all shards, rank r's table points at its slices (``shard_slices``), every rank
has its own state block, and the "all-gather" of the W sums of squares is the tensor the W ``tp_optim_sumsq`` calls wrote into.

Checked: W = 1 with grad_scale = 1 IS tp_optim_step, bit for bit (bf16, fp16, fp32); W in {2, 3, 8} against tests/optim_ref.py (norm,
elementwise bounds, param the cast of the master, every rank the same state block); grad_scale against inv_scale; a NaN / inf in one
shard skips all; an empty shard; reproducibility; the argument checks.  Shapes: one element up to a few chunks (shard boundaries
inside tensors), 33 tensors (two launches), and an unaligned layout (slices off 16-byte boundaries: the scalar path)."""
import ctypes

import pytest
import torch

from tests import optim_ref as R
from tokenpacker_amd import _capi, shard_layout, shard_slices

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {torch.bfloat16: _capi.TP_BF16, torch.float16: _capi.TP_F16, torch.float32: _capi.TP_F32}
NUMELS = (1, 3, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 4, 70_000)
TABLES = {   # name: (numels, align)
    "sizes": (NUMELS, 64),
    "table_of_33": (tuple(NUMELS[i % 9] for i in range(33)), 64),
    "unaligned": (NUMELS, 1),
}
assert len(TABLES["table_of_33"][0]) > R.TABLE
HYPER = R.Hyper(0.9, 0.999, 1e-8, 1.0)
WORDS = _capi.TP_OPTIM_STATE_BYTES // 4


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


class Ranks:
    """W ranks over one flat index space: master / grad / exp_avg / exp_avg_sq (fp32) and param (dtype; fp32: the master is the
    parameter and there is none), a table and a state block per rank."""

    def __init__(self, table, dtype, world, seed=3):
        numels, align = TABLES[table] if isinstance(table, str) else table
        self.numels, self.dtype, self.world, self.seed = tuple(numels), dtype, world, seed
        self.layout = lay = shard_layout(numels, world, align=align)
        self.own_master = dtype == torch.float32
        total = lay["total"]
        self.flat = {k: torch.zeros(total, dtype=torch.float32, device=DEV) for k in ("p", "g", "m", "v")}
        self.flat["param"] = None if self.own_master else torch.zeros(total, dtype=dtype, device=DEV)
        self.tensors = R.make_tensors(numels, seed, device=DEV, param_dtype=torch.bfloat16 if self.own_master else dtype)
        for t, off in zip(self.tensors, lay["offsets"]):
            n = t["p"].numel()
            self.flat["p"][off:off + n].copy_(t["p"])
            for k in ("p", "g", "m", "v"):
                t[k] = self.flat[k][off:off + n]
            t["param"] = None if self.own_master else self.flat["param"][off:off + n]
            if t["param"] is not None:
                t["param"].copy_(t["p"])
        lib = _capi.load_library()
        self.tables, self.workspaces = [], []
        for r in range(world):
            sl = shard_slices(lay, r)
            tab = (_capi.tp_optim_tensor * max(len(sl), 1))()
            for e, (i, start, length, off) in zip(tab, sl):
                at = r * lay["shard"] + off
                assert at == lay["offsets"][i] + start
                e.param = None if self.own_master else self.flat["param"].data_ptr() + at * self.flat["param"].element_size()
                e.master, e.grad, e.exp_avg, e.exp_avg_sq = (self.flat[k].data_ptr() + 4 * at for k in ("p", "g", "m", "v"))
                e.numel, e.lr, e.weight_decay = length, self.tensors[i]["lr"], self.tensors[i]["wd"]
            self.tables.append((tab, len(sl)))
            nbytes = lib.tp_optim_workspace_bytes(tab, len(sl)) if sl else 0
            self.workspaces.append(torch.empty(nbytes, dtype=torch.uint8, device=DEV) if sl else None)
        self.states = torch.zeros(world, WORDS, dtype=torch.int32, device=DEV)
        self.sums = torch.full((world,), 7.0, dtype=torch.float64, device=DEV)
        ws = lib.tp_optim_workspace_bytes(*self.tables[0]) if world == 1 else 0
        self.step_workspace = torch.empty(ws, dtype=torch.uint8, device=DEV) if ws else None

    def set_grads(self, step, kind="above", scale=1.0):
        for t, g in zip(self.tensors, R.make_grads(self.numels, self.seed, step, kind, device=DEV)):
            t["g"].copy_(g * scale)

    def snapshot(self):
        return [{k: (t[k].clone() if isinstance(t[k], torch.Tensor) else t[k]) for k in ("p", "m", "v", "g", "param", "lr", "wd")}
                for t in self.tensors]

    def hyper(self):
        return _capi.tp_optim_hyper(HYPER.beta1, HYPER.beta2, HYPER.eps, HYPER.max_grad_norm, DT[self.dtype], 0)

    def sumsq(self, r, inv_scale=None, grad_scale=1.0):
        tab, n = self.tables[r]
        ws = self.workspaces[r]
        return _capi.load_library().tp_optim_sumsq(tab, n, None if inv_scale is None else inv_scale.data_ptr(), grad_scale,
                                                   self.sums[r:].data_ptr(), None if ws is None else ws.data_ptr(),
                                                   0 if ws is None else ws.numel(), torch.cuda.current_stream().cuda_stream)

    def apply(self, r, inv_scale=None, grad_scale=1.0):
        tab, n = self.tables[r]
        h = self.hyper()
        return _capi.load_library().tp_optim_apply(tab, n, ctypes.byref(h), None if inv_scale is None else inv_scale.data_ptr(),
                                                   grad_scale, self.sums.data_ptr(), self.world, self.states[r].data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)

    def step(self, inv_scale=None, grad_scale=1.0):
        """Every rank's sum of squares, then (the gather being the shared tensor) every rank's update.  -> rank 0's state words"""
        for r in range(self.world):
            _capi.check(self.sumsq(r, inv_scale, grad_scale), "tp_optim_sumsq")
        for r in range(self.world):
            _capi.check(self.apply(r, inv_scale, grad_scale), "tp_optim_apply")
        torch.cuda.synchronize()
        return self.read_state()

    def fused_step(self, inv_scale=None):
        """tp_optim_step on the same table (world 1 only)."""
        assert self.world == 1
        tab, n = self.tables[0]
        h = self.hyper()
        rc = _capi.load_library().tp_optim_step(tab, n, ctypes.byref(h), None if inv_scale is None else inv_scale.data_ptr(),
                                                self.states[0].data_ptr(), self.step_workspace.data_ptr(), self.step_workspace.numel(),
                                                torch.cuda.current_stream().cuda_stream)
        _capi.check(rc, "tp_optim_step")
        torch.cuda.synchronize()
        return self.read_state()

    def read_state(self):
        words = self.states.cpu()
        for r in range(1, self.world):
            assert torch.equal(words[r], words[0]), f"rank {r}'s state block differs from rank 0's"
        f = words[0].view(torch.float32)
        return {"norm": f[0].clone(), "coef": f[1].clone(), "found_inf": int(words[0][2]), "step": int(words[0][3]),
                "skipped": int(words[0][4])}

    def same_bits(self, other, what=""):
        for k in ("p", "m", "v", "param"):
            if self.flat[k] is not None:
                assert torch.equal(bits(self.flat[k]), bits(other.flat[k])), (what, k)
        assert torch.equal(self.states.cpu()[0], other.states.cpu()[0]), (what, "state block")


def check_step(run, before, got, step_before, scale, what):
    ref = R.step_ref(before, HYPER, step_before, scale)
    assert got["found_inf"] == 0 == ref["found_inf"] and got["step"] == ref["step"], (what, got)
    norm = float(got["norm"].double())
    print(f"{what}: norm {norm:.9g} (ref {ref['norm']:.9g}), |norm^2 - ref| / ref = "
          f"{abs(norm ** 2 - ref['norm'] ** 2) / ref['norm'] ** 2 / R.U32:.2f} u of {R.SUMSQ_REL / R.U32:.0f} u")
    assert abs(norm ** 2 - ref["norm"] ** 2) <= R.SUMSQ_REL * ref["norm"] ** 2, what
    worst = {}
    for i, (t, (p2, m2, v2), (ep, em, ev)) in enumerate(zip(run.tensors, ref["out"], R.bounds(before, HYPER, step_before, ref, scale))):
        for name, a, b, e in (("master", t["p"], p2, ep), ("exp_avg", t["m"], m2, em), ("exp_avg_sq", t["v"], v2, ev)):
            r = R.worst_ratio(a, b, e)
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, f"{what} tensor {i} ({t['p'].numel()} elements) {name}: |got - ref| / bound = {r:.3f}"
        if t["param"] is not None:
            assert torch.equal(bits(t["param"]), bits(R.cast_ref(t["p"], run.dtype))), f"{what} tensor {i}: param is not the cast of master"
    print(f"{what}: worst |got - ref| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("table", list(TABLES))
def test_one_rank_is_tp_optim_step_bit_for_bit(table, dtype):
    split, fused = Ranks(table, dtype, 1), Ranks(table, dtype, 1)
    for step in range(3):
        for run in (split, fused):
            run.set_grads(step)
        a, b = split.step(), fused.fused_step()
        assert a["step"] == b["step"] == step + 1 and float(a["coef"]) < 1.0
        split.same_bits(fused, f"{table} step {step}")
    assert torch.equal(bits(split.flat["g"]), bits(fused.flat["g"])) and bool(split.flat["g"].any())    # (flags 0: not zeroed)


@pytest.mark.parametrize("scale", [1.0, 0.5], ids=["sum", "scaled"])
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("table", list(TABLES))
def test_shards_match_the_reference(table, world, scale):
    run = Ranks(table, torch.bfloat16, world)
    assert sum(n for _, n in run.tables) >= len(run.numels)
    for step in range(3):
        run.set_grads(step)
        before = run.snapshot()
        got = run.step(grad_scale=scale)
        check_step(run, before, got, step, scale, f"{table} W={world} scale {scale} step {step}")
        assert got["skipped"] == 0 and float(got["coef"]) < 1.0


def test_fp32_parameters_are_their_own_masters_in_shards():
    run = Ranks("sizes", torch.float32, 3)
    for step in range(3):
        run.set_grads(step)
        before = run.snapshot()
        check_step(run, before, run.step(), step, 1.0, f"fp32 W=3 step {step}")


@pytest.mark.parametrize("table", ["sizes", "unaligned"])
def test_grad_scale_is_inv_scale(table):
    """grad_scale = 0.25 and inv_scale = 0.25 with grad_scale = 1 are the same product: the same bits — and so are 0.5 x 0.5."""
    runs = [Ranks(table, torch.bfloat16, 2) for _ in range(3)]
    quarter, half = (torch.tensor([v], dtype=torch.float32, device=DEV) for v in (0.25, 0.5))
    for step in range(3):
        for run in runs:
            run.set_grads(step)
        got = [runs[0].step(grad_scale=0.25), runs[1].step(inv_scale=quarter), runs[2].step(inv_scale=half, grad_scale=0.5)]
        assert got[0]["step"] == step + 1
        for other in runs[1:]:
            runs[0].same_bits(other, f"step {step}")


@pytest.mark.parametrize("table", ["sizes", "unaligned"])
def test_a_non_finite_gradient_in_one_shard_skips_every_shard(table):
    run = Ranks(table, torch.float16, 3)
    run.set_grads(0)
    assert run.step(grad_scale=0.5)["step"] == 1
    lay = run.layout
    victim = shard_slices(lay, 1)[0]                        # an element only rank 1 reads
    for k, bad in enumerate((float("nan"), float("inf"))):
        run.set_grads(1 + k)
        run.tensors[victim[0]]["g"][victim[1]] = bad
        before = run.snapshot()
        got = run.step(grad_scale=0.5)
        assert (got["found_inf"], got["step"], got["skipped"]) == (1, 1, 1 + k), got      # (read_state: in EVERY rank's block)
        assert not torch.isfinite(got["norm"])
        sums = run.sums.cpu()
        assert torch.isfinite(sums[0]) and torch.isfinite(sums[2]) and not torch.isfinite(sums[1])
        for t, b in zip(run.tensors, before):
            for key in ("p", "m", "v", "param", "g"):
                assert torch.equal(bits(t[key]), bits(b[key])), f"{key} of a skipped step changed"
    run.set_grads(3)
    before = run.snapshot()
    got = run.step(grad_scale=0.5)
    assert (got["found_inf"], got["step"], got["skipped"]) == (0, 2, 2), got
    check_step(run, before, got, 1, 0.5, "the step after the skipped ones")


def test_an_empty_shard_takes_part():
    run = Ranks(((1, 3, 63), 64), torch.bfloat16, 8)
    assert [n for _, n in run.tables] == [3, 0, 0, 0, 0, 0, 0, 0]
    for step in range(2):
        run.set_grads(step)
        before = run.snapshot()
        got = run.step()                                     # (read_state: the empty ranks' counters advanced with rank 0's)
        assert run.sums.cpu()[1:].tolist() == [0.0] * 7 and float(run.sums[0]) > 0
        check_step(run, before, got, step, 1.0, f"empty shards step {step}")


def test_two_runs_from_the_same_state_give_the_same_bits():
    a, b = Ranks("table_of_33", torch.bfloat16, 3), Ranks("table_of_33", torch.bfloat16, 3)
    for step in range(3):
        for r in (a, b):
            r.set_grads(step)
        a.step(grad_scale=0.5), b.step(grad_scale=0.5)
        a.same_bits(b, f"step {step}")
        assert torch.equal(bits(a.sums), bits(b.sums))


def test_bad_arguments_are_refused_before_any_launch():
    run = Ranks("sizes", torch.bfloat16, 2)
    run.set_grads(0)
    lib = _capi.load_library()
    tab, n = run.tables[0]
    ws, stream = run.workspaces[0], torch.cuda.current_stream().cuda_stream
    h = run.hyper()
    out, state = run.sums.data_ptr(), run.states[0].data_ptr()

    def sumsq(grad_scale=1.0, out=out, tab=tab):
        return lib.tp_optim_sumsq(tab, n, None, grad_scale, out, ws.data_ptr(), ws.numel(), stream)

    def apply(grad_scale=1.0, sums=out, nsums=2, tab=tab, h=h):
        return lib.tp_optim_apply(tab, n, ctypes.byref(h), None, grad_scale, sums, nsums, state, stream)

    def copy_of(tab, **fields):
        new = (_capi.tp_optim_tensor * n)()
        ctypes.memmove(new, tab, ctypes.sizeof(new))
        for k, v in fields.items():
            setattr(new[1], k, v)
        return new

    f32 = run.hyper()
    f32.dtype = _capi.TP_F32
    bad = {
        "sumsq: grad_scale 0": lambda: sumsq(0.0), "sumsq: grad_scale < 0": lambda: sumsq(-0.5),
        "sumsq: grad_scale NaN": lambda: sumsq(float("nan")), "sumsq: grad_scale inf": lambda: sumsq(float("inf")),
        "sumsq: NULL sumsq_out": lambda: sumsq(out=None), "sumsq: misaligned sumsq_out": lambda: sumsq(out=out + 4),
        "sumsq: NULL grad": lambda: sumsq(tab=copy_of(tab, grad=None)),
        "sumsq: duplicate grad": lambda: sumsq(tab=copy_of(tab, grad=tab[0].grad)),
        "apply: nsums 0": lambda: apply(nsums=0), "apply: NULL sums": lambda: apply(sums=None),
        "apply: misaligned sums": lambda: apply(sums=out + 4),
        "apply: grad_scale 0": lambda: apply(0.0), "apply: grad_scale < 0": lambda: apply(-1.0),
        "apply: grad_scale NaN": lambda: apply(float("nan")),
        "apply: NULL param": lambda: apply(tab=copy_of(tab, param=None)),
        "apply: misaligned master": lambda: apply(tab=copy_of(tab, master=tab[1].master + 2)),
        "apply: duplicate address": lambda: apply(tab=copy_of(tab, exp_avg=tab[0].exp_avg)),
        "apply: param with TP_F32": lambda: apply(h=f32),
    }
    for what, call in bad.items():
        assert call() == _capi.TP_ERR_INVALID_ARG, what
        msg = _capi.last_error()
        assert msg.startswith("tp_optim_sumsq:" if what.startswith("sumsq") else "tp_optim_apply:") and len(msg) > 20, (what, msg)
    torch.cuda.synchronize()
    assert run.sums.cpu().tolist() == [7.0, 7.0] and not bool(run.states.any()), "nothing was launched"
    assert not bool(run.flat["m"].any())
    assert sumsq() == _capi.TP_OK                            # ... and the same arguments, unbroken, are accepted
