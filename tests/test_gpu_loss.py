"""tokenpacker_amd.loss.shifted_cross_entropy on the GPU against the reference's op sequence in float64 (tests/loss_ref.py).

Inputs come from seeds: logits ~ N(0, 4^2) rounded to the dtype, a third of the targets -100.

Loss:      |loss - loss64| <= 2e-6 max(1, |loss64|)  (torch's own fp32 path: 1.5e-7 relative on the CPU at V = 32 000; the bound
           is that times about 13 for the device's fast exp / log), and for bf16 / fp16 never further from float64 than the
           reference's own-dtype loss is.
Gradient:  bf16 / fp16: every element within one unit in the last place of the float64 gradient rounded to the dtype;
           fp32: within 4e-7 max|g64|.  For an upstream gradient of 1, 2^-7 and 2^10.
The worst values seen are printed (pytest -s)."""
import math

import pytest
import torch

from tests import loss_ref
from tests.splice_ref import HD_GOLDEN, load_batch
from tokenpacker_amd import loss, splice

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
VOCABS = [1, 7, 64, 2049, 32000, 32003]
SHAPES = [(1, 2), (3, 5), (2, 9)]
UPSTREAM = [1.0, 2.0 ** -7, 2.0 ** 10]
LOSS_TOL = 2e-6
GRAD_TOL_F32 = 4e-7
INF = float("inf")
WORST = {"loss": 0.0, "grad_ulp": 0, "grad_f32": 0.0}


def make_case(V, B, L, dtype, seed=0):
    """(logits [B, L, V] in `dtype`, labels [B, L]) on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * V + 31 * B + L)
    x = (torch.randn(B, L, V, generator=g) * 4).to(dtype)
    y = torch.randint(0, V, (B, L), generator=g)
    y[torch.rand(B, L, generator=g) < 1 / 3] = -100
    return x, y


def on_gpu(x, layout="contiguous"):
    """`x` on the device in one of the layouts the kernels accept; the values of x and nothing else are addressed by the view."""
    B, L, V = x.shape
    if layout == "contiguous":
        return x.cuda()
    if layout == "padded":                            # a padded-vocabulary view: row stride V + 64
        buf = torch.full((B, L, V + 64), float("nan"), dtype=x.dtype, device="cuda")
        view = buf[..., :V]
    elif layout == "offset":                          # the base one element into an allocation
        buf = torch.full((B * L * V + 1,), float("nan"), dtype=x.dtype, device="cuda")
        view = buf[1:].view(B, L, V)
    elif layout == "batch_strided":                   # three spare rows behind every sample
        buf = torch.full((B, L + 3, V), float("nan"), dtype=x.dtype, device="cuda")
        view = buf[:, :L]
    elif layout == "all":                             # all of it at once
        buf = torch.full((1 + B * (L + 3) * (V + 64),), float("nan"), dtype=x.dtype, device="cuda")
        view = buf.as_strided((B, L, V), ((L + 3) * (V + 64), V + 64, 1), 1)
    view.copy_(x)
    return view


def run_ours(xg, y, upstream=(1.0,), **kw):
    """-> (loss on the CPU (fp32 0-dim), [gradient on the CPU for every upstream value], n_valid)."""
    xg = xg.detach().requires_grad_(True)
    out, n_valid = loss.shifted_cross_entropy(xg, y.cuda(), return_n_valid=True, **kw)
    assert out.dtype == torch.float32 and out.dim() == 0 and out.is_cuda and n_valid.dtype == torch.int64 and n_valid.dim() == 0
    grads = []
    for i, g in enumerate(upstream):
        grad, = torch.autograd.grad(out, xg, torch.tensor(g, device="cuda"), retain_graph=i + 1 < len(upstream))
        assert grad.dtype == xg.dtype and grad.shape == xg.shape
        grads.append(grad.cpu())
    torch.cuda.synchronize()
    return out.detach().cpu(), grads, int(n_valid)


def check_loss(got, ref64, own=None):
    want = float(ref64)
    if math.isnan(want) or math.isinf(want):
        assert (math.isnan(float(got)) and math.isnan(want)) or float(got) == want, (float(got), want)
        return
    err = abs(float(got) - want)
    WORST["loss"] = max(WORST["loss"], err / max(1.0, abs(want)))
    assert err <= LOSS_TOL * max(1.0, abs(want)), (float(got), want, err)
    if own is not None and math.isfinite(float(own)):
        assert err <= abs(float(own) - want), (float(got), float(own), want)


def check_grad(got, g64, dtype, scale=1.0):
    """`got` against the float64 gradient `g64 * scale` (scale a power of two: exact).  Non-finite entries must match in kind."""
    want = g64 * scale
    finite = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN pattern"
    assert torch.equal(got[~finite & ~torch.isnan(want)].double(), want[~finite & ~torch.isnan(want)]), "inf pattern"
    if dtype == torch.float32:
        bound = GRAD_TOL_F32 * float(want[finite].abs().max()) if finite.any() else 0.0
        err = float((got.double() - want)[finite].abs().max()) if finite.any() else 0.0
        if bound > 0:
            WORST["grad_f32"] = max(WORST["grad_f32"], err / bound * GRAD_TOL_F32)
        assert err <= bound, (err, bound)
    else:
        ulps = (loss_ref.ordered_bits(got) - loss_ref.ordered_bits(want.to(dtype)))[finite].abs()
        worst = int(ulps.max()) if ulps.numel() else 0
        WORST["grad_ulp"] = max(WORST["grad_ulp"], worst)
        assert worst <= 1, (worst, int((ulps > 1).sum()))


def check_zero_rows(grad, y, V, ignore_index=-100):
    """The row before an ignored (or out-of-range) target and the last row of every sample: exact zeros."""
    assert torch.equal(grad[:, -1], torch.zeros_like(grad[:, -1]))
    nxt = y[:, 1:]
    dead = (nxt == ignore_index) | (nxt < 0) | (nxt >= V)
    assert torch.equal(grad[:, :-1][dead], torch.zeros_like(grad[:, :-1][dead]))


def check_case(x, y, layout="contiguous", upstream=UPSTREAM, reduction="mean", xg=None):
    dtype, V = x.dtype, x.shape[-1]
    ref = loss_ref.shifted_cross_entropy(x, y, reduction=reduction)
    own = loss_ref.shifted_cross_entropy(x, y, None, reduction=reduction) if dtype != torch.float32 else None
    got, grads, n_valid = run_ours(on_gpu(x, layout) if xg is None else xg, y, upstream, reduction=reduction)
    assert n_valid == ref.n_valid
    check_loss(got, ref.loss, own.loss if own is not None else None)
    for g, grad in zip(upstream, grads):
        check_grad(grad, ref.grad, dtype, g)
        check_zero_rows(grad, y, V)
    return got, grads, ref


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    print(f"\nshifted_cross_entropy worst: loss {WORST['loss']:.3e} of max(1, |loss64|) (bound {LOSS_TOL:.0e}); gradient "
          f"{WORST['grad_ulp']} ulp (bf16 / fp16, bound 1), {WORST['grad_f32']:.3e} of max|g64| (fp32, bound {GRAD_TOL_F32:.0e})")


# ---- 1. the grid -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("B,L", SHAPES)
@pytest.mark.parametrize("V", VOCABS)
def test_grid_against_float64(V, B, L, dtype):
    x, y = make_case(V, B, L, dtype)
    y[0, 1] = (V - 1) if L % 2 else 0                    # at least one labelled row
    got, _, _ = check_case(x, y)
    if V == 1:
        assert float(got) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("layout", ["padded", "offset", "batch_strided", "all"])
@pytest.mark.parametrize("V", [7, 2049, 32003])
def test_layouts(V, layout, dtype):
    x, y = make_case(V, 3, 5, dtype, seed=1)
    y[1, 2] = 1
    xg = on_gpu(x, layout)
    assert not xg.is_contiguous() or layout == "offset"
    check_case(x, y, upstream=[1.0], xg=xg)
    # the forward wrote nothing, and the fresh gradient is a buffer of its own: everything outside the view is still NaN
    assert int(torch.isnan(xg._base).sum()) == xg._base.numel() - x.numel()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_targets_at_both_ends_of_the_vocabulary(dtype):
    for V in (7, 2049, 32003):
        x, y = make_case(V, 2, 9, dtype, seed=2)
        y[:, 1::2] = 0
        y[:, 2::2] = V - 1
        y[1, 5] = -100
        check_case(x, y, upstream=[1.0])


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_no_labelled_row(dtype):
    for V in (7, 32000):
        x, _ = make_case(V, 3, 5, dtype)
        y = torch.full((3, 5), -100)
        y[:, 0] = 3                                      # the first label is never a target
        for reduction in ("mean", "sum"):
            got, (grad,), n = run_ours(x.cuda(), y, reduction=reduction)
            assert n == 0 and (math.isnan(float(got)) if reduction == "mean" else float(got) == 0.0)
            assert torch.equal(grad, torch.zeros_like(grad))
    # L = 1: no row at all
    x, y = make_case(2049, 3, 1, dtype)
    got, (grad,), n = run_ours(x.cuda(), y.abs())
    assert n == 0 and math.isnan(float(got)) and torch.equal(grad, torch.zeros_like(grad))


# ---- 2. non-finite logits ------------------------------------------------------------------------------------------------------
def element_of_thread(ptr, V, es, thread):
    """The elements of a row at address `ptr` that thread `thread` of the 256 reads (the map documented in tp_loss.hip)."""
    per = 16 // es
    head = min(V, ((16 - ptr % 16) % 16) // es)
    nvec = (V - head) // per
    tail = V - head - nvec * per
    idx = [thread] if thread < head else []
    for v in range(thread, nvec, 256):
        idx += range(head + per * v, head + per * v + per)
    if thread < tail:
        idx.append(head + per * nvec + thread)
    return idx


def check_non_finite(x, y, reduction="mean"):
    """Pattern of finite / inf / NaN as the float32 reference, finite values to the float64 tolerances."""
    dtype = x.dtype
    r32 = loss_ref.shifted_cross_entropy(x, y, torch.float32, reduction=reduction)
    r64 = loss_ref.shifted_cross_entropy(x, y, reduction=reduction)
    got, (grad,), _ = run_ours(x.cuda(), y, reduction=reduction)
    lg, l32 = float(got), float(r32.loss)
    assert math.isnan(lg) == math.isnan(l32) and math.isinf(lg) == math.isinf(l32), (lg, l32)
    assert torch.equal(torch.isnan(grad), torch.isnan(r32.grad)) and torch.equal(torch.isinf(grad), torch.isinf(r32.grad))
    if math.isfinite(l32):
        check_loss(got, r64.loss)
    check_grad(grad, r64.grad, dtype)
    return got, grad


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("V", [7, 32000])
def test_non_finite_cases(V, dtype):
    x, y = make_case(V, 2, 5, dtype, seed=3)
    y[:, 1:] = torch.randint(0, V, (2, 4), generator=torch.Generator().manual_seed(V))
    # -inf logits in rows that keep finite ones (never at a target): finite loss, exact zeros there
    a = x.clone()
    holes = torch.rand(a.shape, generator=torch.Generator().manual_seed(1)) < 0.25
    for b in range(2):
        for t in range(4):
            holes[b, t, y[b, t + 1]] = False
    a[holes] = -INF
    got, grad = check_non_finite(a, y)
    assert math.isfinite(float(got)) and torch.equal(grad[holes], torch.zeros_like(grad[holes]))
    # -inf at a target: +inf, finite gradient
    a2 = a.clone()
    a2[0, 1, y[0, 2]] = -INF
    got, grad = check_non_finite(a2, y, reduction="sum")
    assert float(got) == INF and torch.isfinite(grad).all() and float(grad[0, 1, y[0, 2]]) == -1.0
    # a row of -inf only: NaN, NaN in that row and nowhere else
    a3 = a.clone()
    a3[1, 2] = -INF
    got, grad = check_non_finite(a3, y, reduction="sum")
    assert math.isnan(float(got)) and torch.isnan(grad[1, 2]).all() and int(torch.isnan(grad).sum()) == V
    # +-3e38 (one row: a second one would overflow the fp32 sum of the reference)
    if dtype != torch.float16:
        a4 = torch.full((1, 2, V), -3e38).to(dtype)
        a4[0, 0, 1], a4[0, 0, V // 2], a4[0, 0, V - 1] = 0.0, 3e38, 0.0
        y4 = torch.tensor([[0, V - 1]])
        got, grad = check_non_finite(a4, y4)
        big = float(torch.tensor(3e38).to(dtype))
        assert float(got) == float(torch.tensor(big, dtype=torch.float32))
        want = torch.zeros(V, dtype=dtype)
        want[V // 2], want[V - 1] = 1.0, -1.0
        assert torch.equal(grad[0, 0], want)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_minus_inf_in_front_of_a_row_and_in_all_of_one_threads_elements(dtype):
    """An online maximum that is still -inf after the first elements must not produce exp(-inf - (-inf))."""
    es = torch.finfo(dtype).bits // 8
    for V in (2049, 32000):
        for layout in ("contiguous", "offset"):
            x, y = make_case(V, 1, 4, dtype, seed=4)
            xg = on_gpu(x, layout)
            x[0, 0, :min(4096, V - 8)] = -INF           # the leading 4 096 logits: every thread starts on -inf, some see nothing else
            for thread in (0, 1, 255):                   # every logit one thread reads (rows 1 and 2)
                x[0, 1, element_of_thread(xg[0, 1].data_ptr(), V, es, thread)] = -INF
            x[0, 2, element_of_thread(xg[0, 2].data_ptr(), V, es, 64)] = -INF      # the first thread of the second wave
            for t in range(3):                           # every target at a logit that stayed finite
                y[0, t + 1] = int(torch.nonzero(torch.isfinite(x[0, t].float()))[-1 - t])
            xg.copy_(x)
            r64 = loss_ref.shifted_cross_entropy(x, y)
            got, (grad,), _ = run_ours(xg, y)
            assert math.isfinite(float(got))
            check_loss(got, r64.loss)
            check_grad(grad, r64.grad, dtype)
            assert torch.equal(grad[x == -INF], torch.zeros_like(grad[x == -INF]))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_out_of_range_targets_give_nan_and_a_zero_row(dtype):
    for V in (7, 32003):
        x, y = make_case(V, 2, 5, dtype, seed=5)
        y[:, 1:] = 2
        good = y.clone()
        for (b, t), bad in zip(((0, 1), (0, 3), (1, 4)), (V, -1, 2 ** 40)):
            y[b, t] = bad
            good[b, t] = -100
        for reduction in ("mean", "sum"):
            got, (grad,), n = run_ours(x.cuda(), y, reduction=reduction)
            torch.cuda.synchronize()                     # the run ends clean: no device assert, no fault
            assert math.isnan(float(got)) and n == 8
            check_zero_rows(grad, y, V)
        # under "sum" the other rows' gradients are those of the batch without the bad targets
        check_grad(grad, loss_ref.shifted_cross_entropy(x, good, reduction="sum").grad, dtype)
        # a wide ignore_index is a label like any other
        got, (grad,), n = run_ours(x.cuda(), y, ignore_index=2 ** 40)
        assert n == 7 and math.isnan(float(got))


# ---- 3. reductions, in place, determinism, memory ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_sum_and_mean_differ_by_n_valid(dtype):
    x, y = make_case(2049, 3, 5, dtype, seed=6)
    xg = x.cuda()
    mean, (gm,), n = run_ours(xg, y)
    total, (gs,), n2 = run_ours(xg, y, reduction="sum")
    assert n == n2 == int((y[:, 1:] != -100).sum()) and n > 1
    assert abs(float(total) - n * float(mean)) <= 2.0 ** -22 * abs(float(total))
    fi = torch.finfo(dtype)
    slack = 1.01 * fi.eps * gs.double().abs() + n * fi.smallest_normal * fi.eps
    assert bool(((gs.double() - n * gm.double()).abs() <= slack).all())
    check_case(x, y, reduction="sum")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("layout", ["contiguous", "all"])
def test_in_place_gradient(layout, dtype):
    x, y = make_case(32003, 2, 5, dtype, seed=7)
    _, (fresh,), _ = run_ours(on_gpu(x, layout), y, upstream=[0.5])
    xg = on_gpu(x, layout).requires_grad_(True)
    out = loss.shifted_cross_entropy(xg, y.cuda(), inplace_grad=True)
    grad, = torch.autograd.grad(out, xg, torch.tensor(0.5, device="cuda"), retain_graph=True)
    assert grad.data_ptr() == xg.data_ptr() and grad.stride() == xg.stride()
    assert torch.equal(grad.cpu().view(torch.int32 if dtype == torch.float32 else torch.int16),
                       fresh.view(torch.int32 if dtype == torch.float32 else torch.int16))
    assert torch.equal(xg.detach().cpu(), grad.cpu())           # the logits are gone
    with pytest.raises(RuntimeError, match="second backward"):
        torch.autograd.grad(out, xg, torch.tensor(0.5, device="cuda"))
    # without the option a second backward is an ordinary one
    xg = on_gpu(x, layout).requires_grad_(True)
    out = loss.shifted_cross_entropy(xg, y.cuda())
    g1, = torch.autograd.grad(out, xg, retain_graph=True)
    g2, = torch.autograd.grad(out, xg)
    assert g1.data_ptr() != xg.data_ptr() and torch.equal(g1, g2) and torch.equal(xg.detach().cpu(), x)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_two_runs_give_the_same_bits(dtype):
    x, y = make_case(32003, 2, 9, dtype, seed=8)
    runs = [run_ours(on_gpu(x, "offset"), y) for _ in range(2)]
    as_int = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1][0].view(as_int), runs[1][1][0].view(as_int))


def test_no_grad_and_backward_through_a_graph():
    x, y = make_case(2049, 2, 5, torch.bfloat16, seed=9)
    ref = loss_ref.shifted_cross_entropy(x, y, grad_out=3.0)
    with torch.no_grad():
        plain = loss.shifted_cross_entropy(x.cuda().requires_grad_(True), y.cuda())
    assert not plain.requires_grad
    leaf = x.cuda().requires_grad_(True)
    out = loss.shifted_cross_entropy(leaf * 1, y.cuda())
    assert out.requires_grad and torch.equal(out.detach(), plain)
    (out * 3).backward()
    check_loss(out.detach().cpu(), ref.loss)
    check_grad(leaf.grad.cpu(), ref.grad, torch.bfloat16)


def test_peak_memory_of_the_in_place_path():
    B, L, V = 2, 64, 32000
    x, y = make_case(V, B, L, torch.bfloat16, seed=10)
    xg = x.cuda().requires_grad_(True)
    yg = y.cuda()
    up = torch.ones((), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = loss.shifted_cross_entropy(xg, yg, inplace_grad=True)
    grad, = torch.autograd.grad(out, xg, up)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    logits_bytes = B * L * V * 2
    print(f"\npeak memory over forward + backward in place: +{rise} B, the logits are {logits_bytes} B")
    assert grad.data_ptr() == xg.data_ptr() and rise < logits_bytes / 4


# ---- 4. 64-bit addressing --------------------------------------------------------------------------------------------------------
def test_offsets_beyond_32_bits():
    """B = 2, L = 3, V = 2 049 in bf16, the view 2^31 elements into one uninitialised allocation with a batch stride of
    2^31 + 24: sample 1 lies 2^31 + 24 + t 2 049 elements (2^32 + 48 + ... bytes) behind the view's base.  An element offset cut
    to a signed 32 bits lands at element 24 + t 2 049 of the ALLOCATION, a byte offset cut to 32 bits (signed or unsigned) at
    element 24 + t 2 049 of the VIEW, inside sample 0's rows: both inside the allocation and both hold other values (decoys at the
    first site, sample 0 at the second), so a kernel that truncates fails on values and does not fault."""
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        print(f"\nSKIPPED: {free / 2 ** 30:.1f} GiB free, the 64-bit addressing test wants 16 GiB")
        pytest.skip("less than 16 GiB of device memory free")
    B, L, V = 2, 3, 2049
    start, bs = 2 ** 31, 2 ** 31 + 24
    x, y = make_case(V, B, L, torch.bfloat16, seed=11)
    y[:, 1:] = torch.tensor([[5, 2048], [0, 77]])
    buf = torch.empty(start + bs + L * V + 64, dtype=torch.bfloat16, device="cuda")          # about 8.6 GB, not initialised
    view = buf.as_strided((B, L, V), (bs, V, 1), start)
    view.copy_(x)
    decoy = (torch.randn(24 + L * V, generator=torch.Generator().manual_seed(12)) * 4).to(torch.bfloat16)
    buf[:24 + L * V].copy_(decoy)
    ref = loss_ref.shifted_cross_entropy(x, y)
    for inplace in (False, True):
        xg = view.detach().requires_grad_(True)
        out = loss.shifted_cross_entropy(xg, y.cuda(), inplace_grad=inplace)
        grad, = torch.autograd.grad(out, xg)
        torch.cuda.synchronize()
        check_loss(out.detach().cpu(), ref.loss)
        check_grad(grad.cpu(), ref.grad, torch.bfloat16)
        assert torch.equal(buf[:24 + L * V].cpu(), decoy)                                     # nothing was written at the decoys
    del buf, view, xg, grad
    torch.cuda.empty_cache()


# ---- 5. with the splice ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_labels_of_the_splice_go_straight_in(dtype):
    b = load_batch("ragged", HD_GOLDEN)
    emb = torch.nn.Embedding.from_pretrained(b["table"].to(dtype), padding_idx=b.get("padding_idx")).cuda()
    _, embeds, labels = splice.build_multimodal_inputs(
        b["ids"].cuda(), emb, b["feats"].to(dtype).cuda(), labels=b["labels"].cuda(), attention_mask=b["attention_mask"].cuda(),
        mode="slice", h_block=b["hb"], w_block=b["wb"], sep_id=b["sep_id"], ret_id=b["ret_id"])
    B, L = labels.shape
    V = b["table"].shape[0]
    assert embeds.shape[:2] == (B, L) and int((labels[:, 1:] != -100).sum()) > 0
    x = (torch.randn(B, L, V, generator=torch.Generator().manual_seed(13)) * 4).to(dtype)
    ref = loss_ref.shifted_cross_entropy(x, labels)
    xg = x.cuda().requires_grad_(True)
    out, n = loss.shifted_cross_entropy(xg, labels, return_n_valid=True)
    grad, = torch.autograd.grad(out, xg)
    assert int(n) == ref.n_valid
    check_loss(out.detach().cpu(), ref.loss, loss_ref.shifted_cross_entropy(x, labels, None).loss)
    check_grad(grad.cpu(), ref.grad, dtype)
    check_zero_rows(grad.cpu(), labels.cpu(), V)
