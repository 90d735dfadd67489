"""Every kernel of the BACKWARD on its own, on a real MI355X, through the test hooks of include/tokenpacker_test.h
(libtokenpacker_exp.so: pass-throughs to the launchers tp_backward calls), against fp64 math on the same rounded operands
(tests/bwd_ref.py) — ELEMENTWISE against the derived bound of each kernel, bit for bit where the kernel only moves or casts, and
exactly on integer-valued data where it sums.  tests/test_bwd_ref_cpu.py proves the references and their bounds without a GPU.

Every test prints the worst error / bound it reached (`[bwd-ratio] kernel family ratio`, pytest -s); > 1 fails."""
import ctypes
import math

import pytest
import torch

from tokenpacker_amd import _capi
from tests import bwd_ref as br
from tests import gpu_util as gu

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
RATIOS = {}


def _tl():
    return _capi.load_test_library()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ok(rc, what):
    assert rc == _capi.TP_OK, f"{what}: status {rc}: {_tl().tp_last_error().decode()}"


def _sync():
    torch.cuda.synchronize()


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _scalar(v):
    return torch.tensor([v], dtype=F32, device="cuda")


def _record(kernel, family, ratio):
    key = (kernel, family)
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    print(f"[bwd-ratio] {kernel} {family} {ratio:.4f}")


def _within(got, ref, bound, name, kernel, family):
    """Elementwise |got - ref| <= bound; ref / bound may live on the CPU or on the GPU.  For a 16-bit result the bound's rounding
    term alone is reached by construction (half an ulp at the bottom of a binade IS u_T |ref|), so the share of the bound's
    fp32-class part that the error beyond one rounding takes is recorded as well (`<kernel> beyond rounding`)."""
    g = got.detach().to(ref.device)
    assert not bool(torch.isnan(g.float()).any()), f"{name}: NaN in the result"
    ratio = br.worst_ratio(g.to(F64), ref.to(F64), bound)
    _record(kernel, family, ratio)
    if got.dtype in (F16, BF16):
        rb = br.round_bound(ref.to(F64), got.dtype)
        over = ((g.to(F64) - ref.to(F64)).abs() - rb).clamp(min=0.0)
        _record(kernel + " beyond rounding", family, br.worst_ratio(over, torch.zeros_like(over), (bound - rb).clamp(min=1e-300)))
    assert ratio <= 1.0, f"{name}: worst error / bound = {ratio:.3f}\n" + gu.describe_mismatch(
        g.reshape(-1, g.shape[-1]), ref.reshape(-1, ref.shape[-1]), name, 0.0)


def _same_bits(got, want, name):
    g, w = got.detach().cpu(), want.detach().cpu()
    assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
    assert torch.equal(g, w), gu.describe_mismatch(g.reshape(-1, g.shape[-1]), w.reshape(-1, w.shape[-1]), name, 0.0)


@pytest.fixture(scope="module", autouse=True)
def _ratio_table():
    yield
    print("\n[bwd-ratio] ---- worst error / bound per kernel and case family ----")
    for (kernel, family), r in sorted(RATIOS.items()):
        print(f"[bwd-ratio-summary] {kernel:28s} {family:24s} {r:.4f}")


# ================================================================================================================================
# transposes
# ================================================================================================================================
def _transpose(src_view, R, C, ld, rpb, bstride, dst_dtype, Rpad, mr=None, gamma=None, beta=None, want_colsum=False):
    ldd = Rpad + 8
    dst = _nan((C, ldd), dst_dtype)
    slabs = (Rpad + 63) // 64
    cs = _nan((slabs, C), F32) if want_colsum else None
    _ok(_tl().tp_test_bw_transpose(gu.DT[src_view.dtype], gu.DT[dst_dtype], src_view.data_ptr(), ld, rpb, bstride, R, C, dst.data_ptr(),
                                   ldd, Rpad, _ptr(mr), _ptr(gamma), _ptr(beta), _ptr(cs), slabs * C if want_colsum else 0,
                                   gu.stream_ptr()), "tp_test_bw_transpose")
    _sync()
    assert bool(torch.isnan(dst[:, Rpad:].float()).all()), "columns beyond Rpad were written"
    return dst[:, :Rpad], cs


def _pads(R):
    return sorted({-(-R // m) * m for m in (8, 64, 1024)})


@pytest.mark.parametrize("C", [8, 72, 1024])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 1000])
def test_transpose_moves_casts_pads_and_sums(R, C):
    g = torch.Generator().manual_seed(R * 7 + C)
    ld = C + 8                                                        # ld > C
    for sdt in br.GDTYPES:
        buf = (3.0 * torch.randn(R, ld, generator=g)).to(sdt)
        buf[0, 0] = 70000.0 if sdt == BF16 else 65504.0               # (bf16 -> fp16 saturates at +-65504)
        ints = torch.randint(-8, 9, (R, ld), generator=g).to(sdt)
        for ddt in br.GDTYPES:
            for Rpad in _pads(R):
                got, cs = _transpose(buf.cuda(), R, C, ld, 0, 0, ddt, Rpad, want_colsum=True)
                ref, bound = br.transpose_ref(buf[:, :C], Rpad, ddt)
                assert bound is None
                _same_bits(got, br.cast_exact(ref, ddt), f"transpose {sdt}->{ddt} R={R} C={C} Rpad={Rpad}")
                assert float(got[:, R:].float().abs().max() if Rpad > R else 0.0) == 0.0          # padding: exact zeros over the NaN
                # one slab of column sums per 64-row block, the last partial block included; blocks past R are zeros
                slabs = (Rpad + 63) // 64
                rows = torch.zeros(slabs * 64, C, dtype=F64)
                rows[:R] = buf[:, :C].double()
                blocks = rows.reshape(slabs, 64, C)
                _within(cs, blocks.sum(1), 64 * br.EPS32 * blocks.abs().sum(1) + br.EPS32 * blocks.sum(1).abs(),
                        f"transpose colsum_part R={R} C={C}", "transpose", "colsum_part")
            # integer-valued rows: every partial sum is exact
            got, cs = _transpose(ints.cuda(), R, C, ld, 0, 0, ddt, _pads(R)[1 if len(_pads(R)) > 1 else 0], want_colsum=True)
            rows = torch.zeros(cs.shape[0] * 64, C, dtype=F64)
            rows[:R] = ints[:, :C].double()
            assert torch.equal(cs.double().cpu(), rows.reshape(-1, 64, C).sum(1)), "integer column sums must be exact"


@pytest.mark.parametrize("C", [72, 1024])
def test_transpose_batch_strided_source(C):
    """rows_per_batch 576 inside a CLS-prefixed [B, 577, C] buffer (the tower's [:, 1:] slices)."""
    B, T = 3, 576
    for sdt, ddt in ((BF16, F16), (F16, F16), (BF16, BF16), (F16, BF16)):
        buf = (2.0 * torch.randn(B, T + 1, C, generator=torch.Generator().manual_seed(C))).to(sdt).cuda()
        view = buf[:, 1:]
        R = B * T
        for Rpad in (R, R + 64 - R % 64 if R % 64 else R + 64):
            got, cs = _transpose(view, R, C, view.stride(1), T, view.stride(0), ddt, Rpad, want_colsum=True)
            a = view.reshape(R, C).cpu()
            ref, _ = br.transpose_ref(a, Rpad, ddt)
            _same_bits(got, br.cast_exact(ref, ddt), f"strided transpose {sdt}->{ddt} C={C} Rpad={Rpad}")
            ref_cs, bound = br.colsum_ref(a, 64 * 2)
            _within(cs.double().sum(0), ref_cs, bound, "strided transpose colsum", "transpose", "colsum_part strided")


@pytest.mark.parametrize("R,C", [(1, 1024), (65, 1024), (1000, 1024), (63, 72), (1000, 8)])
def test_transpose_applies_the_layernorm(R, C):
    g = torch.Generator().manual_seed(R + C)
    x = (1.5 * torch.randn(R, C, generator=g) + 2.0 * torch.randn(R, 1, generator=g)).half()
    xd = x.double()
    mu = xd.mean(1)
    mr = torch.stack([mu, 1.0 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(1) + 1e-6)], 1).float()
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    gamma[::5] = 0.0
    gamma[1::7] = -gamma[1::7].abs() - 0.1                           # zeros and negatives
    beta = 0.2 * torch.randn(C, generator=g)
    for ddt in br.GDTYPES:
        for Rpad in _pads(R)[:2]:
            got, _ = _transpose(x.cuda(), R, C, C, 0, 0, ddt, Rpad, mr.cuda(), gamma.cuda(), beta.cuda())
            ref, bound = br.transpose_ref(x, Rpad, ddt, mr, gamma, beta)
            _within(got, ref, bound, f"transpose + LayerNorm -> {ddt} R={R} C={C} Rpad={Rpad}", "transpose", "LayerNorm applied")
            if Rpad > R:
                assert float(got[:, R:].float().abs().max()) == 0.0   # (not beta: the padding is zero)


def test_transpose_batch_of_eight_matrices():
    shapes = [(1, 8), (63, 72), (64, 1024), (65, 8), (1000, 72), (256, 256), (7, 1024), (129, 136)]
    g = torch.Generator().manual_seed(8)
    for sdt in br.GDTYPES:
        for ddt in br.GDTYPES:
            srcs, dsts, lds, Rs, Cs, Rpads = [], [], [], [], [], []
            for i, (R, C) in enumerate(shapes):
                ld = C + 8 * (i % 3)
                srcs.append((2.0 * torch.randn(R, ld, generator=g)).to(sdt).cuda())
                Rpad = -(-R // 8) * 8 + 8 * (i % 2)
                dsts.append(_nan((C, Rpad), ddt))
                lds.append(ld); Rs.append(R); Cs.append(C); Rpads.append(Rpad)
            n = len(shapes)
            _ok(_tl().tp_test_bw_transpose_batch(
                gu.DT[sdt], gu.DT[ddt], n, (ctypes.c_void_p * n)(*[t.data_ptr() for t in srcs]), (ctypes.c_int64 * n)(*lds),
                (ctypes.c_int * n)(*Rs), (ctypes.c_int * n)(*Cs), (ctypes.c_void_p * n)(*[t.data_ptr() for t in dsts]),
                (ctypes.c_int * n)(*Rpads), gu.stream_ptr()), "tp_test_bw_transpose_batch")
            _sync()
            for i, (R, C) in enumerate(shapes):
                ref, _ = br.transpose_ref(srcs[i].cpu()[:, :C], Rpads[i], ddt)
                _same_bits(dsts[i], br.cast_exact(ref, ddt), f"transpose batch {sdt}->{ddt} matrix {i}")


# ================================================================================================================================
# column sums and the reductions
# ================================================================================================================================
def _colsum_rows(v, R, C, ld, want_amax=False, finite=True):
    part = _nan((512, C), F32)
    amax = _nan((4096,), F32) if want_amax else None
    cnt = ctypes.c_int(-1)
    S = _tl().tp_test_bw_colsum_rows(gu.DT[v.dtype], v.data_ptr(), ld, R, C, part.data_ptr(), part.numel(), _ptr(amax), 4096 if want_amax else 0,
                                     ctypes.byref(cnt), gu.stream_ptr())
    assert S >= 1, f"tp_test_bw_colsum_rows: {S}: {_tl().tp_last_error().decode()}"
    _sync()
    assert S <= max(1, min(512, R // 64))
    assert bool(torch.isnan(part[S:]).all()) and not (finite and bool(torch.isnan(part[:S]).any())), "slices written != the returned count"
    return part[:S], S, (amax, cnt.value)


def _reduce_many(part, nparts, n, stride, out_dtype, out_scale=None, n_out=-1):
    out = _nan((n,), out_dtype)
    scratch = _nan((32 * n,), F32)
    _ok(_tl().tp_test_bw_reduce_many_parts(gu.DT[out_dtype], part.data_ptr(), stride, nparts, n, out.data_ptr(), scratch.data_ptr(),
                                           scratch.numel(), _ptr(out_scale), n_out, gu.stream_ptr()), "tp_test_bw_reduce_many_parts")
    _sync()
    return out


@pytest.mark.parametrize("R,C,ld", br.COLSUM_CASES)
def test_colsum_rows_and_its_reduction(R, C, ld):
    full = R in br.FULL_ROWS
    dev = "cuda" if full else "cpu"                                   # (full size: the fp64 reference is torch on the GPU)
    g = torch.Generator(device=dev).manual_seed(R + C)
    for dtype in ((BF16,) if full else br.GDTYPES):
        buf = torch.randn(R, ld, generator=g, device=dev).to(dtype)
        ints = torch.randint(-8, 9, (R, ld), generator=g, device=dev).to(dtype)
        for data, exact in ((buf, False), (ints, True)):
            dg = data.cuda()
            part, S, (amax, cnt) = _colsum_rows(dg, R, C, ld, want_amax=True)
            v = data[:, :C]
            depth = br.sum_depth(R, S)                                # from the geometry passed and the slice count returned
            ref, bound = br.colsum_ref(v, depth)
            fam = "full size" if full else ("ld = 2C" if ld != C else "plain")
            if exact:
                assert torch.equal(part.double().sum(0).to(ref.device), ref), f"integer column sums R={R} C={C}: not exact"
            else:
                _within(part.double().sum(0), ref, bound, f"colsum_rows {dtype} R={R} C={C} ld={ld}", "colsum_rows", fam)
            # max |v| per workgroup: the maximum is exact
            assert cnt >= 1 and not bool(torch.isnan(amax[:cnt]).any()) and bool(torch.isnan(amax[cnt:]).all())
            assert float(amax[:cnt].max()) == float(v.float().abs().max())
            # ... and the second stage: bias-gradient form, every output dtype, with and without the 1 / S of a scaled chain
            for odt in (BF16, F16, F32):
                for sc in (None, 2.0 ** -5):
                    out = _reduce_many(part, S, C, C, odt, None if sc is None else _scalar(sc))
                    d2 = depth + br.sum_depth(S, 1)
                    ref2, bound2 = br.colsum_ref(v, d2, odt, 1.0 if sc is None else sc)
                    if exact:
                        _same_bits(out.reshape(1, -1), br.cast_exact(ref2, odt).reshape(1, -1), f"integer bias gradient {odt} R={R} C={C}")
                    else:
                        _within(out.reshape(1, -1), ref2.reshape(1, -1), bound2.reshape(1, -1), f"colsum + reduce {odt} R={R} C={C}",
                                "colsum_rows + reduce_many", fam)
        del buf, ints


def test_colsum_amax_keeps_inf_and_nan():
    R, C = 4097, 520
    v = torch.randn(R, C, generator=torch.Generator().manual_seed(1)).to(BF16)
    v[4000, 519] = float("inf")
    _, _, (amax, cnt) = _colsum_rows(v.cuda(), R, C, C, want_amax=True)
    assert float(amax[:cnt].max()) == math.inf                        # inf is kept
    v[4096, 0] = NAN
    _, _, (amax, cnt) = _colsum_rows(v.cuda(), R, C, C, want_amax=True, finite=False)
    assert bool(torch.isnan(amax[:cnt]).any())                        # a NaN sticks ...
    scale = _nan((2,), F32)
    _ok(_tl().tp_test_bw_dynamic_scale(amax.data_ptr(), cnt, scale.data_ptr(), gu.stream_ptr()), "tp_test_bw_dynamic_scale")
    _sync()
    assert scale.tolist() == [1.0, 1.0]                               # ... through to S = 1


@pytest.mark.parametrize("n,nparts", br.REDUCE_CASES)
def test_reduce_parts_and_reduce_many_parts(n, nparts):
    g = torch.Generator().manual_seed(n * 31 + nparts)
    stride = n + 4 * (nparts % 3)
    n_out = n - 3 if n > 4 else n - 1                                  # n_out < n
    sc = 2.0 ** -5
    for exact in (False, True):
        part = (torch.randint(-8, 9, (nparts, stride), generator=g).float() if exact else torch.randn(nparts, stride, generator=g))
        pg = part.cuda()
        for odt in (BF16, F16, F32):
            for scale in (None, sc):
                s = 1.0 if scale is None else scale
                out = _reduce_many(pg, nparts, n, stride, odt, None if scale is None else _scalar(scale), n_out)
                assert bool(torch.isnan(out[n_out:].float()).all()), "columns beyond n_out were written"
                ref, bound = br.colsum_ref(part[:, :n_out], br.sum_depth(nparts, 1), odt, s)
                out1, sct = _nan((n,), odt), (None if scale is None else _scalar(scale))
                _ok(_tl().tp_test_bw_reduce_parts(gu.DT[odt], pg.data_ptr(), stride, nparts, n_out, out1.data_ptr(), _ptr(sct),
                                                  gu.stream_ptr()), "tp_test_bw_reduce_parts")
                _sync()
                assert bool(torch.isnan(out1[n_out:].float()).all())
                ref1, bound1 = br.colsum_ref(part[:, :n_out], nparts, odt, s)           # (one sequential chain of nparts additions)
                if exact:
                    _same_bits(out[:n_out].reshape(1, -1), br.cast_exact(ref, odt).reshape(1, -1), f"integer reduce_many n={n} nparts={nparts}")
                    _same_bits(out1[:n_out].reshape(1, -1), br.cast_exact(ref1, odt).reshape(1, -1), f"integer reduce n={n} nparts={nparts}")
                else:
                    _within(out[:n_out].reshape(1, -1), ref.reshape(1, -1), bound.reshape(1, -1), f"reduce_many {odt} n={n} nparts={nparts}",
                            "reduce_many_parts", str(odt).split(".")[-1])
                    _within(out1[:n_out].reshape(1, -1), ref1.reshape(1, -1), bound1.reshape(1, -1), f"reduce {odt} n={n} nparts={nparts}",
                            "reduce_parts", str(odt).split(".")[-1])


# ================================================================================================================================
# dynamic scale, scale + cast
# ================================================================================================================================
def test_dynamic_scale_is_the_exact_power_of_two():
    amaxes = [2.0 ** e for e in range(-70, 71)] + [1.5 * 2.0 ** e for e in range(-70, 71, 3)] + \
        [16.0, math.nextafter(32.0, 0.0), 32.0, math.nextafter(16.0, 0.0), 2.0 ** -133, 2.0 ** -126 * 0.75, 65504.0, 3.3895e38,
         0.0, math.inf, NAN]
    amaxes = [float(torch.tensor(a, dtype=F32)) for a in amaxes]      # (what the kernel is given is the fp32 value)
    g = torch.Generator().manual_seed(2)
    for i, a in enumerate(amaxes):
        nparts = (1, 7, 300, 4096)[i % 4]
        part = torch.rand(nparts, generator=g) * (a if (a == a and a < math.inf) else 1.0) * 0.99
        part[int(torch.randint(0, nparts, (1,), generator=g))] = a
        scale, pg = _nan((2,), F32), part.cuda()
        _ok(_tl().tp_test_bw_dynamic_scale(pg.data_ptr(), nparts, scale.data_ptr(), gu.stream_ptr()), "tp_test_bw_dynamic_scale")
        _sync()
        S, inv = br.dynamic_scale_ref(a)
        assert scale.tolist() == [S, inv], (a, scale.tolist(), (S, inv))
        if a == a and 0 < a < math.inf and abs(math.log2(S)) < 60:
            assert 16.0 <= a * S < 32.0


@pytest.mark.parametrize("sdt", br.GDTYPES)
def test_scale_cast_is_bit_exact_and_reports_saturation(sdt):
    g = torch.Generator().manual_seed(4)
    for n in (8, 8 * 12345, 8 * 2048 * 256 + 8):
        for k in (0, 3, 7, 12):
            src = (torch.randn(n, generator=g) * 2.0 ** -k).to(sdt)
            src[::1001] = 2.0 ** -20 * 2.0 ** -k                       # (lands on the fp16 subnormal grid)
            S = 2.0 ** k
            for case in ("plain", "edge", "over", "nan"):
                s = src.clone()
                if case == "edge":
                    s[n // 2] = 65504.0 / S if sdt == F16 else 65280.0 / S   # just under 65520: no report
                if case == "over":
                    s[n - 1] = -65536.0 / S                             # >= 65520: reported, clamped
                if case == "nan":
                    s[3] = NAN
                dst, flag = _nan((n,), F16), torch.zeros(1, dtype=torch.int32, device="cuda")
                sg, scl = s.cuda(), torch.tensor([S, 1.0 / S], dtype=F32, device="cuda")
                _ok(_tl().tp_test_bw_scale_cast(gu.DT[sdt], sg.data_ptr(), n, scl.data_ptr(), dst.data_ptr(), flag.data_ptr(), gu.stream_ptr()),
                    "tp_test_bw_scale_cast")
                _sync()
                prod = s.double() * S
                keep = ~torch.isnan(prod)
                want = br.cast_exact(torch.where(keep, prod, torch.zeros_like(prod)), F16)
                assert torch.equal(dst.cpu()[keep], want[keep]), f"scale_cast {sdt} n={n} k={k} {case}"
                want_flag = bool((~(prod.abs() < br.SAT_THRESHOLD)).any())
                assert want_flag == (case in ("over", "nan"))
                assert int(flag.item()) == (1 if want_flag else 0), f"saturation bit {sdt} n={n} k={k} {case}: {int(flag.item())}"


# ================================================================================================================================
# LayerNorm backward
# ================================================================================================================================
def _ln_backward(dy, x, mr, gamma, beta, nblocks, with_xn, want_flag=False):
    rows = dy.shape[0]
    dx, xn = _nan(tuple(dy.shape), dy.dtype), (_nan(tuple(dy.shape), dy.dtype) if with_xn else None)
    part = _nan((nblocks, 3, br.E), F32)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ok(_tl().tp_test_bw_ln_backward(gu.DT[dy.dtype], dy.data_ptr(), x.data_ptr(), mr.data_ptr(), gamma.data_ptr(), dx.data_ptr(),
                                     part.data_ptr(), part.numel(), nblocks, rows, _ptr(beta if with_xn else None), _ptr(xn),
                                     flag.data_ptr(), gu.stream_ptr()), "tp_test_bw_ln_backward")
    _sync()
    assert not bool(torch.isnan(part).any()), "a workgroup did not write its slab of partial sums"
    return dx, xn, part, int(flag.item())


def _check_ln(dy, x, mr, gamma, beta, nblocks, with_xn, family, name):
    """dy .. beta on the device the reference is to be computed on; launches on copies on the GPU."""
    rows, gdtype = dy.shape[0], dy.dtype
    dx, xn, part, flag = _ln_backward(dy.cuda(), x.cuda(), mr.cuda(), gamma.cuda(), beta.cuda(), nblocks, with_xn)
    ref = br.ln_backward_ref(dy, x, mr, gamma, beta if with_xn else None, gdtype=gdtype)
    _within(dx, ref["dx"], ref["dx_bound"], f"{name} dx", "ln_backward dx", family)
    if with_xn:
        _within(xn, ref["xn"], ref["xn_bound"], f"{name} xn", "ln_backward xn", family)
    d = br.sum_depth(rows, nblocks)
    sums = part.double().sum(0).to(dy.device)                          # [3][E]: exact sum of the workgroups' fp32 partials
    for i, key in ((0, "dgamma"), (1, "dbeta")):
        t = ref[key + "_terms"]
        _within(sums[i].reshape(1, -1), t.sum(0).reshape(1, -1), (d * br.EPS32 * t.abs().sum(0)).reshape(1, -1), f"{name} {key}",
                "ln_backward " + key, family)
    dxd = dx.to(dy.device).double()                                    # the column sums of the ROUNDED dx the kernel wrote
    _within(sums[2].reshape(1, -1), dxd.sum(0).reshape(1, -1), (d * br.EPS32 * dxd.abs().sum(0)).reshape(1, -1), f"{name} colsum(dx)",
            "ln_backward colsum(dx)", family)
    assert flag == 0 or gdtype == F16
    return dx


def _ln_integer_cases(rows, nblocks, gdtype, dev):
    """Integer-valued data with (mean, rstd) = (0, 1), gamma = 1: every product and partial sum is exact in fp32."""
    g = torch.Generator(device=dev).manual_seed(rows + nblocks)
    ri = lambda *shape: torch.randint(-8, 9, shape, generator=g, device=dev).float()     # noqa: E731
    mr = torch.tensor([0.0, 1.0], device=dev).repeat(rows, 1).contiguous()
    one, zero = torch.ones(br.E, device=dev), torch.zeros(br.E, device=dev)
    # (A) dgamma = sum dy x and dbeta = sum dy, exactly
    dy, x = ri(rows, br.E).to(gdtype), ri(rows, br.E).half()
    _, _, part, _ = _ln_backward(dy.cuda(), x.cuda(), mr.cuda(), one.cuda(), zero.cuda(), nblocks, False)
    sums = part.double().sum(0).to(dev)
    assert torch.equal(sums[0], (dy.double() * x.double()).sum(0)), f"integer dgamma rows={rows} nblocks={nblocks}"
    assert torch.equal(sums[1], dy.double().sum(0)), f"integer dbeta rows={rows} nblocks={nblocks}"
    # (B) rows with mean(g) = mean(g xhat) = 0 (x constant along the row, dy = [u, -u]): dx = dy exactly, and so its column sums
    u = ri(rows, br.E // 2)
    dy = torch.cat([u, -u], 1).to(gdtype)
    x = ri(rows, 1).expand(rows, br.E).contiguous().half()
    dx, _, part, _ = _ln_backward(dy.cuda(), x.cuda(), mr.cuda(), one.cuda(), zero.cuda(), nblocks, False)
    assert torch.equal(dx.to(dev).float(), dy.float()), f"integer dx rows={rows} nblocks={nblocks}"
    assert torch.equal(part.double().sum(0).to(dev)[2], dy.double().sum(0)), f"integer colsum(dx) rows={rows} nblocks={nblocks}"


@pytest.mark.parametrize("family", br.LN_FAMILIES)
@pytest.mark.parametrize("nblocks", br.LN_NBLOCKS)
@pytest.mark.parametrize("rows", [r for r in br.LN_ROWS if r not in br.FULL_ROWS])
def test_ln_backward(rows, nblocks, family):
    for gdtype in br.GDTYPES:
        dy, x, mr, gamma, beta = br.ln_inputs(family, rows, gdtype, 100 + rows)
        if rows >= 3:
            dy[1] = 0.0                                               # a zero dy row ...
        with_xn = nblocks != 7                                        # (with and without the normalised output)
        dx = _check_ln(dy, x, mr, gamma, beta, nblocks, with_xn, family, f"ln_backward {family} {gdtype} rows={rows} nblocks={nblocks}")
        if rows >= 3:
            assert float(dx[1].float().abs().max()) == 0.0            # ... gives a dx row of exact zeros
    if family == "plain":
        for gdtype in br.GDTYPES:
            _ln_integer_cases(rows, nblocks, gdtype, "cpu")


@pytest.mark.parametrize("nblocks", br.LN_NBLOCKS)
@pytest.mark.parametrize("rows,family", br.LN_FULL_CASES)
def test_ln_backward_full_size(rows, family, nblocks):
    """The B = 32 / B = 256 row counts (ln_backward_kernel grid-strides 144 rows per wave at 147 456 rows over 256 workgroups);
    the fp64 reference is plain torch on the GPU; one gradient dtype."""
    dy, x, mr, gamma, beta = br.ln_inputs(family, rows, BF16, 100 + rows, device="cuda")
    _check_ln(dy, x, mr, gamma, beta, nblocks, True, family + " full size", f"ln_backward {family} rows={rows} nblocks={nblocks}")
    del dy, x, mr
    _ln_integer_cases(rows, nblocks, BF16, "cuda")


def test_ln_backward_fp16_saturation_bit():
    """The LayerNorm backward's bit of tp_backward's status word (bit 1, value 2: include/tokenpacker.h) is set exactly when a dx
    value reaches 65520 (what fp16 would round to inf); the value is clamped."""
    rows = 36
    dy, x, mr, gamma, beta = br.ln_inputs("tinyvar", rows, F16, 9)
    base = float(br.ln_backward_ref(dy, x, mr, gamma)["dx"].abs().max())
    for target, want in ((0.5, False), (0.97, False), (1.03, True), (4.0, True)):
        dys = (dy.float() * (target * br.SAT_THRESHOLD / base)).half()
        ref = br.ln_backward_ref(dys, x, mr, gamma, gdtype=F16)
        top = float(ref["dx"].abs().max())
        assert abs(top / br.SAT_THRESHOLD - 1.0) > 0.01 and (top >= br.SAT_THRESHOLD) == want      # (the case is not marginal)
        for nblocks in (1, 7):
            dx, _, _, flag = _ln_backward(dys.cuda(), x.cuda(), mr.cuda(), gamma.cuda(), beta.cuda(), nblocks, False)
            assert flag == (2 if want else 0), (target, nblocks, flag)
            clamped = ref["dx"].clamp(-br.F16_MAX, br.F16_MAX)
            _within(dx, clamped, ref["dx_bound"], f"ln_backward saturating x{target}", "ln_backward dx", "fp16 saturation")
        dxb, _, _, flag = _ln_backward(dys.bfloat16().cuda(), x.cuda(), mr.cuda(), gamma.cuda(), beta.cuda(), 7, False)
        assert flag == 0                                               # bf16 has the range: nothing to report


# ================================================================================================================================
# region attention backward
# ================================================================================================================================
def _attention(q, k, v, dout, B, grid, s, mask=None, mode=0, want_dmask=False, inv_scale=None):
    gdtype = dout.dtype
    M, N, S2 = (grid // s) ** 2, grid * grid, s * s
    S2p = (S2 + 3) & ~3
    dq, dk, dv = _nan((B, M, br.E), gdtype), _nan((B, N, br.E), gdtype), _nan((B, N, br.E), gdtype)
    dmask = part = red = None
    if want_dmask:
        dmask = _nan((S2p,) if mode == 1 else (M * B * br.HEADS, S2), F32)
        if mode == 1:
            part, red = _nan((B * M, S2p), F32), _nan((32 * S2p,), F32)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ok(_tl().tp_test_bw_region_attention(
        gu.DT[gdtype], q.data_ptr(), k.data_ptr(), v.data_ptr(), dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), B, grid, s,
        _ptr(mask), mode, _ptr(dmask), _ptr(inv_scale), _ptr(part), 0 if part is None else part.numel() * 4, _ptr(red),
        0 if red is None else red.numel(), flag.data_ptr(), gu.stream_ptr()), "tp_test_bw_region_attention")
    _sync()
    assert int(flag.item()) == 0
    if part is not None:
        assert float(part[:, S2:].abs().max() if S2p > S2 else 0.0) == 0.0, "mode-1 padding columns must be zero"
        assert not bool(torch.isnan(part).any())
        assert bool(torch.isnan(dmask[S2:]).all())
        dmask = dmask[:S2]
    return dq, dk, dv, dmask


@pytest.mark.parametrize("variant", br.ATTN_VARIANTS)
@pytest.mark.parametrize("grid,s,B", br.ATTN_CASES)
def test_region_attention_backward(grid, s, B, variant):
    for gdtype in br.GDTYPES:
        q, k, v, dout, mask, mode = br.attn_inputs(grid, s, B, gdtype, variant, 11 + s)
        ref = br.attention_bwd_ref(q, k, v, dout, grid, s, mask, mode, gdtype=gdtype)
        if variant == "peaked" and s > 1:
            assert float(ref["p"].max()) > 0.99                       # the case really is peaked
        dev = [t.cuda() for t in (q, k, v, dout)]
        mg = None if mask is None else mask.cuda()
        dq, dk, dv, dmask = _attention(*dev, B, grid, s, mg, mode, want_dmask=bool(mode))
        name = f"attention bwd {variant} {gdtype} grid={grid} s={s} B={B}"
        fam = variant if s > 1 else "s = 1"
        if s == 1:                                                     # dQ = dK = 0 and dV = cast(dO), exactly
            assert float(dq.float().abs().max()) == 0.0 and float(dk.float().abs().max()) == 0.0
            _same_bits(dv, dout.reshape(B, grid * grid, br.E), name + " dv")
        for n, got in (("dq", dq), ("dk", dk), ("dv", dv)):
            _within(got, ref[n], ref[n + "_bound"], f"{name} {n}", "attention " + n, fam)
        if mode:
            bound = ref["dmask_bound"]
            if mode == 1:
                nq = B * (grid // s) ** 2
                bound = bound + (br.sum_depth(nq, 1) + 8) * br.EPS32 * ref["dmask_abs"]
            _within(dmask.reshape(1, -1), ref["dmask"].reshape(1, -1), bound.reshape(1, -1), f"{name} dmask", f"attention dmask mode {mode}", fam)
            # without dmask the other three keep their bits; inv_scale = 2^-7 is exactly 2^-7 times the unscaled result
            dq2, dk2, dv2, _ = _attention(*dev, B, grid, s, mg, mode, want_dmask=False)
            assert torch.equal(dq, dq2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
            _, _, _, dms = _attention(*dev, B, grid, s, mg, mode, want_dmask=True, inv_scale=_scalar(2.0 ** -7))
            big = (dmask.abs() >= 2.0 ** -100) | (dmask == 0)             # (2^-7 times a value next to fp32's subnormals is not exact)
            assert torch.equal(dms[big], (dmask * 2.0 ** -7)[big]), f"{name}: inv_scale is not an exact factor"
        if variant == "plain":                                        # an all-zero mask gives the unmasked launch's bits
            for m2 in (1, 2):
                zero = torch.zeros(s * s if m2 == 1 else B * (grid // s) ** 2 * br.HEADS * s * s, device="cuda")
                dq0, dk0, dv0, _ = _attention(*dev, B, grid, s, zero, m2, want_dmask=True)
                assert torch.equal(dq, dq0) and torch.equal(dk, dk0) and torch.equal(dv, dv0), f"{name}: zero mask, mode {m2}"


# ================================================================================================================================
# point-query transpose
# ================================================================================================================================
@pytest.mark.parametrize("dtype", br.GDTYPES)
@pytest.mark.parametrize("grid,s", br.PQ_CASES)
def test_point_queries_backward_bit_exact(grid, s, dtype):
    B = 3
    M = (grid // s) ** 2
    dq0 = 50.0 * torch.randn(B * M, br.E, generator=torch.Generator().manual_seed(s + grid))
    dq0[0, :8] = torch.tensor([1e6, -1e6, 65519.0, 65520.0 * 4, 2.0 ** -24, 2.0 ** -26, 0.0, -0.0])     # clamp / subnormal edges
    for inv in (None, 2.0 ** -9):
        dx, dqg, isc = _nan((B, grid * grid, br.E), dtype), dq0.cuda(), (None if inv is None else _scalar(inv))
        _ok(_tl().tp_test_point_queries_bwd(gu.DT[dtype], dqg.data_ptr(), _ptr(isc), dx.data_ptr(), B, grid, s, gu.stream_ptr()),
            "tp_test_point_queries_bwd")
        _sync()
        ref = br.point_queries_bwd_ref(dq0, B, grid, s, 1.0 if inv is None else inv)
        # ("rounded once to T", include/tokenpacker.h: dx is the caller's gradient — IEEE rounding, an fp16 overflow is an inf, not a clamp)
        _same_bits(dx, br.cast_exact(ref, dtype, clamp=False), f"point_queries_bwd {dtype} grid={grid} s={s} inv_scale={inv}")


# ================================================================================================================================
# data-gradient GEMM with the gelu' / out_scale epilogue
# ================================================================================================================================
def _linear_bwd(dy, w, out_dtype, z=None, ldz=0, out_scale=None, tile=0, expect=_capi.TP_OK):
    M, K = dy.shape
    N = w.shape[0]
    C = _nan((M, N), out_dtype)
    rc = _tl().tp_test_linear_bwd(M, N, K, gu.DT[dy.dtype], gu.DT[out_dtype], _capi.TP_LINEAR_GELU_BWD if z is not None else 0, dy.data_ptr(), K,
                                  w.data_ptr(), C.data_ptr(), N, _ptr(z), ldz, _ptr(out_scale), tile, gu.stream_ptr())
    _sync()
    assert rc == expect, f"tp_test_linear_bwd: status {rc}: {_tl().tp_last_error().decode()}"
    return C


def test_gelu_grad_over_every_fp16_value():
    """Operands that make the GEMM result exactly 1.0, z = every finite fp16 value: the output is the rounding of gelu'(z).
    The training epilogue is built for 16-bit outputs only (an fp32 output is refused on the host), so the absolute bound
    6e-7 is met under one output rounding: |err| <= u_T |gelu'(z)| + 6e-7."""
    M = N = 256
    K = 64
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(F16)
    z = torch.where(torch.isfinite(bits), bits, torch.zeros_like(bits)).reshape(M, N)
    zbuf = torch.zeros(M, 2 * N, dtype=F16)
    zbuf[:, N:] = z                                                    # ldz = 2N
    zg = zbuf.cuda()
    ref = br.gelu_grad_ref(z)
    for dt in br.GDTYPES:
        a, w = torch.zeros(M, K, dtype=dt), torch.zeros(N, K, dtype=dt)
        a[:, 3], w[:, 3] = 1.0, 1.0
        for odt in br.GDTYPES:
            outs = []
            for tile in (128, 256):
                got = _linear_bwd(a.cuda(), w.cuda(), odt, zg[:, N:], 2 * N, None, tile)
                _within(got, ref, br.round_bound(ref, odt) + br.GELU_GRAD_ABS, f"gelu' {dt}->{odt} tile {tile}", "gelu'", f"out {str(odt).split('.')[-1]}")
                outs.append(got)
            assert torch.equal(outs[0], outs[1]), "the 128-tile and the ping-pong kernel share the epilogue: same bits"
        # an fp32 output of the training epilogue does not exist: an error code, not a launch
        for tile in (128, 256):
            _linear_bwd(a.cuda(), w.cuda(), F32, zg[:, N:], 2 * N, None, tile, expect=_capi.TP_ERR_INVALID_ARG)


@pytest.mark.parametrize("M,N,K", br.DGRAD_CASES)
def test_linear_bwd_with_gelu_grad_and_out_scale(M, N, K):
    SMALL = 0
    route = _tl().tp_test_gemm_route(M, N, K, _capi.TP_LINEAR_GELU_BWD, 1)
    # the automatic route of the two small launches is the 128-tile kernel, of the two large ones the persistent 256-tile kernel
    assert (route == SMALL) == (M < 4608), f"M={M}: route {route}"
    dev = "cuda" if M >= 4608 else "cpu"
    g = torch.Generator(device=dev).manual_seed(M)
    z = br.gelu_z(M, 2 * N, 3, device=dev)                               # ldz = 2N: the second half is the operand
    sc = 2.0 ** -6
    for dt in br.GDTYPES:
        dy = torch.randn(M, K, generator=g, device=dev).to(dt)
        w = (torch.randn(N, K, generator=g, device=dev) * K ** -0.5).to(dt)
        dyg, wg, zg = dy.cuda(), w.cuda(), z.cuda()
        for odt in br.GDTYPES:
            for zz in (None, z[:, N:]):
                ref, bound = br.linear_bwd_ref(dy, w, zz, 1.0, odt)
                refs, bounds = br.linear_bwd_ref(dy, w, zz, sc, odt)
                zarg = None if zz is None else zg[:, N:]
                tiles = (0, 128, 256) if N % 256 == 0 else (0, 128)
                outs = {}
                for tile in tiles:
                    got = _linear_bwd(dyg, wg, odt, zarg, 2 * N if zz is not None else 0, None, tile)
                    fam = ("gelu'" if zz is not None else "plain") + f" -> {str(odt).split('.')[-1]}"
                    _within(got, ref, bound, f"dgrad {dt}->{odt} {M}x{N}x{K} tile {tile} z={zz is not None}", "dgrad", fam)
                    gots = _linear_bwd(dyg, wg, odt, zarg, 2 * N if zz is not None else 0, _scalar(sc), tile)
                    _within(gots, refs, bounds, f"dgrad out_scale {dt}->{odt} {M}x{N}x{K} tile {tile}", "dgrad", fam + " out_scale")
                    # out_scale multiplies the fp32 result before the ONE rounding: away from fp16's subnormals the scaled output
                    # is exactly 2^-6 times the unscaled one
                    normal = (got.float().abs() * sc >= 2.0 ** -14) | (got.float() == 0) if odt == F16 else torch.ones_like(got, dtype=torch.bool)
                    assert torch.equal(gots.float()[normal], got.float()[normal] * sc), "out_scale is not an exact factor"
                    outs[tile] = got
                for tile in tiles[1:]:
                    assert torch.equal(outs[tile], outs[0]), f"tile {tile} differs from the automatic route"
