"""The forward's two attention kernels under masks that put -inf (or fp32's lowest value, or -1e4) at ANY key position — the whole
first key group of the plain kernel's online softmax included — on a real MI355X, through the test hooks of
include/tokenpacker_test.h (tp_test_region_attention, tp_test_region_attention_absorbed: pass-throughs to the launchers
tp_forward* calls).  The reference is fp64 softmax · V on the same fp16 operands, as in tests/test_gpu_kernels.py, at that test's
tolerance; the masks are tests/mask_patterns.py's (tests/test_mask_patterns_cpu.py: none masks a whole row, the reference is finite)."""
import ctypes
import functools
import math

import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tokenpacker_amd import _capi
from tests import gpu_util as gu
from tests import mask_patterns as mp

pytestmark = pytest.mark.gpu

E, H, D = 1024, 8, 128
TOL = 2.0 ** -11 * 1.05 + 1e-5                     # tests/test_gpu_kernels.py::test_region_attention
F16 = torch.float16
PLAIN_PARAMS = [(c, n) for c in mp.CASES for n in mp.pattern_names(c[1]) + ["random"]]
ABSORBED_PARAMS = [(c, n) for c, n in PLAIN_PARAMS if c[1] ** 2 <= mp.ABSORBED_MAX_KEYS]
_id = lambda p: f"g{p[0][0]}s{p[0][1]}B{p[0][2]}-{p[1]}"      # noqa: E731


def _tl():
    return _capi.load_test_library()


def _ok(rc, what):
    assert rc == _capi.TP_OK, f"{what}: status {rc}: {_tl().tp_last_error().decode()}"


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=F16, device="cuda")


def _masks_of(case, name, value):
    grid, s, B = case
    if name == "random":
        return [(2, mp.mode2_random(grid, s, B, value))]
    return [(1, mp.mode1(name, s, value)), (2, mp.mode2_rows(name, grid, s, B, value))]


def _one_ulp(want: torch.Tensor) -> torch.Tensor:
    """The spacing of fp16 at `want` (fp64 in, fp64 out)."""
    return torch.exp2(torch.floor(torch.log2(want.abs().clamp(min=2.0 ** -14))) - 10)


# ---- plain kernel --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_case(case, qscale=1.0):
    """Operands of one case (device, both K/V layouts) and the mask-independent part of the fp64 reference.  Never modified."""
    grid, s, B = case
    G, S2 = grid // s, s * s
    M, N = G * G, grid * grid
    gen = torch.Generator().manual_seed(100 * grid + s)
    q = (torch.randn(B, M, E, generator=gen) * qscale).half()
    k = torch.randn(B, N, E, generator=gen).half()
    v = torch.randn(B, N, E, generator=gen).half()
    Kr, Vr = orc.region_gather(k, grid, s), orc.region_gather(v, grid, s)        # [B, G, G, S2, E]
    Q = q.double().reshape(B, G, G, H, D) / math.sqrt(D)
    K = Kr.double().reshape(B, G, G, S2, H, D)
    return {"q": q.cuda(), "k": (k.cuda(), Kr.reshape(B, N, E).contiguous().cuda()), "v": (v.cuda(), Vr.reshape(B, N, E).contiguous().cuda()),
            "logits": torch.einsum("bijhd,bijkhd->bijhk", Q, K), "V": Vr.double().reshape(B, G, G, S2, H, D)}


def _plain_ref(c, case, mask, mode):
    grid, s, B = case
    logits = c["logits"] if not mode else c["logits"] + mp.regions(mask, mode, B, grid // s, s)
    P = torch.softmax(logits, dim=-1)
    return torch.einsum("bijhk,bijkhd->bijhd", P, c["V"]).reshape(B, -1, E), P


def _plain_run(c, case, mask, mode, region_major):
    grid, s, B = case
    o = _nan((B, (grid // s) ** 2, E))
    mg = None if mask is None else mask.cuda()
    _ok(_tl().tp_test_region_attention(c["q"].data_ptr(), c["k"][region_major].data_ptr(), c["v"][region_major].data_ptr(), o.data_ptr(),
                                       B, grid, s, None if mg is None else mg.data_ptr(), mode, region_major, gu.stream_ptr()),
        "tp_test_region_attention")
    torch.cuda.synchronize()
    return o


def _check(failures, o, ref, name):
    """Finite everywhere and within TOL of the reference; a failure is collected, so that one run names every failing variant."""
    try:
        assert bool(torch.isfinite(o).all()), f"[{name}] {int((~torch.isfinite(o)).sum())} non-finite outputs of {o.numel()}"
        gu.assert_close(o, ref, name, TOL)
    except AssertionError as e:
        failures.append(str(e).split("\n")[0])
        return False
    return True


@pytest.mark.parametrize("case,name", PLAIN_PARAMS, ids=[_id(p) for p in PLAIN_PARAMS])
def test_region_attention_masked(case, name):
    grid, s, B = case
    c = _plain_case(case)
    G, S2 = grid // s, s * s
    failures = []
    for tag, value in mp.MASKED_VALUES:
        for mode, mask in _masks_of(case, name, value):
            ref, _ = _plain_ref(c, case, mask, mode)
            for rm in (0, 1):
                o = _plain_run(c, case, mask, mode, rm)
                what = f"region_attention {name} {tag} mode {mode} region_major {rm} grid={grid} s={s} B={B}"
                if _check(failures, o, ref, what) and name.startswith("only_key_"):
                    # one visible key: p = 1 exactly (exp(0) = 1, the masked keys' exp underflows to 0, 1 / den = 1), so the
                    # output row IS the visible V row — bit-exact on the GPU (the issue asks for one fp16 ulp)
                    want = c["V"][:, :, :, int(name[9:])].reshape(B, G * G, E)
                    if not torch.equal(o.double().cpu(), want):
                        failures.append(f"[{what}] the output is not the visible V row: max diff {float((o.double().cpu() - want).abs().max()):.3e}")
    assert not failures, f"{len(failures)} variants fail:\n" + "\n".join(failures)


@pytest.mark.parametrize("case", [c for c in mp.CASES if c[1] >= 3], ids=lambda c: f"g{c[0]}s{c[1]}B{c[2]}")
@pytest.mark.parametrize("name", ["lead_4", "lead_5"])
def test_region_attention_masked_peaked(case, name):
    """q scaled by 6 (logits ~ +-60, as test_region_attention_peaked_softmax): after masked leading groups the first rescale of
    the running maximum happens from -inf, and the later ones across large steps."""
    grid, s, B = case
    c = _plain_case(case, 6.0)
    failures = []
    for tag, value in mp.MASKED_VALUES:
        for mode, mask in _masks_of(case, name, value):
            ref, P = _plain_ref(c, case, mask, mode)
            assert float(P.max()) > 0.99                                   # the case really is peaked
            for rm in (0, 1):
                _check(failures, _plain_run(c, case, mask, mode, rm), ref,
                       f"region_attention peaked {name} {tag} mode {mode} region_major {rm} grid={grid} s={s} B={B}")
    assert not failures, f"{len(failures)} variants fail:\n" + "\n".join(failures)


@pytest.mark.parametrize("case", mp.CASES, ids=lambda c: f"g{c[0]}s{c[1]}B{c[2]}")
def test_zero_and_null_mask_are_the_public_kernel(case):
    """Through the hook, no mask and an all-zero mask of either mode reproduce tp_region_attention bit for bit."""
    grid, s, B = case
    c = _plain_case(case)
    M = (grid // s) ** 2
    pub = _nan((B, M, E))
    desc = _capi.make_desc(B, grid, s, 4096, _capi.TP_F16)
    _capi.check(_capi.load_library().tp_region_attention(ctypes.byref(desc), c["q"].data_ptr(), c["k"][0].data_ptr(), c["v"][0].data_ptr(),
                                                         pub.data_ptr(), gu.stream_ptr()), "tp_region_attention")
    torch.cuda.synchronize()
    ref, _ = _plain_ref(c, case, None, 0)
    gu.assert_close(pub, ref, f"tp_region_attention grid={grid} s={s} B={B}", TOL)
    for mode, mask in ((0, None), (1, torch.zeros(s * s)), (2, torch.zeros(M * B * H, s * s))):
        for rm in (0, 1):
            assert torch.equal(_plain_run(c, case, mask, mode, rm), pub), (mode, rm)


# ---- absorbed kernel -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _absorbed_case(case):
    """As test_region_attention_absorbed builds them: rows of H2 with a large common offset and their exact (mean, rstd)."""
    grid, s, B = case
    G, S2 = grid // s, s * s
    M, N = G * G, grid * grid
    gen = torch.Generator().manual_seed(200 * grid + s)
    qt = (0.4 * torch.randn(B, M, H, E, generator=gen)).half()
    h2 = [(1.7 * torch.randn(B, N, E, generator=gen) + 3.0 * torch.randn(B, N, 1, generator=gen)).half() for _ in range(2)]
    mr, n = [], []
    for h in h2:
        hd = h.double()
        st = torch.stack([hd.mean(-1), 1.0 / torch.sqrt(hd.var(-1, unbiased=False) + 1e-6)], dim=-1).float()        # [B, N, 2]
        mr.append(st.reshape(B * N, 2).contiguous())
        n.append(orc.region_gather((hd - st[..., :1].double()) * st[..., 1:].double(), grid, s))                 # [B, G, G, S2, E]
    logits = torch.einsum("bijhe,bijke->bijhk", qt.double().reshape(B, G, G, H, E), n[0]) / math.sqrt(D)
    return {"qt": qt.cuda(), "h2": [h.cuda() for h in h2], "mr": [m.cuda() for m in mr], "logits": logits, "nv": n[1]}


def _absorbed_ref(c, case, mask, mode):
    grid, s, B = case
    logits = c["logits"] if not mode else c["logits"] + mp.regions(mask, mode, B, grid // s, s)
    return torch.einsum("bijhk,bijke->bijhe", torch.softmax(logits, dim=-1), c["nv"]).reshape(-1, E)


def _absorbed_run(c, case, mask, mode, expect=_capi.TP_OK):
    grid, s, B = case
    u = _nan((B * (grid // s) ** 2 * H, E))
    mg = None if mask is None else mask.cuda()
    rc = _tl().tp_test_region_attention_absorbed(c["qt"].data_ptr(), c["h2"][0].data_ptr(), c["h2"][1].data_ptr(), c["mr"][0].data_ptr(),
                                                 c["mr"][1].data_ptr(), u.data_ptr(), B, grid, s, None if mg is None else mg.data_ptr(),
                                                 mode, gu.stream_ptr())
    torch.cuda.synchronize()
    assert rc == expect, f"tp_test_region_attention_absorbed: status {rc}: {_tl().tp_last_error().decode()}"
    return u


@pytest.mark.parametrize("case,name", ABSORBED_PARAMS, ids=[_id(p) for p in ABSORBED_PARAMS])
def test_region_attention_absorbed_masked(case, name):
    grid, s, B = case
    c = _absorbed_case(case)
    G = grid // s
    failures = []
    for tag, value in mp.MASKED_VALUES:
        for mode, mask in _masks_of(case, name, value):
            u = _absorbed_run(c, case, mask, mode)
            what = f"region_attention_absorbed {name} {tag} mode {mode} grid={grid} s={s} B={B}"
            if _check(failures, u, _absorbed_ref(c, case, mask, mode), what) and name.startswith("only_key_"):
                # every head's u is the visible key's normalised V-side row: (h - mean) rstd in fp32 against fp64, one rounding
                want = c["nv"][:, :, :, int(name[9:])].reshape(B * G * G, 1, E).expand(-1, H, -1).reshape(-1, E)
                over = (u.double().cpu() - want).abs() - _one_ulp(want)
                if float(over.max()) > 0:
                    failures.append(f"[{what}] more than one fp16 ulp from the visible row: {float(over.max()):.3e} beyond")
    assert not failures, f"{len(failures)} variants fail:\n" + "\n".join(failures)


@pytest.mark.parametrize("case", [c for c in mp.CASES if c[1] ** 2 <= mp.ABSORBED_MAX_KEYS], ids=lambda c: f"g{c[0]}s{c[1]}B{c[2]}")
def test_absorbed_zero_and_null_mask_are_the_public_kernel(case):
    grid, s, B = case
    c = _absorbed_case(case)
    M = (grid // s) ** 2
    pub = _nan((B * M * H, E))
    desc = _capi.make_desc(B, grid, s, 4096, _capi.TP_F16)
    _capi.check(_capi.load_library().tp_region_attention_absorbed(ctypes.byref(desc), c["qt"].data_ptr(), c["h2"][0].data_ptr(),
                                                                  c["h2"][1].data_ptr(), c["mr"][0].data_ptr(), c["mr"][1].data_ptr(),
                                                                  pub.data_ptr(), gu.stream_ptr()), "tp_region_attention_absorbed")
    torch.cuda.synchronize()
    gu.assert_close(pub, _absorbed_ref(c, case, None, 0), f"tp_region_attention_absorbed grid={grid} s={s} B={B}", TOL)
    for mode, mask in ((0, None), (1, torch.zeros(s * s)), (2, torch.zeros(M * B * H, s * s))):
        assert torch.equal(_absorbed_run(c, case, mask, mode), pub), mode


def test_absorbed_hook_returns_the_launchers_refusal_beyond_64_keys():
    """s*s > 64: the logits of a region no longer fit the kernel's LDS; the launcher refuses on the host and nothing is written."""
    for grid, s in ((18, 9), (24, 12)):
        B, N, M = 1, grid * grid, (grid // s) ** 2
        z = torch.zeros(max(B * N, B * M * H), E, dtype=F16, device="cuda")
        mr = torch.ones(B * N, 2, device="cuda")
        c = {"qt": z, "h2": [z, z], "mr": [mr, mr]}
        u = _absorbed_run(c, (grid, s, B), None, 0, expect=_capi.TP_ERR_INVALID_ARG)
        assert "keys > 64" in _tl().tp_last_error().decode()
        assert bool(torch.isnan(u).all())
