"""The weight-gradient contraction's host side, without a GPU: the split rule both launchers use (tp_test_wgrad_plan calls it) against
the workspace contract of tp_wgrad_workspace_bytes, the host-side refusals of tp_test_wgrad, and the `ints` operand family of
tests/bwd_ref.py (what makes the GPU tests' bit-for-bit comparison sensitive to a single token row)."""
import ctypes

import pytest
import torch

from tokenpacker_amd import _capi
from tests import bwd_ref as br

E = _capi.TP_ERR_INVALID_ARG
SHAPES = ((8, 256), (256, 256), (264, 512), (1024, 1024), (2048, 4096), (4096, 4096))
MAX_ROWS = 40000


def _plan(tl, rows, n_out, k_in, transposed=0, rpad=0):
    s, ks = ctypes.c_int(-1), ctypes.c_longlong(-1)
    rc = tl.tp_test_wgrad_plan(rows, n_out, k_in, transposed, rpad, ctypes.byref(s), ctypes.byref(ks))
    assert rc == _capi.TP_OK, tl.tp_last_error().decode()
    return s.value, ks.value


@pytest.mark.parametrize("n_out,k_in", SHAPES)
@pytest.mark.parametrize("transposed", [0, 1])
def test_plan_fits_the_workspace_and_covers_every_row(n_out, k_in, transposed):
    """Over every R in 1 .. 40000: S in {1, 2, 4, 8, 16}, Ks whole K-tiles that fit an int, S * Ks >= R, no empty split (in-place
    form; the transposed form splits rpad = ceil1024(R), where S * Ks = rpad exactly), and S partials fit tp_wgrad_workspace_bytes."""
    lib, tl = _capi.load_library(), _capi.load_test_library()
    ws = lib.tp_wgrad_workspace_bytes(n_out, k_in)
    assert ws == 16 * n_out * k_in * 4
    seen = set()
    for R in range(1, MAX_ROWS + 1):
        rpad = (R + 1023) // 1024 * 1024
        S, Ks = _plan(tl, R, n_out, k_in, transposed, rpad if transposed else 0)
        seen.add(S)
        what = (R, n_out, k_in, transposed, S, Ks)
        assert S in (1, 2, 4, 8, 16), what
        assert Ks > 0 and Ks % 64 == 0 and Ks < 2 ** 31, what
        assert S * Ks >= R, what
        if transposed:
            assert S * Ks == rpad, what
        else:
            assert (S - 1) * Ks < R, what
        assert S * n_out * k_in * 4 <= ws, what
    tiles = (n_out + 255) // 256 * (k_in // 256)
    allowed = {s for s in (1, 2, 4, 8, 16) if s == 1 or tiles * s // 2 < 256}      # (doubling stops once S * tiles fills 256 CUs)
    # in place every allowed S occurs over these R; rpad >= 1024 columns are split as far as the tiles allow from the start
    assert (seen <= allowed and max(seen) == max(allowed)) if transposed else seen == allowed, (seen, tiles)


def test_plan_values_the_gpu_cases_are_named_for():
    """The (S, Ks) the rule gives at the row counts tests/test_gpu_wgrad_edges.py exercises, worked out by hand from the rule as
    tp_train.hip documents it: in place, S doubles while a split keeps >= 512 rows and S * tiles < 256, Ks = ceil64(ceil(R / S)),
    and S is halved again while the last split would own no row; transposed, S doubles while rpad / S stays a multiple of 64
    columns and >= 256, Ks = rpad / S."""
    tl = _capi.load_test_library()
    for R, want in ((1, (1, 64)), (64, (1, 64)), (65, (1, 128)), (1023, (1, 1024)), (1024, (2, 512)), (1025, (2, 576)),
                    (2047, (2, 1024)), (2048, (4, 512)), (2049, (4, 576)), (4096, (8, 512)), (8191, (8, 1024)), (8192, (16, 512)),
                    (16384, (16, 1024)), (16385, (16, 1088)), (18432, (16, 1152)), (36864, (16, 2304))):
        assert _plan(tl, R, 256, 256) == want, R
    # S = 16 splits of ceil64(ceil(R / 16)) rows would leave the last one past R: 15 * 576 >= 8193, 8640; 8 splits it is
    assert _plan(tl, 8193, 256, 256) == (8, 1088) and _plan(tl, 8640, 256, 256) == (8, 1088) and _plan(tl, 8641, 256, 256) == (16, 576)
    assert _plan(tl, 3000, 512, 768) == (4, 768)                       # 6 tiles
    assert _plan(tl, 18432, 2048, 4096) == (2, 9216)                   # 128 tiles: two splits fill the chip
    assert _plan(tl, 18432, 4096, 4096) == (1, 18432)                  # 256 tiles
    assert _plan(tl, 18432, 512, 1024) == (16, 1152)
    for R, rpad, want in ((1, 1024, (4, 256)), (1, 3072, (8, 384)), (1025, 2048, (8, 256)), (1025, 4096, (16, 256)),
                          (4608, 5120, (16, 320)), (4608, 7168, (16, 448)), (36864, 36864, (16, 2304))):
        assert _plan(tl, R, 256, 256, 1, rpad) == want, (R, rpad)
    assert _plan(tl, 18432, 2048, 4096, 1, 18432) == (2, 9216)
    s, ks = ctypes.c_int(), ctypes.c_longlong()
    for args in ((0, 256, 256, 0, 0), (100, 0, 256, 0, 0), (100, 256, 0, 0, 0), (100, 260, 256, 0, 0), (100, 256, 200, 0, 0),
                 (100, 256, 256, 2, 0), (100, 256, 256, 1, 1000), (2000, 256, 256, 1, 1024)):
        assert tl.tp_test_wgrad_plan(*args, ctypes.byref(s), ctypes.byref(ks)) == E, args
        assert tl.tp_last_error().decode().startswith("tp_test_wgrad_plan"), args
    assert tl.tp_test_wgrad_plan(100, 256, 256, 0, 0, None, ctypes.byref(ks)) == E


# (dy, ldy, x, ldx, rows_per_batch, batch_stride, x_part0..3, n_part, rows, n_out, k_in, dtype, out_dtype, grad_out, grad_out_hi,
#  split_row, out_scale, accumulate, counters, counter_ints, part, part_bytes, transposed, stream)
P, ODD, P256 = 4096, 4104, 8192                   # fake device pointers: aligned | 8 bytes off | 256-byte aligned; never dereferenced
I = dict(dy=0, ldy=1, x=2, ldx=3, rpb=4, bstride=5, p0=6, p1=7, p2=8, p3=9, n_part=10, rows=11, n_out=12, k_in=13, dtype=14,
         out_dtype=15, grad_out=16, grad_out_hi=17, split_row=18, out_scale=19, accumulate=20, counters=21, counter_ints=22, part=23,
         part_bytes=24, transposed=25, stream=26)


def _good(**over):
    a = [P, 512, P, 1024, 0, 0, None, None, None, None, 0, 3000, 512, 1024, _capi.TP_BF16, _capi.TP_F32, P, None, 0, None, 0,
         None, 0, P256, 16 * 512 * 1024 * 4, 0, None]
    for k, v in over.items():
        a[I[k]] = v
    return a


def test_wgrad_hook_refuses_on_the_host():
    """Everything the launchers leave to tp_backward, tp_test_wgrad refuses itself — TP_ERR_INVALID_ARG and a message that names
    the hook (or, for a shape, the launcher), before anything is enqueued: no device is touched here."""
    tl = _capi.load_test_library()

    def refused(why, **over):
        assert tl.tp_test_wgrad(*_good(**over)) == E, over
        msg = tl.tp_last_error().decode()
        assert why in msg and msg.startswith(("tp_test_wgrad", "tp wgrad")), (over, msg)

    for name in ("dy", "x", "grad_out", "part"):
        refused("NULL", **{name: None})
    refused("NULL", split_row=256, grad_out=None, grad_out_hi=None)               # (with a split, ONE side may be NULL)
    refused("without a split_row", grad_out_hi=P)
    for name in ("dy", "x", "grad_out"):
        refused("16-byte aligned", **{name: ODD})
    refused("16-byte aligned", split_row=256, grad_out_hi=ODD)
    refused("256-byte aligned", part=P + 16)
    refused("4-byte aligned", out_scale=P + 2)
    refused("4-byte aligned", counters=P + 2, counter_ints=32)
    refused("32 zeroed ints", counters=P, counter_ints=31)
    refused("accumulate needs an fp32 output", accumulate=1, out_dtype=_capi.TP_BF16)
    refused("accumulate needs an fp32 output", accumulate=1, out_dtype=_capi.TP_F16)
    refused("accumulate 0 / 1", accumulate=2)
    refused("dtype", dtype=_capi.TP_F32)
    refused("dtype", out_dtype=3)
    parts = dict(x=None, p0=P, p1=P, p2=P, p3=P, n_part=256, ldx=256)
    refused("not four parts", transposed=1, **parts)
    refused("no split_row", transposed=1, ldx=3072, split_row=256, grad_out_hi=P)
    refused("no batch stride", transposed=1, ldx=3072, rpb=576, bstride=577 * 1024)
    refused("all four", **dict(parts, p2=None))
    refused("all four", **dict(parts, x=P))
    refused("n_part > 0", **dict(parts, n_part=0))
    refused("16-byte aligned", **dict(parts, p3=ODD))
    refused("split_row must lie", split_row=512)
    refused("split_row must lie", split_row=-8)
    refused("ldy < n_out", ldy=504)
    refused("shorter than a row", ldx=1016)
    refused("batch_stride must cover", rpb=576, bstride=575 * 1024)
    refused("rpad", transposed=1, ldx=2048)                                       # (ldx = rpad < rows)
    # shapes: the launchers' own host-side refusals, passed on
    refused("unsupported shape", k_in=1000, ldx=1000)
    refused("unsupported shape", n_out=508)
    refused("unsupported shape", ldy=516)
    refused("batches of a multiple of 64 rows", rpb=96, bstride=97 * 1024)
    refused("batches of a multiple of 64 rows", rpb=100, bstride=101 * 1024)
    refused("batches of a multiple of 64 rows", rpb=64, bstride=65 * 1024)        # (one K-tile per batch: not served)
    refused("unsupported shape", transposed=1, ldx=3000)                          # (rpad % 1024)
    assert tl.tp_test_wgrad(*_good(part_bytes=4 * 512 * 1024 * 4 - 1)) == _capi.TP_ERR_WORKSPACE     # (R = 3000, 8 tiles: S = 4)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ints_family_is_exact_and_row_dependent(dtype):
    """The `ints` operands: integers in [-2, 2] that survive the rounding to 16 bits, pairwise distinct outer products, and a
    contraction that fp32 arithmetic gets exactly right in ANY order (here: torch's, and a reversed one) — while dropping, doubling
    or mis-pairing ONE row moves the exact result."""
    rows, n_out, k_in = 3000, 16, 256
    dy, x = br.wgrad_operands("ints", rows, n_out, k_in, dtype, seed=5)
    for t in (dy, x):
        assert t.dtype == dtype and torch.equal(t.float(), t.float().round()) and float(t.float().abs().max()) == 2.0
    assert torch.unique(x[:, :1 + br.WGRAD_DIGITS].float(), dim=0).shape[0] == rows           # the stamped digits tell the rows apart
    assert bool((dy[:, 0] == 1).all()) and bool((x[:, 0] == 1).all())
    ref = br.wgrad_ref(dy, x, rows)
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2 ** 24
    assert torch.equal((dy.float().t() @ x.float()).double(), ref)
    assert torch.equal((dy.float().flip(0).t() @ x.float().flip(0)).double(), ref)
    assert torch.equal(br.wgrad_ref(dy, x, rows, chunk=7), ref)
    # rows beyond `rows` are not read
    junk = torch.full((5, n_out), float("nan"), dtype=dtype)
    assert torch.equal(br.wgrad_ref(torch.cat([dy, junk]), torch.cat([x, torch.full((5, k_in), float("nan"), dtype=dtype)]), rows), ref)
    # one row dropped / counted twice / paired with its neighbour's x: the exact result moves
    assert not torch.equal(br.wgrad_ref(dy, x, rows - 1), ref)
    twice = torch.cat([dy, dy[1234:1235]]), torch.cat([x, x[1234:1235]])
    assert not torch.equal(br.wgrad_ref(*twice, rows + 1), ref)
    xs = x.clone()
    xs[[100, 101]] = x[[101, 100]]
    assert not torch.equal(br.wgrad_ref(dy, xs, rows), ref)
    g1, g2 = br.wgrad_operands("gauss", 64, 8, 256, dtype, seed=5)
    assert g1.dtype == dtype and g2.shape == (64, 256) and 0.8 < float(g2.float().std()) < 1.2
