"""The weight-gradient contraction dW = dY^T · X at its edges, on a real MI355X, through tp_test_wgrad (include/tokenpacker_test.h:
a pass-through to wgrad_tt_launch / wgrad_tn_launch, the objects and kernels tp_backward runs) against fp64 math on the same rounded
operands (tests/bwd_ref.py: wgrad_ref, the `ints` and `gauss` operand families).

The harness of every case:
  * dy and x are VIEWS into larger allocations in which every element the contraction must not use is NaN: the rows from R to
    S * Ks + 64 (a wrong num_records in a K-tile's descriptor reads them), the CLS rows and the batches behind the last one of a
    batch-strided x, the other columns of a wider dy.  The allocations reach that far, so a wrong mask reads a NaN — which no sum
    survives — and never leaves the allocation: these tests cannot fault.  (The transposed form's X^T carries ZEROS beyond column R,
    the caller's contract; its dy rows beyond R are NaN all the same — 0 * NaN is NaN, so dy must be masked.)
  * the split partials start as NaN; what lies behind the S partials the plan announces must still be NaN afterwards;
  * every output starts as NaN (or as known integers, to accumulate onto) and is followed by a canary that must come back as it was;
  * the (S, Ks) of tp_test_wgrad_plan is asserted against the value the case is named for (worked out by hand from the rule).
`ints` must come out BIT FOR BIT (fp32: the fp64 reference itself; 16 bits: its one rounding) — one token row dropped, doubled or
misplaced fails that at any R; `gauss` within the tolerances of tests/test_gpu_wgrad.py (bwd_ref.WGRAD_TOL), the worst error of each
output dtype printed (`[wgrad-gauss] ...`, pytest -s).

What notices which mistake (scratch builds of tp_gemm8.hip's issue(), profiles/README.md, tag wg1): adding one to `bidx` fails every
case with more than one batch (8 of the 72); dropping BOTH clamps of the descriptor length (rows_left to [0, 64] and nrec >= 0)
fails the 36 cases in which a whole K-tile lies beyond R; dropping the rows_left clamp alone changes nothing — a negative length is
clamped again, and the lanes address 64 rows whatever the length says.  R = 18432 = 16 * 1152 masks no row: 16385 is its ragged twin."""
import ctypes

import pytest
import torch

from tokenpacker_amd import _capi
from tests import bwd_ref as br

pytestmark = pytest.mark.gpu

F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
DT = {BF16: _capi.TP_BF16, F16: _capi.TP_F16, F32: _capi.TP_F32}
NAN = float("nan")
CANARY = 2048                                      # elements behind every output: 4 KiB of 16-bit values, 8 KiB of fp32
DTYPES = (BF16, F16)
WORST = {}


def _tl():
    return _capi.load_test_library()


def _plan(rows, n_out, k_in, transposed=0, rpad=0):
    s, ks = ctypes.c_int(-1), ctypes.c_longlong(-1)
    rc = _tl().tp_test_wgrad_plan(rows, n_out, k_in, transposed, rpad, ctypes.byref(s), ctypes.byref(ks))
    assert rc == _capi.TP_OK, _tl().tp_last_error().decode()
    return s.value, ks.value


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


class Case:
    """The operands of one case in their allocations, the launch arguments that address them, the plan and the fp64 reference.
    layout: "rows" (x contiguous) | "batched" (x = hidden[:, 1:] of a [B, rpb + 1, k_in] tensor) | "parts" (the same, k_in spread
    over four separately allocated tensors) | "transposed" (X^T [k_in, rpad], zero beyond column R)."""

    def __init__(self, family, dtype, R, n_out, k_in, want, *, layout="rows", ldy=None, col0=0, rpb=0, rpad=0, seed=0,
                 operands=None, ref=None):
        self.family, self.dtype, self.R, self.n_out, self.k_in, self.layout = family, dtype, R, n_out, k_in, layout
        self.transposed = int(layout == "transposed")
        self.S, self.Ks = _plan(R, n_out, k_in, self.transposed, rpad)
        assert (self.S, self.Ks) == tuple(want), f"plan {(self.S, self.Ks)} is not the {tuple(want)} this case is named for"
        span = rpad if self.transposed else self.S * self.Ks
        assert span >= R
        rows_alloc = span + 64
        dyv, xv = operands if operands is not None else br.wgrad_operands(family, R, n_out, k_in, dtype, 1000 * seed + R, "cuda")
        self.dyv, self.xv = dyv, xv
        self.ldy = n_out if ldy is None else ldy
        self.dy_full = _nan((rows_alloc, self.ldy), dtype)
        self.dy = self.dy_full[:, col0:col0 + n_out]
        self.dy[:R] = dyv
        self.rpb, self.bstride, self.parts, self.n_part = 0, 0, (None,) * 4, 0
        if layout == "rows":
            self.x_full = _nan((rows_alloc, k_in), dtype)
            self.x_full[:R] = xv
            self.x, self.ldx = self.x_full, k_in
        elif layout in ("batched", "parts"):
            assert R % rpb == 0
            B, B_alloc = R // rpb, -(-rows_alloc // rpb) + 1
            np_ = k_in // 4 if layout == "parts" else k_in
            hidden = [_nan((B_alloc, rpb + 1, np_), dtype) for _ in range(k_in // np_)]           # separate allocations
            for i, h in enumerate(hidden):
                h[:B, 1:] = xv[:, i * np_:(i + 1) * np_].reshape(B, rpb, np_)
            self.hidden = hidden
            self.rpb, self.bstride, self.ldx = rpb, (rpb + 1) * np_, np_
            if layout == "parts":
                self.x, self.parts, self.n_part = None, tuple(h[:, 1:] for h in hidden), np_
            else:
                self.x = hidden[0][:, 1:]
        else:
            self.x_full = torch.zeros(k_in, rpad, dtype=dtype, device="cuda")
            self.x_full[:, :R] = xv.t()
            self.x, self.ldx = self.x_full, rpad
        self.ref = br.wgrad_ref(dyv, xv, R) if ref is None else ref
        lib = _capi.load_library()
        self.used = self.S * n_out * k_in                                     # floats of `part` the plan announces
        ws = lib.tp_wgrad_workspace_bytes(n_out, k_in) // 4
        self.part_floats = ws if ws * 4 <= (64 << 20) else self.used          # (the full-size cases: what the plan needs, no more)
        assert self.used <= self.part_floats

    def sink(self, out_dtype, prior=None):
        """[n_out * k_in | canary]: NaN (or `prior`), then CANARY known values."""
        n = self.n_out * self.k_in
        buf = torch.empty(n + CANARY, dtype=out_dtype, device="cuda")
        buf[:n] = NAN if prior is None else prior.reshape(-1)
        buf[n:] = (torch.arange(CANARY, device="cuda") % 251 + 1).to(out_dtype)
        return buf

    def launch(self, buf, out_dtype, *, split_row=0, lo=True, hi=False, out_scale=None, accumulate=False, counters=None,
               expect=_capi.TP_OK):
        """One tp_test_wgrad into `buf` (a sink): grad_out = buf (if `lo`), grad_out_hi = buf + split_row * k_in (if `hi`) — the two
        sides of a split are neighbours in ONE buffer, so a side that must not be written is watched as closely as the canary."""
        n = self.n_out * self.k_in
        canary = buf[n:].clone()
        part = _nan((self.part_floats + CANARY,), F32)
        part[self.part_floats:] = 7.0
        esz = buf.element_size()
        p = lambda t: None if t is None else t.data_ptr()                    # noqa: E731
        rc = _tl().tp_test_wgrad(
            self.dy.data_ptr(), self.ldy, p(self.x), self.ldx, self.rpb, self.bstride, *[p(t) for t in self.parts], self.n_part,
            self.R, self.n_out, self.k_in, DT[self.dtype], DT[out_dtype], buf.data_ptr() if lo else None,
            buf.data_ptr() + split_row * self.k_in * esz if hi else None, split_row, p(out_scale), int(accumulate), p(counters),
            0 if counters is None else counters.numel(), part.data_ptr(), self.part_floats * 4, self.transposed,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == expect, f"tp_test_wgrad: status {rc}: {_tl().tp_last_error().decode()}"
        assert torch.equal(buf[n:], canary), "the canary behind the output was written"
        assert bool((part[self.part_floats:] == 7.0).all()), "the canary behind the partials was written"
        if rc == _capi.TP_OK:
            assert not bool(torch.isnan(part[:self.used]).any()), "a NaN in the split partials: a masked element was read"
            assert bool(torch.isnan(part[self.used:self.part_floats]).all()), "partials were written behind the S the plan announces"
        else:
            assert bool(torch.isnan(part[:self.part_floats]).all()) and bool(torch.isnan(buf[:n].float()).all()), "a refused call wrote"
        return buf[:n].reshape(self.n_out, self.k_in)

    def run(self, out_dtype, **kw):
        return self.launch(self.sink(out_dtype), out_dtype, **kw)

    def check(self, got, out_dtype, scale=1.0, name=""):
        """`ints`: bit for bit; `gauss`: max-norm error <= WGRAD_TOL[out_dtype] of max|ref|.  scale: an out_scale the launch had."""
        what = f"{name} {self.family} {self.dtype} -> {out_dtype} R={self.R} {self.n_out}x{self.k_in} {self.layout} S={self.S} Ks={self.Ks}"
        assert not bool(torch.isnan(got.float()).any()), f"{what}: NaN in the result — an element outside the contraction was read"
        ref = self.ref * scale
        if self.family == "ints":
            assert torch.equal(ref.float().double(), ref), "the scaled reference is not exact in fp32"
            if out_dtype == F16:
                assert float(ref.abs().max()) < 65504.0                        # (no fp16 clamp in play: the rounding is all there is)
            want = ref.float().to(out_dtype)
            bad = int((got != want).sum())
            assert bad == 0, f"{what}: {bad} elements differ from the exact result; first at {torch.nonzero(got != want)[:4].tolist()}"
        else:
            err = float((got.double() - ref).abs().max() / ref.abs().max())
            WORST[out_dtype] = max(WORST.get(out_dtype, 0.0), err)
            print(f"[wgrad-gauss] {what} err {err:.3e} worst {out_dtype} {WORST[out_dtype]:.3e}")
            assert err <= br.WGRAD_TOL[out_dtype], f"{what}: {err:.3e} > {br.WGRAD_TOL[out_dtype]:.3e}"


def _sweep(R, n_out, k_in, want, **kw):
    """Both operand dtypes, both families, fp32 and 16-bit output."""
    for dtype in DTYPES:
        for family in br.WGRAD_FAMILIES:
            c = Case(family, dtype, R, n_out, k_in, want, **kw)
            for out_dtype in (F32, dtype):
                c.check(c.run(out_dtype), out_dtype)


# ---- row edges ---------------------------------------------------------------------------------------------------------------------
# (R, n_out, k_in, (S, Ks)).  R = 1025: the last split holds 7 full K-tiles, one K-tile of a single row and one of none (the
# rows_left = 1 and = 0 descriptors).  R = 8193: 16 splits of 576 rows would leave the last one without a row; the rule halves S.
ROW_CASES = [(R, 256, 256, want) for R, want in (
    (1, (1, 64)), (63, (1, 64)), (64, (1, 64)), (65, (1, 128)), (127, (1, 128)), (129, (1, 192)), (1023, (1, 1024)),
    (1024, (2, 512)), (1025, (2, 576)), (2047, (2, 1024)), (2048, (4, 512)), (2049, (4, 576)), (8191, (8, 1024)),
    (8193, (8, 1088)), (16384, (16, 1024)), (16385, (16, 1088)), (18432, (16, 1152)))] + [(3000, 512, 768, (4, 768))]


@pytest.mark.parametrize("R,n_out,k_in,want", ROW_CASES, ids=[f"R{c[0]}-S{c[3][0]}" for c in ROW_CASES])
def test_row_edges_in_place(R, n_out, k_in, want):
    _sweep(R, n_out, k_in, want, seed=1)


# ---- column edges ------------------------------------------------------------------------------------------------------------------
# (n_out, k_in, ldy, col0): a tile that overhangs n_out inside a wider dy (its other columns NaN: nothing of them may reach a stored
# element), dy as the right and as the left half of a matrix twice as wide, more than one tile in both directions
COL_CASES = [(8, 256, 512, 0), (264, 256, 512, 0), (256, 256, 512, 256), (256, 256, 512, 0), (512, 1024, 512, 0), (512, 1024, 1024, 512)]


@pytest.mark.parametrize("n_out,k_in,ldy,col0", COL_CASES)
@pytest.mark.parametrize("R,want", [(129, (1, 192)), (1025, (2, 576))])
def test_column_edges(n_out, k_in, ldy, col0, R, want):
    _sweep(R, n_out, k_in, want, ldy=ldy, col0=col0, seed=2)


# ---- batch-strided x ---------------------------------------------------------------------------------------------------------------
# (rows_per_batch, batches, (S, Ks)): 2, 3 and 9 K-tiles per batch for the magic-number division; one batch; 5 * 576 with the split
# boundaries (768, 1536, 2304) inside batches; 9 * 128 with the boundary (576) inside a batch; 300 and 576 K-tiles in all
BATCH_CASES = [(128, 1, (1, 128)), (192, 1, (1, 192)), (576, 1, (1, 576)), (128, 9, (2, 576)), (576, 5, (4, 768)),
               (192, 100, (16, 1216)), (576, 64, (16, 2304))]


@pytest.mark.parametrize("rpb,B,want", BATCH_CASES)
def test_batch_strided_x(rpb, B, want):
    _sweep(rpb * B, 256, 256, want, layout="batched", rpb=rpb, seed=3)


@pytest.mark.parametrize("rpb", [96, 100])
def test_batch_strided_x_refuses_partial_k_tiles(rpb):
    """A batch that is not whole 64-row K-tiles cannot be read in place: refused on the host, nothing written."""
    c = Case("ints", BF16, 5 * 192, 256, 256, (1, 960), layout="batched", rpb=192, seed=3)
    c.rpb = rpb                                                               # (the allocation and its stride stay; the launch argument lies)
    c.run(F32, expect=_capi.TP_ERR_INVALID_ARG)
    msg = _tl().tp_last_error().decode()
    assert msg.startswith("tp wgrad: unsupported shape") and "batches of a multiple of 64 rows" in msg, msg


# ---- four-part x -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rpb,B,want", [(192, 3, (1, 576)), (576, 5, (4, 768))])
def test_four_part_x(dtype, rpb, B, want):
    """k_in = 1024 from four separately allocated [B, T + 1, 256] tensors: `ints` equal the contraction over their torch.cat bit
    for bit; on `gauss` the parts launch and the launch on the one concatenated tensor give the same bits."""
    R = rpb * B
    for family in br.WGRAD_FAMILIES:
        four = Case(family, dtype, R, 256, 1024, want, layout="parts", rpb=rpb, seed=4)
        one = Case(family, dtype, R, 256, 1024, want, layout="batched", rpb=rpb, operands=(four.dyv, four.xv))
        for out_dtype in (F32, dtype):
            a, b = four.run(out_dtype), one.run(out_dtype)
            four.check(a, out_dtype, name="parts")
            assert torch.equal(a, b), f"{family} {dtype} -> {out_dtype}: four parts and their torch.cat differ"


# ---- split_row / grad_out_hi -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("split_row", [256, 8, 504])
def test_split_row_routes_two_parameters(dtype, split_row):
    """n_out = 512 behind one contraction, rows [0, split_row) to grad_out and the rest to grad_out_hi: each side is bit-equal to
    its rows of the unsplit launch; a NULL side is not written (it lies between the other side and the canary, still NaN)."""
    n_out, k_in, R = 512, 256, 1025
    for family in br.WGRAD_FAMILIES:
        c = Case(family, dtype, R, n_out, k_in, (2, 576), seed=5)
        for out_dtype in (F32, dtype):
            whole = c.run(out_dtype)
            c.check(whole, out_dtype, name="unsplit")
            both = c.run(out_dtype, split_row=split_row, lo=True, hi=True)
            assert torch.equal(both, whole)
            low = c.run(out_dtype, split_row=split_row, lo=True, hi=False)
            assert torch.equal(low[:split_row], whole[:split_row]) and bool(torch.isnan(low[split_row:].float()).all())
            high = c.run(out_dtype, split_row=split_row, lo=False, hi=True)
            assert torch.equal(high[split_row:], whole[split_row:]) and bool(torch.isnan(high[:split_row].float()).all())


# ---- out_scale ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,want", [(1025, (2, 576)), (129, (1, 192))])
def test_out_scale(dtype, R, want):
    """A power of two is exact (`ints`: 2^-7 and 2^5); 1 / 3 on `gauss` against fp64 times the fp32 value of 1 / 3."""
    ints, gauss = (Case(f, dtype, R, 256, 256, want, seed=6) for f in br.WGRAD_FAMILIES)
    for out_dtype in (F32, dtype):
        for s in (2.0 ** -7, 2.0 ** 5):
            sc = torch.tensor([s], dtype=F32, device="cuda")
            ints.check(ints.run(out_dtype, out_scale=sc), out_dtype, scale=s, name=f"out_scale {s}")
        third = torch.tensor([1.0 / 3.0], dtype=F32, device="cuda")
        gauss.check(gauss.run(out_dtype, out_scale=third), out_dtype, scale=float(third.double()), name="out_scale 1/3")


# ---- accumulate --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,want", [(1025, (2, 576)), (8191, (8, 1024))])
def test_accumulate_onto_an_fp32_sink(dtype, R, want):
    c = Case("ints", dtype, R, 256, 256, want, seed=7)
    prior = torch.randint(-1000, 1001, (256, 256), device="cuda", generator=torch.Generator("cuda").manual_seed(R)).float()
    buf = c.sink(F32, prior)
    once = c.launch(buf, F32, accumulate=True)
    assert torch.equal(once.double(), prior.double() + c.ref), "prior + dW"
    twice = c.launch(buf, F32, accumulate=True)
    assert torch.equal(twice.double(), prior.double() + 2 * c.ref), "prior + 2 dW"
    half = torch.tensor([0.5], dtype=F32, device="cuda")
    thrice = c.launch(buf, F32, accumulate=True, out_scale=half)              # (2 dW + dW / 2 stays exact: integers / 2 below 2^24)
    assert torch.equal(thrice.double(), prior.double() + 2.5 * c.ref), "prior + 2.5 dW"
    c.run(dtype, accumulate=True, expect=_capi.TP_ERR_INVALID_ARG)           # a 16-bit sink cannot accumulate: refused, nothing written
    assert "accumulate needs an fp32 output" in _tl().tp_last_error().decode()


# ---- tile queue --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,n_out,k_in,want", [(1025, 256, 256, (2, 576)), (2049, 512, 768, (4, 576)), (129, 4352, 4352, (1, 192)),
                                                (8191, 256, 256, (8, 1024))])
def test_tile_queue_counters(R, n_out, k_in, want):
    """S <= 4: a zeroed 32-int counters slot (dynamic per-XCD tile queue) and NULL (static tile lists) give identical bits, a second
    launch on a fresh slot again; 4352 x 4352 has 289 tiles, more than the chip has CUs — the only launch here whose workgroups
    draw from the queue, and its slot shows the draws.  S > 4: the launcher passes no queue on; the slot comes back untouched."""
    for family, dtype in (("ints", BF16), ("gauss", F16)):
        c = Case(family, dtype, R, n_out, k_in, want, seed=8)
        static = c.run(F32)
        c.check(static, F32, name="static")
        for attempt in range(2):
            slot = torch.zeros(32, dtype=torch.int32, device="cuda") if c.S <= 4 else torch.full((32,), 77, dtype=torch.int32, device="cuda")
            queued = c.run(F32, counters=slot)
            assert torch.equal(queued, static), f"{family} launch {attempt}: the tile queue changed the result"
            if c.S > 4:
                assert bool((slot == 77).all()), "S > 4: the counters slot was touched"
            elif n_out * k_in > 256 * 256 * 256:
                assert int(slot.sum()) > 0 and bool((slot[8 * c.S:] == 0).all()), slot.tolist()
            else:
                assert bool((slot == 0).all()), slot.tolist()                  # (one tile per workgroup: nothing is drawn)


# ---- transposed form ---------------------------------------------------------------------------------------------------------------
# (R, rpad, (S, Ks)): rpad = ceil1024(R), and 2048 columns more (rpad must stay a multiple of 1024) — whole splits of zero padding
TN_CASES = [(1, 1024, (4, 256)), (1, 3072, (8, 384)), (100, 1024, (4, 256)), (100, 3072, (8, 384)), (1024, 1024, (4, 256)),
            (1024, 3072, (8, 384)), (1025, 2048, (8, 256)), (1025, 4096, (16, 256)), (4608, 5120, (16, 320)), (4608, 7168, (16, 448))]


@pytest.mark.parametrize("R,rpad,want", TN_CASES)
def test_transposed_form(R, rpad, want):
    """wgrad_tn_launch: X^T zero-padded to rpad columns (the caller's contract), dy read in place with NaN rows from R on."""
    _sweep(R, 256, 256, want, layout="transposed", rpad=rpad, seed=9)


# ---- full size ---------------------------------------------------------------------------------------------------------------------
def test_full_size_both_forms():
    """The reference's per-GPU batch on the first K/V layer's weight, (R, n_out, k_in) = (18432, 2048, 4096): 128 tiles, two splits
    of 9216 rows.  `ints`, bf16: exact, where the whole backward's 1e-2 gate would let a lost token row (0.74 %) pass."""
    R, n_out, k_in = 18432, 2048, 4096
    a = Case("ints", BF16, R, n_out, k_in, (2, 9216), seed=10)
    for out_dtype in (F32, BF16):
        a.check(a.run(out_dtype), out_dtype, name="in place")
    b = Case("ints", BF16, R, n_out, k_in, (2, 9216), layout="transposed", rpad=R, operands=(a.dyv, a.xv), ref=a.ref)
    for out_dtype in (F32, BF16):
        b.check(b.run(out_dtype), out_dtype, name="transposed")
