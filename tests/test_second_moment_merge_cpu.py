"""The second-moment merge of the triangular statistics path, restated in numpy.

A triangular statistics GEMM leaves 16 fp32 partial sums of squares per row (one per 64 output columns, accumulated per lane
with two running sums — the halves of a packed FMA — then added over the 4 lane groups); ln_finalize, the 128-tile kernel's
in-kernel merge and the decoupled V launch add the 16 partials as a balanced tree over the part index and return
rstd = 1 / sqrt(sum / n + eps).  This file pins that order and its accuracy against fp64 on rows with mean 0 and with a mean of
40 sigma (on the centred chain the quantity wanted IS the second moment of y = R h + c~, so the mean-dominated row is one whose
second moment is dominated by one direction: nothing cancels, whatever the mean)."""
import numpy as np

PARTS, N, EPS = 16, 1024, 1e-6
f32 = np.float32


def lane_partial(v):
    """One lane's 16 values of a 64-column slice (4 fragments x 4 consecutive columns), fp32: packed FMA halves, then their sum."""
    s = np.zeros(2, f32)
    for frag in v.reshape(4, 4):
        for pair in (frag[0:2], frag[2:4]):
            # (fma(x, x, s) rounds once; fp64 product + fp32 rounding of the sum reproduces it for fp32 inputs)
            s = (pair.astype(np.float64) ** 2 + s.astype(np.float64)).astype(f32)
    return f32(s[0] + s[1])


def wave_partial(cols64):
    """A wave's 64-column partial of one row: lane group g owns columns j*16 + g*4 .. +3 of fragment j; xor 16, then xor 32."""
    lanes = [lane_partial(np.concatenate([cols64[j * 16 + g * 4: j * 16 + g * 4 + 4] for j in range(4)])) for g in range(4)]
    a, b = f32(lanes[0] + lanes[1]), f32(lanes[2] + lanes[3])      # xor 16: (0,1) (2,3)
    return f32(a + b)                                              # xor 32


def tree_sum(parts):
    """ln_second_moment_rstd: a balanced tree over the part index."""
    v = [f32(x) for x in parts]
    assert len(v) == PARTS
    a = [f32(f32(v[4 * k] + v[4 * k + 1]) + f32(v[4 * k + 2] + v[4 * k + 3])) for k in range(4)]
    return f32(f32(a[0] + a[1]) + f32(a[2] + a[3]))


def merge(parts, inv_dim=f32(1.0 / N), eps=f32(EPS)):
    var = f32(np.float64(tree_sum(parts)) * np.float64(inv_dim) + np.float64(eps))       # fmaf(ss, inv_dim, eps)
    return f32(1.0) / np.sqrt(var, dtype=f32)


def rstd_fp32(row):
    return merge([wave_partial(row[p * 64:(p + 1) * 64]) for p in range(PARTS)])


def rstd_fp64(row):
    r = row.astype(np.float64)
    return 1.0 / np.sqrt((r * r).sum() / N + EPS)


def test_merge_order_is_a_balanced_tree():
    """2^24 followed by fifteen ones: added one after the other every 1 is rounded away; the tree keeps 2 + 4 + 4 + 4."""
    v = np.ones(PARTS, f32)
    v[0] = f32(2.0 ** 24)
    seq = f32(0)
    for x in v:
        seq = f32(seq + x)
    assert seq == f32(2.0 ** 24)
    assert tree_sum(v) == f32(2.0 ** 24 + 14)


def test_second_moment_rstd_against_fp64():
    """Bound: the sum of 1024 non-negative terms by a depth-10 tree of fp32 adds (4 in the lane, 2 across the lane groups,
    4 over the parts) carries at most ~(1 + 10) rounding steps of 2^-24 each on every term, all of one sign: a relative error of
    at most 11 * 2^-24 in the sum, half of that in rstd, plus the rounding of the scale, the rsqrt and the division (3 more
    half-ulps): 8.5 * 2^-24 < 6e-7.  The same bound serves both rows: a sum of squares does not cancel."""
    rng = np.random.default_rng(5)
    bound = 6e-7
    worst = {}
    for name, mean in (("mean 0", 0.0), ("mean 40 sigma", 40.0)):
        w = 0.0
        for _ in range(24):
            row = (rng.standard_normal(N) + mean).astype(f32)
            w = max(w, abs(float(rstd_fp32(row)) / rstd_fp64(row) - 1.0))
        worst[name] = w
    print("\n[second-moment merge] worst relative error of rstd:", {k: f"{v:.2e}" for k, v in worst.items()}, f"bound {bound:.1e}")
    assert all(v <= bound for v in worst.values()), worst
