"""The masks of tests/mask_patterns.py are what the GPU tests need them to be — conditions on the INPUTS, established without the
kernel: no row of any (pattern, case, masked value) is fully masked, every `lead_k` with k >= 4 (and `top_row` at s >= 4) really
covers the plain kernel's first key group, the planted rows sit where they should, and the fp64 reference output is finite
everywhere."""
import pytest
import torch

from oracle import tokenpacker_oracle as orc
from tests import mask_patterns as mp


def _is_masked(mask, value):
    return mask == value


@pytest.mark.parametrize("grid,s,B", mp.CASES)
def test_pattern_names_and_keys(grid, s, B):
    S2 = s * s
    names = mp.pattern_names(s)
    assert len(names) == len(set(names))
    for k in (1, 3, 4, 5, 8, S2 - 1):
        assert (f"lead_{k}" in names) == (0 < k < S2)
    for j in (0, 3, 4, S2 - 1):
        assert f"only_key_{j}" in names
    for n in names:
        hit = mp.masked_keys(n, s)
        assert hit.shape == (S2,) and bool(hit.any()) and not bool(hit.all()), n
        if n.startswith("lead_"):
            k = int(n[5:])
            assert int(hit.sum()) == k and bool(hit[:k].all())
            assert bool(hit[:mp.KU].all()) == (k >= mp.KU)               # k >= 4 really covers the first group of four
        if n.startswith("only_key_"):
            assert int((~hit).sum()) == 1 and not bool(hit[int(n[9:])])
    assert bool(mp.masked_keys("top_row", s)[:mp.KU].all()) == (s >= mp.KU)
    assert mp.masked_keys("top_row", s).nonzero().flatten().tolist() == list(range(s))
    assert mp.masked_keys("left_col", s).nonzero().flatten().tolist() == list(range(0, S2, s))
    assert mp.masked_keys("mid_group", s).nonzero().flatten().tolist() == [4, 5, 6, 7]
    tail = mp.masked_keys("tail", s).nonzero().flatten().tolist()
    assert tail[-1] == S2 - 1 and tail[0] % mp.KU == 0 and len(tail) == (S2 - 1) % mp.KU + 1
    if S2 == 9:
        assert tail == [8]


@pytest.mark.parametrize("grid,s,B", mp.CASES)
def test_planted_rows_and_the_random_pattern(grid, s, B):
    S2, rows = s * s, (grid // s) ** 2 * B * mp.HEADS
    at = mp.planted_rows(grid, s, B)
    assert sorted(at.values()) == sorted(mp.pattern_names(s))            # one row of every single-row pattern
    assert 0 in at and rows - 1 in at and max(at) < rows
    queries = [r // mp.HEADS for r in at]
    shared = [q for q in set(queries) if queries.count(q) >= 2]
    assert any({r % mp.HEADS < 4 for r in at if r // mp.HEADS == q} == {True, False} for q in shared)   # both halves of a lane's heads
    hit = mp.random_hit(grid, s, B)
    assert hit.shape == (rows, S2) and not bool(hit.all(1).any())
    for r, n in at.items():
        assert torch.equal(hit[r], mp.masked_keys(n, s)), (r, n)
    free = torch.ones(rows, dtype=torch.bool)
    free[list(at)] = False
    assert 0.35 < float(hit[free].float().mean()) < 0.55                 # p = 0.5, one entry per row forced visible
    assert bool(hit[free][:, 0].any())                                   # key 0 is not pinned
    if rows >= 96:                                                       # (enough rows for a 1-in-16 event)
        assert bool(hit[free][:, :mp.KU].all(1).any())                   # a whole first group masked happens by chance too
    assert torch.equal(mp.mode2_bool(grid, s, B), hit.unsqueeze(1))


@pytest.mark.parametrize("tag,value", mp.MASKED_VALUES)
@pytest.mark.parametrize("grid,s,B", mp.CASES)
def test_no_row_is_fully_masked_and_the_reference_is_finite(grid, s, B, tag, value):
    S2, G, d = s * s, grid // s, 128
    M = G * G
    gen = torch.Generator().manual_seed(7)
    q = torch.randn(B, M, mp.HEADS * d, generator=gen).half()
    k = torch.randn(B, grid * grid, mp.HEADS * d, generator=gen).half()
    v = torch.randn(B, grid * grid, mp.HEADS * d, generator=gen).half()
    Q = q.double().reshape(B, G, G, mp.HEADS, d)
    K = orc.region_gather(k.double(), grid, s).reshape(B, G, G, S2, mp.HEADS, d)
    V = orc.region_gather(v.double(), grid, s).reshape(B, G, G, S2, mp.HEADS, d)
    seen = []
    for name, mode, mask in mp.masks(grid, s, B, value):
        seen.append((name, mode))
        assert mask.dtype == torch.float32 and mask.shape == ((S2,) if mode == 1 else (M * B * mp.HEADS, S2))
        rows = mask.reshape(-1, S2)
        hit = _is_masked(rows, value)
        assert not bool(hit.all(1).any()), (name, mode)                  # no fully masked row
        assert bool(torch.isfinite(rows[~hit]).all()) and float(rows[~hit].abs().max()) < 20.0
        if name != "random":
            assert bool((hit == mp.masked_keys(name, s)).all()), (name, mode)
        if (name.startswith("lead_") and int(name[5:]) >= mp.KU) or (name == "top_row" and s >= mp.KU):
            assert bool(hit[:, :mp.KU].all()), (name, mode)              # the first group carries the masked value in EVERY row
        o, P = mp.attention_ref(Q, K, V, mask, mode, s)
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(P).all()), (name, mode)
        if value == mp.NEG_INF or value == torch.finfo(torch.float32).min:
            assert float(P[mp.regions(hit.reshape(mask.shape).float(), mode, B, G, s) > 0].max()) == 0.0   # masked keys weigh nothing
    assert len(seen) == 2 * len(mp.pattern_names(s)) + 1


def test_module_masks():
    for s in (3, 4, 12):
        m2 = mp.top_row_2d(s)
        assert m2.shape == (1, s * s) and bool(torch.isinf(m2[0, :s]).all()) and bool(torch.isfinite(m2[0, s:]).all())
        m3 = mp.mode2_bool(24, s, 2)
        assert m3.dtype == torch.bool and m3.shape == ((24 // s) ** 2 * 2 * 8, 1, s * s) and not bool(m3.all(-1).any())
