"""Additive fp32 attention masks that put the masked value at ANY key position — the first key group of the online softmax
included — for the per-kernel and whole-module mask tests (tests/test_gpu_attention_masks.py, tests/test_gpu_forward.py,
tests/test_gpu_mask_train.py); tests/test_mask_patterns_cpu.py proves the conditions on them without a GPU.  No fixtures, no GPU.

Layouts are the library's (include/tokenpacker.h): mode 1 `[S2]`, mode 2 `[(M B) 8, S2]` with row index
(region * B + image) * 8 + head.  A pattern says which keys of ONE row are masked; visible keys carry a `3 * randn` bias."""
import math

import torch

HEADS = 8
KU = 4                                             # the plain kernel's key-group size (csrc/tp_kernels.hip)
NEG_INF = float("-inf")
MASKED_VALUES = (("inf", NEG_INF), ("f32min", torch.finfo(torch.float32).min), ("1e4", -1e4))

# (grid, s, B) of the per-kernel tests: ragged last group | two images | 9 queries: the last workgroup is partial | odd s |
# odd s | the absorbed kernel's largest region | beyond it, plain kernel only (81, 144 keys)
CASES = ((6, 3, 2), (8, 4, 3), (12, 4, 1), (10, 5, 1), (14, 7, 1), (16, 8, 1), (18, 9, 1), (24, 12, 1))
ABSORBED_MAX_KEYS = 64


def pattern_names(s: int):
    """The single-row patterns that exist for an s x s region, in a fixed order."""
    S2 = s * s
    names = [f"lead_{k}" for k in sorted({k for k in (1, 3, 4, 5, 8, S2 - 1) if 0 < k < S2})]
    names += [f"only_key_{j}" for j in sorted({j for j in (0, 3, 4, S2 - 1) if j < S2})]
    return names + ["top_row", "left_col", "mid_group", "tail"]


def masked_keys(name: str, s: int) -> torch.Tensor:
    """Boolean [S2]: True where the pattern masks the key."""
    S2 = s * s
    hit = torch.zeros(S2, dtype=torch.bool)
    if name.startswith("lead_"):
        hit[:int(name[5:])] = True
    elif name.startswith("only_key_"):
        hit[:] = True
        hit[int(name[9:])] = False
    elif name == "top_row":
        hit[:s] = True
    elif name == "left_col":
        hit[::s] = True
    elif name == "mid_group":
        hit[4:8] = True
    elif name == "tail":                            # the whole last group of four, a ragged one included (S2 = 9: key 8)
        hit[(S2 - 1) // KU * KU:] = True
    else:
        raise ValueError(name)
    return hit


def _fill(hit: torch.Tensor, value: float, gen: torch.Generator) -> torch.Tensor:
    bias = 3.0 * torch.randn(hit.shape, generator=gen)
    return torch.where(hit, torch.full_like(bias, value), bias)


def mode1(name: str, s: int, value: float, seed: int = 0) -> torch.Tensor:
    """fp32 [S2]: the pattern for every image, region and head."""
    return _fill(masked_keys(name, s), value, torch.Generator().manual_seed(1000 + seed))


def mode2_rows(name: str, grid: int, s: int, B: int, value: float, seed: int = 0) -> torch.Tensor:
    """fp32 [(M B) 8, S2]: the pattern on every row (each head its own bias on the visible keys)."""
    rows = (grid // s) ** 2 * B * HEADS
    return _fill(masked_keys(name, s).expand(rows, s * s), value, torch.Generator().manual_seed(2000 + seed))


def planted_rows(grid: int, s: int, B: int) -> dict:
    """{row index: pattern} of the random mode-2 mask: one row of every single-row pattern at fixed rows — the first and the last
    row of the mask, and two heads (one of the low, one of the high four) of one query among them."""
    rows = (grid // s) ** 2 * B * HEADS
    names = pattern_names(s)
    q = (rows // HEADS) // 2                        # a query in the middle
    fixed = [0, rows - 1, q * HEADS + 1, q * HEADS + 6]
    step = max(1, (rows - 2) // (len(names) + 1))
    at, used = {}, set()
    for i, n in enumerate(names):
        r = fixed[i] if i < len(fixed) else 1 + (i - len(fixed)) * step
        while r in used:
            r += 1
        assert r < rows, (grid, s, B, n)
        used.add(r)
        at[r] = n
    return at


def random_hit(grid: int, s: int, B: int, seed: int = 0) -> torch.Tensor:
    """Boolean [(M B) 8, S2] of the random mode-2 pattern: each entry masked with probability 0.5, each row's guaranteed-visible
    key drawn uniformly over ALL positions, the planted rows on top."""
    S2 = s * s
    rows = (grid // s) ** 2 * B * HEADS
    gen = torch.Generator().manual_seed(3000 + seed)
    hit = torch.rand(rows, S2, generator=gen) < 0.5
    keep = torch.randint(0, S2, (rows,), generator=gen)
    hit[torch.arange(rows), keep] = False
    for r, n in planted_rows(grid, s, B).items():
        hit[r] = masked_keys(n, s)
    return hit


def mode2_random(grid: int, s: int, B: int, value: float, seed: int = 0) -> torch.Tensor:
    """fp32 [(M B) 8, S2]: `random_hit` with the masked value, `3 * randn` elsewhere."""
    return _fill(random_hit(grid, s, B, seed), value, torch.Generator().manual_seed(4000 + seed))


def mode2_bool(grid: int, s: int, B: int, seed: int = 0) -> torch.Tensor:
    """The random mode-2 pattern as the 3-D boolean attn_mask of nn.MultiheadAttention, [(M B) 8, 1, S2] (True = masked)."""
    return random_hit(grid, s, B, seed).unsqueeze(1)


def top_row_2d(s: int, value: float = NEG_INF, seed: int = 0) -> torch.Tensor:
    """`top_row` as the 2-D additive float attn_mask, [1, S2]."""
    return mode1("top_row", s, value, seed).reshape(1, s * s)


def masks(grid: int, s: int, B: int, value: float):
    """Every (name, mode, mask) of one case and one masked value."""
    for n in pattern_names(s):
        yield n, 1, mode1(n, s, value)
        yield n, 2, mode2_rows(n, grid, s, B, value)
    yield "random", 2, mode2_random(grid, s, B, value)


def regions(mask: torch.Tensor, mode: int, B: int, G: int, s: int) -> torch.Tensor:
    """The mask as float64 [B, G, G, 8, S2] (the layout of the references' logits)."""
    S2 = s * s
    m = mask.double()
    if mode == 1:
        return m.reshape(1, 1, 1, 1, S2).expand(B, G, G, HEADS, S2)
    return m.reshape(G * G, B, HEADS, S2).permute(1, 0, 2, 3).reshape(B, G, G, HEADS, S2)


def attention_ref(q, k_regions, v_regions, mask, mode, s):
    """fp64 softmax(q k^T / sqrt(d) + mask) v: q [B, G, G, 8, d], k / v [B, G, G, S2, 8, d] -> (o [B, G, G, 8, d], P)."""
    B, G = q.shape[0], q.shape[1]
    logits = torch.einsum("bijhd,bijkhd->bijhk", q.double(), k_regions.double()) / math.sqrt(q.shape[-1])
    if mode:
        logits = logits + regions(mask, mode, B, G, s)
    P = torch.softmax(logits, dim=-1)
    return torch.einsum("bijhk,bijkhd->bijhd", P, v_regions.double()), P
