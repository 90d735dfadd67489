"""The reference's HD loader for ONE raw RGB image, restated in torch on the CPU — what ``hd.slice_images`` is tested against.

``train.py:696`` runs ``Compose([ToTensor(), Normalize(CLIP mean, CLIP std)])``; torchvision is not a dependency of this
repository, so the two transforms are restated with the torch ops they run, in their order: ``ToTensor`` on a uint8 HWC image is
``permute(2, 0, 1).contiguous().to(float32).div(255)`` and ``Normalize`` is ``sub_(mean[:, None, None]).div_(std[:, None, None])``
with ``mean`` / ``std`` as fp32 tensors.  The slicing behind it (``train.py:699-731``) is ``oracle.hd_oracle.slice_image`` with the
grid ``hd.select_grid`` picks (pinned against the reference by ``tests/golden/hd_grid.json``)."""
import torch

from oracle import hd_oracle
from tokenpacker_amd import hd


def to_tensor_normalize(u8: torch.Tensor, mean=hd.CLIP_MEAN, std=hd.CLIP_STD) -> torch.Tensor:
    """``[H, W, 3]`` uint8 -> ``[3, H, W]`` fp32, ``Compose([ToTensor(), Normalize(mean, std)])``."""
    t = u8.permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m, s = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return t.sub_(m[:, None, None]).div_(s[:, None, None])


def slice_reference(u8: torch.Tensor, patch_num: int = 9, block: int = 336):
    """-> ``(crops [n, 3, block, block] fp32, h_block, w_block)`` of the reference's loader for one uint8 image."""
    H, W = int(u8.shape[0]), int(u8.shape[1])
    hb, wb = hd.select_grid(H, W, patch_num, block)
    return hd_oracle.slice_image(to_tensor_normalize(u8).unsqueeze(0), hb, wb, block), hb, wb


def random_image(h: int, w: int, seed: int = 0) -> torch.Tensor:
    """A seeded ``[h, w, 3]`` uint8 image with every byte value present (given enough pixels)."""
    g = torch.Generator().manual_seed(1000003 * h + 101 * w + seed)
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g)
