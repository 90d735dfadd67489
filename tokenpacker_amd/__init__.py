"""tokenpacker_amd — MI355X-native (gfx950) TokenPacker region-to-point visual projector.

Public surface mirrors the reference's ``llava/model/multimodal_projector/builder.py``:
``TokenPacker`` and ``build_vision_projector``; plus the batch-shard helper for one-process-per-GPU
runs (``tokenpacker_amd.shard``) and the optimizer of ``use_main_grad`` training (``tokenpacker_amd.optim.MainGradAdamW``, over several ranks ``ShardedMainGradAdamW``).  Importing this package needs neither a GPU nor the built
library; *using* the projector needs both.
"""
from .projector import TokenPacker, build_vision_projector  # noqa: F401
from . import splice  # noqa: F401
from .splice import build_multimodal_inputs, splice_layout  # noqa: F401
from . import loss  # noqa: F401
from .loss import shifted_cross_entropy  # noqa: F401
from . import optim  # noqa: F401
from .optim import MainGradAdamW, ShardedMainGradAdamW, shard_layout, shard_slices  # noqa: F401

__all__ = ["TokenPacker", "build_vision_projector", "splice", "build_multimodal_inputs", "splice_layout", "loss", "shifted_cross_entropy", "optim",
           "MainGradAdamW", "ShardedMainGradAdamW", "shard_layout", "shard_slices"]
__version__ = "0.1.0"
