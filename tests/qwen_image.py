"""Shared helpers for the image / mixed image + video fixtures (tests/golden/qwen_image.npz, made by tests/golden/make_qwen_image_fixtures.py)."""
import os

import numpy as np
import torch

from oracle.detweights import det_tensor

GOLD_PATH = os.path.join(os.path.dirname(__file__), "golden", "qwen_image.npz")
VIT_KEYS = ("img1", "img2", "multi", "big")


def gold_image():
    return np.load(GOLD_PATH, allow_pickle=False)


def vit_pixels(gi, key):
    """The pixels of a ViT case (every image of the call in one tensor), drawn as the generator draws them."""
    return det_tensor(f"pixel_values_{key}", (int(np.prod(gi[f"{key}_grid"], axis=1).sum()), 1176), 1.0, seed=5)


def batch_pixels(gi, tag, kinds=("image", "video")):
    """pixel_values (images in batch order) and pixel_values_videos (videos in batch order) of a fixture batch, drawn as the generator draws them."""
    out = []
    for kind, seed in zip(kinds, (5, 6)):
        grid = gi[f"{tag}_{kind}_grid"]
        px = [det_tensor(f"pixel_values_{tag}_{'img' if kind == 'image' else 'vid'}{i}", (int(np.prod(g)), 1176), 1.0, seed=seed) for i, g in enumerate(grid)]
        out.append(torch.cat(px, 0))
    return out
