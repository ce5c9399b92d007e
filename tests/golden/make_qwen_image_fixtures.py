"""Generates tests/golden/qwen_image.npz: the installed transformers (5.15.0) Qwen2.5-VL on IMAGE inputs (pixel_values / image_grid_thw) and on
batches that mix images and videos -- same tiny config and deterministic weights as make_qwen_fixtures.py (whose qwen_tiny.npz holds video forwards only).

Run in the build container only:  python tests/golden/make_qwen_image_fixtures.py
Weights are NOT stored: they are regenerated from parameter names by oracle/detweights.py.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from oracle.detweights import det_tensor  # noqa: E402

import transformers  # noqa: E402
from transformers.vision_utils import get_vision_cu_seqlens, get_vision_position_ids, get_vision_window_index  # noqa: E402

from make_qwen_fixtures import TINY, build_hf, hf_name_to_ckpt, seq_with_video  # noqa: E402,F401

IMG, VID, VS = TINY["image_token_id"], TINY["video_token_id"], TINY["vision_start_token_id"]

# ViT grids (t = 1): partial windows on both axes / one merged token / three images of different sizes in one call / one >= 1024-key full-attention segment
VIT_GRIDS = {"img1": [[1, 10, 14]], "img2": [[1, 2, 2]], "multi": [[1, 2, 2], [1, 10, 14], [1, 6, 6]], "big": [[1, 36, 36]]}


def n_tokens(g):
    t, h, w = g
    return t * (h // 2) * (w // 2)


def seq(parts, seed):
    """parts: ("text", n) | ("image", grid) | ("video", grid); every vision run is preceded by vision_start (as the processor emits it)."""
    g = np.random.default_rng(seed)
    out = []
    for kind, a in parts:
        if kind == "text":
            out.append(g.integers(0, 300, a))
        else:
            out.append([VS])
            out.append(np.full(n_tokens(a), IMG if kind == "image" else VID))
    return np.concatenate(out).astype(np.int64)


def pad_batch(rows, left):
    S = max(len(r) for r in rows)
    ids = np.zeros((len(rows), S), dtype=np.int64)
    am = np.zeros((len(rows), S), dtype=np.int64)
    for b, (r, lp) in enumerate(zip(rows, left)):
        if lp:
            ids[b, S - len(r):] = r; am[b, S - len(r):] = 1
        else:
            ids[b, :len(r)] = r; am[b, :len(r)] = 1
    return ids, am


def token_types(ids, am):
    return torch.from_numpy((np.where(ids == IMG, 1, 0) + np.where(ids == VID, 2, 0)) * am).int()


def vid_px(name, g):
    return det_tensor(name, (int(np.prod(g)), 1176), 1.0, seed=6)


def img_px(name, g):
    return det_tensor(name, (int(np.prod(g)), 1176), 1.0, seed=5)


# the mixed batches (grids chosen so that the hf449 and hf515 temporal rules coincide: integer second_per_grid_t, temporal extent below the spatial one)
ROPE_ROWS = ([("text", 5), ("image", [1, 10, 14]), ("text", 7)],
             [("text", 4), ("video", [2, 8, 12]), ("text", 3), ("image", [1, 2, 2]), ("text", 6)])
MIX_ROWS = ([("text", 5), ("image", [1, 10, 14]), ("text", 12)],
            [("text", 4), ("video", [2, 8, 12]), ("text", 3), ("image", [1, 6, 6]), ("text", 8)])
GEN_MIX_ROWS = ([("text", 3), ("image", [1, 6, 6]), ("text", 5)],
                [("text", 4), ("video", [2, 8, 12]), ("text", 6)])
GEN_IMG_ROW = [("text", 5), ("image", [1, 10, 14]), ("text", 7)]


def grids_of(rows, kind):
    return [a for r in rows for k, a in r if k == kind]


def pixels(rows, tag):
    """pixel_values (images in batch order) and pixel_values_videos (videos in batch order) of a batch."""
    im = [img_px(f"pixel_values_{tag}_img{i}", g) for i, g in enumerate(grids_of(rows, "image"))]
    vd = [vid_px(f"pixel_values_{tag}_vid{i}", g) for i, g in enumerate(grids_of(rows, "video"))]
    return (torch.cat(im, 0) if im else None), (torch.cat(vd, 0) if vd else None)


def main():
    torch.manual_seed(0)
    model, _ = build_hf()
    out = {"transformers_version": np.array(transformers.__version__)}

    # ---- vision index + forward on image grids
    for key, g in VIT_GRIDS.items():
        gt = torch.tensor(g)
        wi, cw = get_vision_window_index(gt, 2, 112, 14)
        out[f"{key}_grid"] = np.array(g)
        out[f"{key}_window_index"] = wi.numpy()
        out[f"{key}_cu_window"] = cw.numpy()
        out[f"{key}_cu_full"] = get_vision_cu_seqlens(gt).numpy()
        out[f"{key}_pos_ids"] = get_vision_position_ids(gt, 2).numpy()
        n = int(np.prod(np.array(g), axis=1).sum())
        px = det_tensor(f"pixel_values_{key}", (n, 1176), 1.0, seed=5)
        with torch.no_grad():
            vo = model.model.visual(px, grid_thw=gt)
        out[f"{key}_pooler"] = vo.pooler_output.numpy()
        if len(g) == 1:
            out[f"{key}_last_hidden"] = vo.last_hidden_state.numpy()

    # ---- rope index: row 0 text / image / text right-padded, row 1 text / video / text / image / text left-padded
    ids, am = pad_batch([seq(r, seed=20 + i) for i, r in enumerate(ROPE_ROWS)], left=(False, True))
    ig, vg = grids_of(ROPE_ROWS, "image"), grids_of(ROPE_ROWS, "video")
    pos, delta = model.model.get_rope_index(torch.from_numpy(ids), mm_token_type_ids=token_types(ids, am), image_grid_thw=torch.tensor(ig),
                                            video_grid_thw=torch.tensor(vg), second_per_grid_ts=torch.tensor([1.0]), attention_mask=torch.from_numpy(am))
    out.update(rope_img_input_ids=ids, rope_img_attention_mask=am, rope_img_image_grid=np.array(ig), rope_img_video_grid=np.array(vg),
               rope_img_spg=np.array([1.0], dtype=np.float32), rope_img_position_ids=pos.numpy(), rope_img_deltas=delta.numpy())

    # ---- full forward, B = 2 padded: sample 0 image only (right-padded), sample 1 video + image (left-padded); labels on the last 8 valid tokens
    ids, am = pad_batch([seq(r, seed=30 + i) for i, r in enumerate(MIX_ROWS)], left=(False, True))
    labels = np.full_like(ids, -100)
    for b in range(2):
        v = np.flatnonzero(am[b])[-8:]
        labels[b, v] = ids[b, v]
    ig, vg = grids_of(MIX_ROWS, "image"), grids_of(MIX_ROWS, "video")
    px, pxv = pixels(MIX_ROWS, "mix")
    spg = torch.tensor([1.0])
    pos, _ = model.model.get_rope_index(torch.from_numpy(ids), mm_token_type_ids=token_types(ids, am), image_grid_thw=torch.tensor(ig),
                                        video_grid_thw=torch.tensor(vg), second_per_grid_ts=spg, attention_mask=torch.from_numpy(am))
    with torch.no_grad():
        o = model(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(am), position_ids=pos, labels=torch.from_numpy(labels),
                  pixel_values=px, image_grid_thw=torch.tensor(ig), pixel_values_videos=pxv, video_grid_thw=torch.tensor(vg),
                  second_per_grid_ts=spg, output_hidden_states=True)
    out.update(mix_input_ids=ids, mix_attention_mask=am, mix_labels=labels, mix_image_grid=np.array(ig), mix_video_grid=np.array(vg),
               mix_position_ids=pos.numpy(), mix_logits=o.logits.numpy(), mix_loss=o.loss.numpy(), mix_hidden_last=o.hidden_states[-1].numpy())

    # ---- greedy generate, 6 tokens: one unpadded image prompt; a left-padded B = 2 batch (image prompt, video prompt)
    ids = seq(GEN_IMG_ROW, seed=40)[None]
    px, _ = pixels([GEN_IMG_ROW], "gen_img")
    ig = grids_of([GEN_IMG_ROW], "image")
    with torch.no_grad():
        gen = model.generate(input_ids=torch.from_numpy(ids), attention_mask=torch.ones(ids.shape, dtype=torch.long), mm_token_type_ids=token_types(ids, np.ones_like(ids)),
                             pixel_values=px, image_grid_thw=torch.tensor(ig), max_new_tokens=6, do_sample=False)
    out.update(gen_img_input_ids=ids, gen_img_image_grid=np.array(ig), gen_img_output_ids=gen.numpy())

    ids, am = pad_batch([seq(r, seed=60 + i) for i, r in enumerate(GEN_MIX_ROWS)], left=(True, True))
    px, pxv = pixels(GEN_MIX_ROWS, "gen_mix")
    ig, vg = grids_of(GEN_MIX_ROWS, "image"), grids_of(GEN_MIX_ROWS, "video")
    with torch.no_grad():
        gen = model.generate(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(am), mm_token_type_ids=token_types(ids, am),
                             pixel_values=px, image_grid_thw=torch.tensor(ig), pixel_values_videos=pxv, video_grid_thw=torch.tensor(vg),
                             second_per_grid_ts=torch.tensor([1.0]), max_new_tokens=6, do_sample=False)
    out.update(gen_mix_input_ids=ids, gen_mix_attention_mask=am, gen_mix_image_grid=np.array(ig), gen_mix_video_grid=np.array(vg),
               gen_mix_output_ids=gen.numpy())

    np.savez_compressed(os.path.join(HERE, "qwen_image.npz"), **out)
    print("wrote qwen_image.npz", {k: v.shape for k, v in out.items() if v.ndim > 0})


if __name__ == "__main__":
    main()
