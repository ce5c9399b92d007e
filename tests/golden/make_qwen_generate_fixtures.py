"""Generates tests/golden/qwen_tiny_generate.npz: greedy generate() WITH a repetition penalty by the installed transformers (5.15.0) Qwen2.5-VL on the tiny
model and the prompt of make_qwen_fixtures.py -- the token ids, the raw logits of every step and the scores HF's RepetitionPenaltyLogitsProcessor left.

The penalty is the smallest of 1.05, 1.3, 2.0 for which at least one generated id differs from the unpenalised `gen_output_ids` of qwen_tiny.npz, so that a
generate() that ignores the argument cannot reproduce the ids.  On the deterministic tiny weights that is 1.05 (Qwen2.5-VL's own generation_config.json value):
the unpenalised run repeats token 297 five times, the penalised one moves on after the first (ids 297 144 253 297 144 263 193 297).

Run in the build container only:  python tests/golden/make_qwen_generate_fixtures.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_qwen_fixtures import TINY, build_hf, seq_with_video  # noqa: E402

from oracle.detweights import det_tensor  # noqa: E402  (make_qwen_fixtures put the repository root on sys.path)

import transformers  # noqa: E402

NEW = 8
PENALTIES = (1.05, 1.3, 2.0)


def run(model, ids, px, penalty):
    ids0 = torch.from_numpy(ids[None])
    tt0 = torch.from_numpy(np.where(ids[None] == TINY["video_token_id"], 2, 0)).int()
    kw = dict(repetition_penalty=penalty, output_logits=True, output_scores=True, return_dict_in_generate=True) if penalty is not None else {}
    with torch.no_grad():
        return model.generate(input_ids=ids0, attention_mask=torch.ones_like(ids0), mm_token_type_ids=tt0, pixel_values_videos=px,
                              video_grid_thw=torch.tensor([[2, 8, 12]]), second_per_grid_ts=torch.tensor([1.0]), max_new_tokens=NEW, do_sample=False, **kw)


def main():
    torch.manual_seed(0)
    model, _ = build_hf()
    ids = seq_with_video(2 * 4 * 6, 6, 10, seed=9)                      # the `gen_input_ids` of qwen_tiny.npz
    px = det_tensor("pixel_values_full0", (2 * 8 * 12, 1176), 1.0, seed=5)
    plain = run(model, ids, px, None).numpy()
    gold = np.load(os.path.join(HERE, "qwen_tiny.npz"), allow_pickle=False)
    assert np.array_equal(gold["gen_input_ids"], ids[None]) and np.array_equal(plain[:, :gold["gen_output_ids"].shape[1]], gold["gen_output_ids"])
    for p in PENALTIES:
        o = run(model, ids, px, p)
        seq = o.sequences.numpy()
        if not np.array_equal(seq, plain):
            break
    else:
        raise SystemExit("no penalty of %s changes the greedy ids" % (PENALTIES,))
    out = {"transformers_version": np.array(transformers.__version__), "penalty": np.array(p, dtype=np.float64), "input_ids": ids[None], "plain_ids": plain,
           "ids": seq, "logits": torch.stack(o.logits, 1).numpy().astype(np.float32), "scores": torch.stack(o.scores, 1).numpy().astype(np.float32)}
    np.savez_compressed(os.path.join(HERE, "qwen_tiny_generate.npz"), **out)
    print("wrote qwen_tiny_generate.npz: penalty", p, "ids", seq[0, len(ids):], "plain", plain[0, len(ids):], {k: v.shape for k, v in out.items() if v.ndim})


if __name__ == "__main__":
    main()
