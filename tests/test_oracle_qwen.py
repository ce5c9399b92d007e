"""CPU: pins the Qwen2.5-VL oracle (oracle/qwen25vl.py) against golden vectors produced by the installed
transformers 5.15.0 implementation (tests/golden/make_qwen_fixtures.py).  Integer outputs bit-exact; fp32 <= 1e-4."""
import os

import numpy as np
import pytest
import torch

from oracle import qwen25vl as Q
from oracle.detweights import det_state_dict, det_tensor

GOLD = os.path.join(os.path.dirname(__file__), "golden", "qwen_tiny.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD, allow_pickle=False)


def tiny_cfg():
    return Q.QwenCfg(
        vision=Q.VisionCfg(depth=4, hidden_size=64, num_heads=4, intermediate_size=88, patch_size=14, temporal_patch_size=2,
                           spatial_merge_size=2, window_size=112, fullatt_block_indexes=(1, 3), out_hidden_size=96,
                           in_channels=3, tokens_per_second=2),
        text=Q.TextCfg(hidden_size=96, num_hidden_layers=2, num_attention_heads=6, num_key_value_heads=2, intermediate_size=160,
                       vocab_size=320, rms_norm_eps=1e-6, rope_theta=1000000.0, mrope_section=(2, 3, 3)),
        image_token_id=301, video_token_id=302, vision_start_token_id=303)


def tiny_params(gold):
    shapes = {str(n): eval(str(s)) for n, s in zip(gold["param_names"], gold["param_shapes"])}
    return det_state_dict(shapes, seed=1)


@pytest.mark.parametrize("key", ["a", "b", "c", "full16"])
def test_vision_index_plumbing_bit_exact(gold, key):
    g = gold[f"g4_{key}_grid"]
    wi, cw = Q.vision_window_index(g, 2, 112, 14)
    assert np.array_equal(wi, gold[f"g4_{key}_window_index"])
    assert np.array_equal(cw, gold[f"g4_{key}_cu_window"])
    assert np.array_equal(Q.vision_cu_seqlens(g), gold[f"g4_{key}_cu_full"])
    assert np.array_equal(Q.vision_position_ids(g, 2), gold[f"g4_{key}_pos_ids"])


@pytest.mark.parametrize("key", ["a", "b"])
@pytest.mark.parametrize("rule", ["hf515", "hf449"])
def test_rope_index_bit_exact(gold, key, rule):
    pos, delta = Q.rope_index(gold[f"rope_{key}_input_ids"], tiny_cfg(), None, gold[f"rope_{key}_grid"], gold[f"rope_{key}_spg"],
                              gold[f"rope_{key}_attention_mask"], temporal_rule=rule)
    assert np.array_equal(pos, gold[f"rope_{key}_position_ids"])
    assert np.array_equal(delta, gold[f"rope_{key}_deltas"])


@pytest.mark.parametrize("key", ["a", "b"])
def test_vit_forward(gold, key):
    cfg, P = tiny_cfg(), tiny_params(gold)
    g = gold[f"g4_{key}_grid"]
    px = det_tensor(f"pixel_values_{key}", (int(np.prod(g[0])), 1176), 1.0, seed=5)
    out, pre = Q.vit_forward(P, px, g, cfg, return_pre_merge=True)
    assert np.abs(out.numpy() - gold[f"vit_{key}_pooler"]).max() < 1e-4
    assert np.abs(pre.numpy() - gold[f"vit_{key}_last_hidden"]).max() < 1e-4


def test_full_forward_and_loss(gold):
    cfg, P = tiny_cfg(), tiny_params(gold)
    px = torch.cat([det_tensor("pixel_values_full0", (192, 1176), 1.0, seed=5), det_tensor("pixel_values_full1", (192, 1176), 1.0, seed=6)], 0)
    r = Q.forward(P, cfg, torch.from_numpy(gold["full_input_ids"]), torch.from_numpy(gold["full_attention_mask"]),
                  labels=torch.from_numpy(gold["full_labels"]), pixel_values_videos=px, video_grid_thw=gold["full_grid"],
                  second_per_grid_ts=np.array([1.0, 1.0]))
    assert np.array_equal(r["position_ids"].numpy(), gold["full_position_ids"])
    am = gold["full_attention_mask"].astype(bool)
    assert np.abs(r["hidden"].numpy() - gold["full_hidden_last"])[am].max() < 2e-4
    assert np.abs(r["logits"].numpy() - gold["full_logits"])[am].max() < 2e-4
    assert abs(float(r["loss"]) - float(gold["full_loss"])) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The bf16-STORAGE mode of the oracle (oracle.qwen25vl.storage), pinned to transformers' own bf16 run.  The full-depth GPU test
# (tests/test_fulldepth_parity_gpu.py) states its bound against what bf16 storage costs the fp32 restatement; that yardstick must be reference-derived, not
# builder-defined.  Fixture: tests/golden/qwen_mid_bf16.npz -- the installed transformers Qwen2.5-VL at a mid size (8 ViT blocks d = 256, 12 decoder layers d = 512,
# conditioned random weights) run on the CPU in bf16 and, same weights, in fp32 (tests/golden/make_qwen_mid_bf16_fixtures.py).
@pytest.fixture(scope="module")
def mid():
    from tests import qwen_mid as QM

    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    g = QM.gold()
    P, cfg, px = QM.params(g), QM.oracle_cfg(), QM.pixel_values(g)
    ids = torch.from_numpy(g["input_ids"])
    am, pos = torch.ones_like(ids), torch.from_numpy(g["position_ids"])

    def run():
        with torch.no_grad():
            e = Q.vit_forward(P, px, g["grid"], cfg)
            x = P["model.embed_tokens.weight"][ids]
            x[ids == QM.VIDEO_TOKEN] = e
            hs = []
            hid = Q.llm_forward(P, x, pos, am, cfg, hidden_states=hs)[0]
            lg = hid @ P["lm_head.weight"].t()
        return {"vit": e, "hidden4": hs[4][0], "hidden8": hs[8][0], "hidden12": hid, "logits_tail": lg[-32:]}

    o32 = run()
    with Q.storage(torch.bfloat16):
        o16 = run()
        o16["logits_tail"] = Q._r(o16["logits_tail"])
    return {"g": g, "P": P, "px": px, "am": am, "pos": pos, "o32": o32, "o16": o16, "QM": QM}


POINTS = ("vit", "hidden4", "hidden8", "hidden12", "logits_tail")


def test_mid_size_fp32_restatement_equals_transformers_fp32(mid):
    g, QM = mid["g"], mid["QM"]
    for k in POINTS:
        assert QM.rel(mid["o32"][k], g[k + "_fp32"]) < 2e-6, k


def test_bf16_storage_mode_one_block_at_a_time_against_transformers_bf16(mid):
    """Teacher-forced: every pinned block / layer of transformers' bf16 run is re-run by the oracle ON THAT RUN'S OWN INPUT.  In storage mode the output must equal
    the stored bf16 output up to rounding flips of differently-ordered fp32 sums (measured 2.1 - 2.6e-4 for a ViT block, 5.2 - 5.4e-4 for a decoder layer); in
    plain fp32 mode the same block sits 2.3e-3 away -- the roundings are where transformers puts them, not merely of the right size.  (The conditioned random weights
    give near-uniform attention, so THIS check does not see how the probabilities are rounded: test_storage_attention_core_rounds_like_the_fused_kernel does.)"""
    g, QM, P, px = mid["g"], mid["QM"], mid["P"], mid["px"]
    U = QM.unbits
    for k in g["vit_pins"]:
        xin, xout = U(g[f"pin_vit{k}_in"]), U(g[f"pin_vit{k}_out"])
        with torch.no_grad():
            tr = []
            Q.vit_forward(P, px, g["grid"], QM.oracle_cfg(), trace=tr, blocks=[int(k)], x_start=xin)
            with Q.storage(torch.bfloat16):
                tr16 = []
                Q.vit_forward(P, px, g["grid"], QM.oracle_cfg(), trace=tr16, blocks=[int(k)], x_start=xin)
        assert QM.rel(tr16[1], xout) < 4e-4, (int(k), QM.rel(tr16[1], xout))
        assert QM.rel(tr[1], xout) > 1.5e-3                                    # fp32 arithmetic is NOT what the bf16 run computes
    for k in g["llm_pins"]:
        xin, xout = U(g[f"pin_llm{k}_in"]), U(g[f"pin_llm{k}_out"])
        Pk, c1 = QM.layer_params(P, int(k)), QM.oracle_cfg(layers=1)
        with torch.no_grad():
            hs = []
            Q.llm_forward(Pk, xin[None], mid["pos"], mid["am"], c1, hidden_states=hs)
            with Q.storage(torch.bfloat16):
                hs16 = []
                Q.llm_forward(Pk, xin[None], mid["pos"], mid["am"], c1, hidden_states=hs16)
        assert QM.rel(hs16[1][0], xout) < 8e-4, (int(k), QM.rel(hs16[1][0], xout))
        assert QM.rel(hs[1][0], xout) > 1.5e-3


def test_bf16_storage_yardstick_equals_what_transformers_bf16_costs(mid):
    """End to end (20 blocks): the distance between the oracle's storage mode and its fp32 mode -- the YARDSTICK of the full-depth GPU test -- equals the distance
    between transformers' bf16 and fp32 runs at every recorded depth to 2 % (measured: 8.06 / 8.05e-3 at the ViT output, 5.64 / 5.63, 7.39 / 7.39, 11.05 / 10.98e-3
    along the decoder, 8.61 / 8.59e-3 on the logits), and the two bf16 runs themselves are 0.36 - 0.57 of a yardstick apart: same rounding points, and from the
    first flipped rounding on, later roundings of slightly different values decorrelate (independent noise of equal size would sit at 1.41)."""
    g, QM = mid["g"], mid["QM"]
    for k in POINTS:
        hf16, hf32 = QM.unbits(g[k + "_bf16"]), torch.from_numpy(g[k + "_fp32"])
        y_hf, y_or = QM.rel(hf16, hf32), QM.rel(mid["o16"][k], mid["o32"][k])
        assert abs(y_or / y_hf - 1.0) < 0.02, (k, y_or, y_hf)
        assert QM.rel(mid["o16"][k], hf16) < 0.7 * y_hf, (k, QM.rel(mid["o16"][k], hf16), y_hf)
    # the yardstick grows like a random walk over the decoder (sqrt of the depth), not linearly: what the GPU test's growth check relies on
    y4, y8, y12 = (QM.rel(mid["o16"][k], mid["o32"][k]) for k in ("hidden4", "hidden8", "hidden12"))
    assert y8 / y4 < (8 / 4) ** 0.5 * 1.1 and y4 < y8


def test_storage_attention_core_rounds_like_the_fused_kernel():
    """softmax(S) V inside a fused attention kernel (flash-attn 2 on the reference's GPUs, train_joint.py:181; torch's CPU flash kernel behind
    attn_implementation="sdpa"; this build's HIP kernels): the UN-normalised exponentials are rounded to bf16 for the second product, the row sums stay fp32, one
    rounding of the output.  On peaked scores the oracle's storage mode must sit on torch's bf16 kernel (measured 6 - 7e-4: the kernel's fast exponential flips
    a few roundings) and the normalise-then-round form (eager attention) must not (2.9e-3)."""
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(0)
    for L, causal in ((64, False), (304, True)):
        q, k, v = (torch.randn(1, 4, L, 64, generator=g).to(torch.bfloat16) for _ in range(3))
        q = q * 2
        ref = F.scaled_dot_product_attention(q, k, v, is_causal=causal).float()
        s = q.float() @ k.float().transpose(2, 3) * 64 ** -0.5
        if causal:
            s = s + torch.full((L, L), float("-inf")).triu(1)
        with Q.storage(torch.bfloat16):
            got = Q._softmax_pv(s, v.float())
            eager = Q._r(Q._r(torch.softmax(s, -1)) @ v.float())
        plain = Q._softmax_pv(s, v.float())
        r = lambda a, b: float((a - b).norm() / b.norm())
        assert r(got, ref) < 1.2e-3, r(got, ref)
        assert r(eager, ref) > 2e-3 and r(eager, ref) > 2.5 * r(got, ref)
        assert r(plain, ref) > 1.2e-3                                              # fp32 mode: no rounding at all


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# IMAGE inputs (pixel_values / image_grid_thw) and batches that mix images and videos, pinned to tests/golden/qwen_image.npz
# (tests/golden/make_qwen_image_fixtures.py: the installed transformers on the same tiny config and weights).  Same bounds as above.
from tests.qwen_image import VIT_KEYS as IMG_KEYS, batch_pixels as _img_pixels, gold_image, vit_pixels  # noqa: E402


@pytest.fixture(scope="module")
def gimg():
    return gold_image()


@pytest.mark.parametrize("key", IMG_KEYS)
def test_vision_index_plumbing_image_grids_bit_exact(gimg, key):
    g = gimg[f"{key}_grid"]
    wi, cw = Q.vision_window_index(g, 2, 112, 14)
    assert np.array_equal(wi, gimg[f"{key}_window_index"])
    assert np.array_equal(cw, gimg[f"{key}_cu_window"])
    assert np.array_equal(Q.vision_cu_seqlens(g), gimg[f"{key}_cu_full"])
    assert np.array_equal(Q.vision_position_ids(g, 2), gimg[f"{key}_pos_ids"])
    if key == "big":
        assert np.diff(gimg["big_cu_full"]).max() >= 1024            # the one full-attention segment is long enough for the split-KV route


@pytest.mark.parametrize("key", IMG_KEYS)
def test_vit_forward_image_grids(gimg, gold, key):
    cfg, P = tiny_cfg(), tiny_params(gold)
    g = gimg[f"{key}_grid"]
    px = vit_pixels(gimg, key)
    out, pre = Q.vit_forward(P, px, g, cfg, return_pre_merge=True)
    assert np.abs(out.numpy() - gimg[f"{key}_pooler"]).max() < 1e-4
    if f"{key}_last_hidden" in gimg.files:
        assert np.abs(pre.numpy() - gimg[f"{key}_last_hidden"]).max() < 1e-4


@pytest.mark.parametrize("rule", ["hf515", "hf449"])
def test_rope_index_image_and_video_bit_exact(gimg, rule):
    """row 0: text / image / text, right-padded; row 1: text / video / text / one-token image / text, left-padded.  The grids make both temporal rules agree."""
    pos, delta = Q.rope_index(gimg["rope_img_input_ids"], tiny_cfg(), gimg["rope_img_image_grid"], gimg["rope_img_video_grid"], gimg["rope_img_spg"],
                              gimg["rope_img_attention_mask"], temporal_rule=rule)
    assert np.array_equal(pos, gimg["rope_img_position_ids"])
    assert np.array_equal(delta, gimg["rope_img_deltas"])


def test_product_rope_index_image_and_video_bit_exact(gimg):
    """The product's host plumbing (rga3.model.qwen_index, what the GPU forward and generate() take their positions and deltas from) on the same batch."""
    from rga3.model import qwen_index as QI

    for rule in ("hf515", "hf449"):
        pos, delta = QI.rope_index(gimg["rope_img_input_ids"], 301, 302, 2, 2, gimg["rope_img_image_grid"], gimg["rope_img_video_grid"], gimg["rope_img_spg"],
                                   gimg["rope_img_attention_mask"], rule)
        assert np.array_equal(pos, gimg["rope_img_position_ids"]) and np.array_equal(delta, gimg["rope_img_deltas"]), rule
    for key in IMG_KEYS:
        g = gimg[f"{key}_grid"]
        wi, cw = QI.vision_window_index(g, 2, 112, 14)
        assert np.array_equal(wi, gimg[f"{key}_window_index"]) and np.array_equal(cw, gimg[f"{key}_cu_window"]), key
        assert np.array_equal(QI.vision_cu_seqlens(g), gimg[f"{key}_cu_full"]) and np.array_equal(QI.vision_position_ids(g, 2), gimg[f"{key}_pos_ids"]), key


def test_full_forward_and_loss_image_and_video(gimg, gold):
    """B = 2, padded: sample 0 image only (right-padded), sample 1 video then image (left-padded)."""
    cfg, P = tiny_cfg(), tiny_params(gold)
    px, pxv = _img_pixels(gimg, "mix")
    r = Q.forward(P, cfg, torch.from_numpy(gimg["mix_input_ids"]), torch.from_numpy(gimg["mix_attention_mask"]), labels=torch.from_numpy(gimg["mix_labels"]),
                  pixel_values=px, image_grid_thw=gimg["mix_image_grid"], pixel_values_videos=pxv, video_grid_thw=gimg["mix_video_grid"],
                  second_per_grid_ts=np.array([1.0]))
    assert np.array_equal(r["position_ids"].numpy(), gimg["mix_position_ids"])
    am = gimg["mix_attention_mask"].astype(bool)
    assert np.abs(r["hidden"].numpy() - gimg["mix_hidden_last"])[am].max() < 2e-4
    assert np.abs(r["logits"].numpy() - gimg["mix_logits"])[am].max() < 2e-4
    assert abs(float(r["loss"]) - float(gimg["mix_loss"])) < 1e-5


def test_greedy_generate_fixtures_follow_the_oracle(gimg, gold):
    """The greedy tokens HF produced for the image prompt and the left-padded image / video batch are the oracle's argmax over the teacher-forced sequence
    (full-sequence forward: the decode positions follow from the prefill's rope deltas), on every step where the oracle's top-1 / top-2 margin is decisive."""
    cfg, P = tiny_cfg(), tiny_params(gold)
    cases = [("gen_img", _img_pixels(gimg, "gen_img", ("image",))[0], None, np.ones_like(gimg["gen_img_input_ids"]))]
    px, pxv = _img_pixels(gimg, "gen_mix")
    cases.append(("gen_mix", px, pxv, gimg["gen_mix_attention_mask"]))
    for tag, px, pxv, am in cases:
        full = gimg[f"{tag}_output_ids"]
        S0 = gimg[f"{tag}_input_ids"].shape[1]
        am_full = np.concatenate([am, np.ones((am.shape[0], full.shape[1] - S0), dtype=am.dtype)], 1)
        r = Q.forward(P, cfg, torch.from_numpy(full), torch.from_numpy(am_full), pixel_values=px, image_grid_thw=gimg[f"{tag}_image_grid"],
                      pixel_values_videos=pxv, video_grid_thw=gimg[f"{tag}_video_grid"] if pxv is not None else None,
                      second_per_grid_ts=np.array([1.0]) if pxv is not None else None)
        lg = r["logits"][:, S0 - 1:-1]
        top2 = lg.topk(2, dim=-1).values
        decided = (top2[..., 0] - top2[..., 1]) > 0.05 * lg.abs().amax(-1)
        assert decided[:, 0].all(), tag
        assert torch.equal(lg.argmax(-1)[decided], torch.from_numpy(full[:, S0:])[decided]), tag


def test_unigr_oracle_vision_inputs_pass_through():
    """oracle.unigr hands images and videos to the Qwen forward when the batch holds them, and leaves either out when it does not."""
    from oracle import unigr as U

    assert U._vision({"pixel_values_videos": torch.ones(2, 3, dtype=torch.float64), "video_grid_thw": "v"}).keys() == {"pixel_values_videos", "video_grid_thw"}
    assert U._vision({"pixel_values": torch.ones(2, 3), "image_grid_thw": "i", "pixel_values_videos": None}).keys() == {"pixel_values", "image_grid_thw"}
    both = U._vision({"pixel_values": torch.ones(2, 3, dtype=torch.bfloat16), "image_grid_thw": "i", "pixel_values_videos": torch.ones(1, 3), "video_grid_thw": "v"})
    assert both["pixel_values"].dtype == torch.float32 and both["image_grid_thw"] == "i" and both["video_grid_thw"] == "v"
