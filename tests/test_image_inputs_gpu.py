"""GPU parity on IMAGE inputs (pixel_values / image_grid_thw) and on batches that mix images and videos: the vision tower on t = 1 grids through both
attention routes, the mixed forward, KV-cached decode and generate() after an image prompt, the training gradients, the joint model's image samples, the
prefetch slots and the bound on the tower's plan cache.  References: the fp32 oracle on the same bf16-rounded weights, and the transformers golden vectors
of tests/golden/qwen_image.npz (pinned to the oracle by tests/test_oracle_qwen.py).
Tolerances: rel-L2 <= 2e-2 on hidden states / logits, losses <= 1e-2 relative, mask IoU >= 0.99, integers and tokens exact."""
import numpy as np
import pytest
import torch

from oracle import qwen25vl as Q
from oracle import unigr as U
from tests.qwen_image import VIT_KEYS, batch_pixels, gold_image, vit_pixels
from tests.qwen_tiny import det_params, gold, oracle_cfg, product_cfg_kwargs, rel_l2

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module")
def gi():
    return gold_image()


@pytest.fixture(scope="module")
def P():
    return det_params(gold())


@pytest.fixture(scope="module")
def model(dev):
    from rga3.model.qwen2_5_vl import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    m = Qwen2_5_VLForConditionalGeneration(Qwen2_5_VLConfig(**product_cfg_kwargs()))
    m.load_state_dict(det_params(gold(), bf16_round=False), strict=True)
    return m.to(BF).to(dev).eval()


def mix_inputs(gi, dev):
    px, pxv = (t.to(BF) for t in batch_pixels(gi, "mix"))
    ids, am, labels = (torch.from_numpy(gi[k]) for k in ("mix_input_ids", "mix_attention_mask", "mix_labels"))
    kw = dict(input_ids=ids.to(dev), attention_mask=am.to(dev), labels=labels.to(dev), pixel_values=px.to(dev), image_grid_thw=torch.from_numpy(gi["mix_image_grid"]),
              pixel_values_videos=pxv.to(dev), video_grid_thw=torch.from_numpy(gi["mix_video_grid"]), second_per_grid_ts=torch.tensor([1.0]))
    ref_kw = dict(labels=labels, pixel_values=px.float(), image_grid_thw=gi["mix_image_grid"], pixel_values_videos=pxv.float(),
                  video_grid_thw=gi["mix_video_grid"], second_per_grid_ts=np.array([1.0]))
    return ids, am, kw, ref_kw


class _Count:
    """Wraps the ops attention entry points the vision blocks call and records which ran (and on how long a segment)."""

    def __init__(self):
        import rga3.model.qwen2_5_vl as QM

        self.QM, self.calls = QM, []

    def __enter__(self):
        ops = self.QM.ops
        self.real = (ops.attn_varlen_rope, ops.attn_varlen)
        r_rope, r_plain = self.real
        ops.attn_varlen_rope = lambda *a, **k: (self.calls.append(("rope", int(a[5]))), r_rope(*a, **k))[1]
        ops.attn_varlen = lambda *a, **k: (self.calls.append(("plain", int(a[5]))), r_plain(*a, **k))[1]
        return self

    def __exit__(self, *e):
        self.QM.ops.attn_varlen_rope, self.QM.ops.attn_varlen = self.real


def _decisive(lg):
    top2 = lg.topk(2, dim=-1).values
    return (top2[..., 0] - top2[..., 1]) > 0.05 * lg.abs().amax(-1)


# ------------------------------------------------------------------------------------------------ vision tower on image grids
@pytest.mark.parametrize("key", VIT_KEYS)
def test_vit_image_grids(model, dev, gi, P, key):
    """t = 1 grids: partial windows on both axes (img1), one merged token = a 4-patch window (img2), three images of different sizes = ragged window and
    full-attention segments (multi), one 1296-key full-attention segment = the split-KV route (big).  Both attention routes of the windowed blocks: under
    no_grad the kernel that rotates q / k while loading them, with grad enabled rope_ + attn_varlen."""
    g = gi[f"{key}_grid"]
    px = vit_pixels(gi, key).to(BF)
    ref = Q.vit_forward(P, px.float(), g, oracle_cfg())
    from rga3.hip import ops

    depth, full = len(model.visual.blocks), model.config.vision_config.fullatt_block_indexes
    pl = model.visual.plan(g, dev)
    # under no_grad every block whose longest segment fits the fused kernel takes it: the windowed ones always, a full-attention one when its image is small
    n_fused = (depth - len(full)) + (len(full) if ops.attn_rope_win_ok(pl["max_full"], 16) else 0)
    assert ops.attn_rope_win_ok(pl["max_win"], 16)
    for route in ("fused", "plain"):
        with _Count() as c, (torch.no_grad() if route == "fused" else torch.enable_grad()):
            out = model.visual(px.to(dev), g).detach()
        kinds = [k for k, _ in c.calls]
        if route == "fused":
            assert kinds.count("rope") == n_fused and kinds.count("plain") == depth - n_fused, c.calls
        else:
            assert kinds.count("plain") == depth and "rope" not in kinds, c.calls
        if key == "big":
            assert max(n for _, n in c.calls) >= 1024         # the long full-attention segment: attn_varlen's split-KV condition (max_k >= 1024)
        assert tuple(out.shape) == tuple(ref.shape)
        assert rel_l2(out, ref) < 2e-2, (route, rel_l2(out, ref))
        assert rel_l2(out, torch.from_numpy(gi[f"{key}_pooler"])) < 3e-2, route      # vs HF fp32 (weights unrounded)


def test_vit_multi_image_rows_in_order(model, dev, gi, P):
    """The three-image call against three one-image calls: each image's merged rows land in that image's place (a row permutation between or inside images,
    which a global rel-L2 could average away, is an O(1) error on that image's block)."""
    g = gi["multi_grid"]
    px = vit_pixels(gi, "multi").to(BF)
    with torch.no_grad():
        out = model.visual(px.to(dev), g).float().cpu()
        a = b = 0
        for t, h, w in g.tolist():
            n = t * h * w
            one = model.visual(px[a:a + n].to(dev), np.array([[t, h, w]])).float().cpu()
            blk = out[b:b + n // 4]
            assert blk.shape == one.shape
            assert rel_l2(blk, one) < 2e-2, (t, h, w, rel_l2(blk, one))
            ref = Q.vit_forward(P, px[a:a + n].float(), np.array([[t, h, w]]), oracle_cfg())
            assert rel_l2(blk, ref) < 2e-2
            # row by row: every row is closest to its own reference row
            d = torch.cdist(blk, ref)
            assert torch.equal(d.argmin(1), torch.arange(blk.shape[0])), (t, h, w)
            a, b = a + n, b + n // 4
        assert b == out.shape[0]


def test_vit_image_7b_dims_long_full_segment(dev):
    """7B vision dims (hidden 1280, 16 heads, D = 80), one windowed + one full-attention block, grid [1, 98, 74]: 7 252 patches, one full-attention segment of
    7 252 keys, windows cut by the grid edge on both axes."""
    from rga3.model.qwen2_5_vl import Qwen2_5_VLVisionConfig, VisionTransformer
    from tests.test_fullsize_parity_gpu import _init

    vc = Qwen2_5_VLVisionConfig(depth=2, fullatt_block_indexes=(1,))
    vt = _init(VisionTransformer(vc), 12)
    grid = np.array([[1, 98, 74]])
    px = torch.randn(98 * 74, 1176, generator=torch.Generator().manual_seed(4)).clamp_(-1.8, 2.2).to(BF)
    Pv = {"visual." + k: v.detach().to(BF).float() for k, v in vt.state_dict().items()}
    vtd = vt.to(BF).to(dev).eval()
    with torch.no_grad():
        y = vtd(px.to(dev), grid)
    pl = vtd.plan(grid, dev)
    assert pl["max_full"] == 7252 and pl["n"] == 7252
    ref = Q.vit_forward(Pv, px.float(), grid, Q.QwenCfg(vision=Q.VisionCfg(depth=2, fullatt_block_indexes=(1,)), text=Q.TextCfg(num_hidden_layers=1)))
    assert tuple(y.shape) == (49 * 37, 3584)
    assert rel_l2(y, ref) < 2e-2, rel_l2(y, ref)


# ------------------------------------------------------------------------------------------------ decoder on mixed batches
def test_forward_mixed_image_video_batch(model, dev, gi, P):
    """B = 2 padded: sample 0 image only (right-padded), sample 1 video then image (left-padded)."""
    ids, am, kw, ref_kw = mix_inputs(gi, dev)
    with torch.no_grad():
        out = model(**kw, output_hidden_states=True)
    pos_hf = gi["mix_position_ids"]
    m = am.bool()
    # positions and rope deltas: bit-exact with HF
    assert np.array_equal(model.__dict__["_last_plan"]["pos3"].cpu().numpy(), pos_hf[:, m.numpy()])
    want_delta = np.array([[pos_hf[:, b][:, m[b].numpy()].max() + 1 - int(m[b].sum())] for b in range(2)])
    assert np.array_equal(out.rope_deltas.cpu().numpy(), want_delta)
    ref = Q.forward(P, oracle_cfg(), ids, am, **ref_kw)
    assert np.array_equal(ref["position_ids"].numpy(), pos_hf)
    assert rel_l2(out.hidden_states[-1][m], ref["hidden"][m]) < 2e-2
    assert rel_l2(out.logits[m], ref["logits"][m]) < 2e-2
    assert abs(out.loss.item() - ref["loss"].item()) / ref["loss"].item() < 1e-2
    assert abs(out.loss.item() - float(gi["mix_loss"])) / float(gi["mix_loss"]) < 2e-2
    assert out.logits[~m].abs().sum().item() == 0 and out.hidden_states[-1][~m].abs().sum().item() == 0


def test_kv_cache_decode_image_prompt(model, dev, gi, P):
    """Prefill on the image prompt, then teacher-forced single-token decode steps through the KV cache (positions from the prefill's rope delta) against the
    oracle's full-sequence logits; the greedy token equals the oracle's on decisive steps and HF's on the first."""
    from rga3.model.qwen2_5_vl import KVCache

    full = torch.from_numpy(gi["gen_img_output_ids"])
    S0 = gi["gen_img_input_ids"].shape[1]
    px = batch_pixels(gi, "gen_img", ("image",))[0].to(BF)
    grid = torch.from_numpy(gi["gen_img_image_grid"])
    ref = Q.forward(P, oracle_cfg(), full, torch.ones_like(full), pixel_values=px.float(), image_grid_thw=grid.numpy())["logits"][0]
    c = model.config
    cache = KVCache(c.num_hidden_layers, 1, full.shape[1] + 1, c.num_key_value_heads, c.head_dim, dev, BF)
    with torch.no_grad():
        out = model(input_ids=full[:, :S0].to(dev), attention_mask=torch.ones(1, S0, dtype=torch.long, device=dev), past_key_values=cache,
                    pixel_values=px.to(dev), image_grid_thw=grid)
        assert int(out.rope_deltas.item()) != 0                  # the image compresses 35 tokens into 7 positions: decode positions depend on the delta
        rows = [out.logits[0, -1].float().cpu()]
        for t in range(S0, full.shape[1] - 1):
            out = model(input_ids=full[:, t:t + 1].to(dev), attention_mask=torch.ones(1, t + 1, dtype=torch.long, device=dev), past_key_values=cache)
            rows.append(out.logits[0, -1].float().cpu())
    got, want = torch.stack(rows), ref[S0 - 1: full.shape[1] - 1]
    assert rel_l2(got, want) < 2e-2
    decided = _decisive(want)
    assert torch.equal(got.argmax(-1)[decided], want.argmax(-1)[decided])
    assert decided[0] and int(got[0].argmax()) == int(full[0, S0])


def _check_against_hf(seq, hf, ref_logits, S0):
    """Generated tokens vs HF's greedy tokens, row by row, up to the first step where the oracle's margin is not decisive (after a near-tie the two greedy
    paths may part legitimately)."""
    dec = _decisive(ref_logits)
    for b in range(hf.shape[0]):
        n = int(dec[b].long().cumprod(0).sum())
        assert n >= 1, b
        assert torch.equal(seq[b, S0:S0 + n].cpu(), torch.from_numpy(hf[b, S0:S0 + n])), (b, seq[b, S0:].tolist(), hf[b, S0:].tolist())


def test_generate_image_prompt_graph_equals_eager(model, dev, gi, P):
    """B = 1 generate() after an image prompt: the captured decode graph (positions advanced on the device from the prefill's rope delta) against the eager loop,
    token for token, and its first tokens against HF's greedy run."""
    ids = torch.from_numpy(gi["gen_img_input_ids"])
    S0 = ids.shape[1]
    px = batch_pixels(gi, "gen_img", ("image",))[0].to(BF)
    grid = torch.from_numpy(gi["gen_img_image_grid"])
    kw = dict(input_ids=ids.to(dev), attention_mask=torch.ones_like(ids).to(dev), pixel_values=px.to(dev), image_grid_thw=grid, max_new_tokens=20,
              do_sample=False, eos_token_id=-1)
    with torch.no_grad():
        a = model.generate(**kw, decode_graph=False)
        b = model.generate(**kw)
    assert any("graph" in st for st in model.__dict__.get("_decode_states", {}).values())        # the captured route ran
    assert a.shape == (1, S0 + 20) and torch.equal(a, b)
    hf = gi["gen_img_output_ids"]
    ref = Q.forward(P, oracle_cfg(), torch.from_numpy(hf), torch.ones(hf.shape, dtype=torch.long), pixel_values=px.float(), image_grid_thw=grid.numpy())["logits"]
    _check_against_hf(a, hf, ref[:, S0 - 1:-1], S0)


def test_generate_mixed_batch_left_padded(model, dev, gi, P):
    """B = 2 left-padded: an image prompt and a video prompt, HF's greedy tokens on decisive steps."""
    ids, am = torch.from_numpy(gi["gen_mix_input_ids"]), torch.from_numpy(gi["gen_mix_attention_mask"])
    S0 = ids.shape[1]
    px, pxv = (t.to(BF) for t in batch_pixels(gi, "gen_mix"))
    ig, vg = torch.from_numpy(gi["gen_mix_image_grid"]), torch.from_numpy(gi["gen_mix_video_grid"])
    with torch.no_grad():
        seq = model.generate(input_ids=ids.to(dev), attention_mask=am.to(dev), pixel_values=px.to(dev), image_grid_thw=ig, pixel_values_videos=pxv.to(dev),
                             video_grid_thw=vg, second_per_grid_ts=torch.tensor([1.0]), max_new_tokens=6, do_sample=False, eos_token_id=-1)
    hf = gi["gen_mix_output_ids"]
    assert seq.shape == hf.shape and torch.equal(seq[:, :S0].cpu(), ids)
    am_full = torch.cat([am, torch.ones(2, hf.shape[1] - S0, dtype=am.dtype)], 1)
    ref = Q.forward(P, oracle_cfg(), torch.from_numpy(hf), am_full, pixel_values=px.float(), image_grid_thw=ig.numpy(), pixel_values_videos=pxv.float(),
                    video_grid_thw=vg.numpy(), second_per_grid_ts=np.array([1.0]))["logits"]
    _check_against_hf(seq, hf, ref[:, S0 - 1:-1], S0)
    # greedy margins of a tiny random model decide only a few steps: the decode positions of the padded rows (valid length + the prefill's rope delta) are
    # pinned by the logits instead -- prefill, then HF's tokens teacher-forced one step at a time through the KV cache, against the oracle's full sequence
    from rga3.model.qwen2_5_vl import KVCache

    _, want_delta = Q.rope_index(ids.numpy(), oracle_cfg(), ig.numpy(), vg.numpy(), np.array([1.0]), am.numpy())
    full = torch.from_numpy(hf)
    c = model.config
    cache = KVCache(c.num_hidden_layers, 2, full.shape[1] + 1, c.num_key_value_heads, c.head_dim, dev, BF)
    with torch.no_grad():
        out = model(input_ids=ids.to(dev), attention_mask=am.to(dev), past_key_values=cache, pixel_values=px.to(dev), image_grid_thw=ig,
                    pixel_values_videos=pxv.to(dev), video_grid_thw=vg, second_per_grid_ts=torch.tensor([1.0]))
        assert np.array_equal(out.rope_deltas.cpu().numpy(), want_delta)
        rows = [out.logits[:, -1].float().cpu()]
        for t in range(S0, full.shape[1] - 1):
            out = model(input_ids=full[:, t:t + 1].to(dev), attention_mask=am_full[:, :t + 1].to(dev), past_key_values=cache)
            rows.append(out.logits[:, -1].float().cpu())
    got = torch.stack(rows, 1)
    assert rel_l2(got, ref[:, S0 - 1:-1]) < 2e-2, rel_l2(got, ref[:, S0 - 1:-1])


# ------------------------------------------------------------------------------------------------ training
def test_training_gradients_image_tokens(dev, gi):
    """test_llm_training_step_gradients (LoRA + lm_head + embed_tokens trainable) on the mixed image / video batch, same bounds; the embedding rows of the image
    and video placeholder ids get no gradient at all (their rows are overwritten by vision features: HF's masked_scatter discards theirs)."""
    from tests.test_train_gpu import _build_lora_model

    G = gold()
    model, lora = _build_lora_model(dev, G)
    ids, am, kw, ref_kw = mix_inputs(gi, dev)
    out = model(**kw, output_hidden_states=True)
    out.loss.backward()
    P = det_params(G)
    P.update({k: v.to(BF).float() for k, v in lora.items()})
    P["lora_scaling"] = 2.0
    train_keys = [k for k in P if isinstance(P[k], torch.Tensor) and ("lora_" in k or k in ("lm_head.weight", "model.embed_tokens.weight"))]
    for k in train_keys:
        P[k].requires_grad_(True)
    ref = Q.forward(P, oracle_cfg(), ids, am, **ref_kw)
    ref["loss"].backward()
    assert abs(out.loss.item() - ref["loss"].item()) / ref["loss"].item() < 1e-2
    got = {n: p.grad for n, p in model.named_parameters() if p.requires_grad}
    assert all(g is not None for g in got.values())
    errs = {k: rel_l2(got[k], P[k].grad) for k in train_keys}
    bad = {k: e for k, e in errs.items() if e >= (3e-2 if k == "lm_head.weight" else 6e-2)}
    assert not bad, (bad, errs)
    m = am.bool()
    assert rel_l2(out.hidden_states[-1][m], ref["hidden"][m].detach()) < 3e-2
    ge = got["model.embed_tokens.weight"]
    c = model.config
    for tok in (c.image_token_id, c.video_token_id):
        assert int((ids == tok).sum()) > 0
        assert torch.count_nonzero(ge[tok]).item() == 0, tok
        assert torch.count_nonzero(P["model.embed_tokens.weight"].grad[tok]).item() == 0
    assert torch.count_nonzero(ge[c.vision_start_token_id]).item() > 0        # a text row of the same batch does get its gradient
    # the data-parallel route: a GradBucketReducer holds the table as a sparse parameter, EmbedFn hands it (unique row ids, summed rows) instead of a dense
    # gradient.  Same rows, same values as the dense route; the placeholder ids are not among the announced rows at all.
    from rga3.parallel.ddp import GradBucketReducer

    model2, _ = _build_lora_model(dev, G)
    emb = model2.model.embed_tokens.weight
    train = [p for p in model2.parameters() if p.requires_grad]
    red = GradBucketReducer(train, bucket_mb=0.25, sparse_params=[emb])
    try:
        red.begin_step()
        red.begin_micro_step()
        out2 = model2(**kw)
        out2.loss.backward()
        red.finish()
        assert emb.grad is None
        gs = red.grad_view(emb)
        union = red._sp[id(emb)]["union"]
        assert c.image_token_id not in union and c.video_token_id not in union and c.vision_start_token_id in union
        assert torch.count_nonzero(gs[c.image_token_id]).item() == 0 and torch.count_nonzero(gs[c.video_token_id]).item() == 0
        assert torch.equal(gs != 0, ge != 0)
        assert rel_l2(gs, ge) < 1e-2                              # one micro-step: the same segment sums, added into a zeroed buffer
        assert rel_l2(gs, P["model.embed_tokens.weight"].grad) < 6e-2
    finally:
        red.remove()


# ------------------------------------------------------------------------------------------------ joint model: image samples
@pytest.fixture(scope="module")
def G():
    from tests.unigr_tiny import gold as ugold

    return ugold()


@pytest.fixture(scope="module")
def joint(dev, G):
    from rga3.model.qwen_2_5_vl_sam2 import UniGRConfig, UniGRModel
    from tests.unigr_tiny import SAM_TINY, SEG, params

    cfg = UniGRConfig(train_mask_decoder=True, out_dim=256, ce_loss_weight=1.0, dice_loss_weight=0.5, bce_loss_weight=2.0, seg_token_idx=SEG,
                      sam_pretrained=None, sam_config=SAM_TINY, **product_cfg_kwargs())
    m = UniGRModel(cfg)
    m.initialize_sam_modules(cfg)
    Pq, PS = params(G)
    sd = dict(Pq)
    sd.update({"grounding_encoder.sam2_model." + k: v for k, v in PS.items()})
    m.load_state_dict(sd, strict=True)
    return m.to(BF).to(dev).eval()


def _to_dev(b, dev):
    out = {}
    for k, v in b.items():
        if isinstance(v, torch.Tensor):
            out[k] = v.to(dev).to(BF) if v.is_floating_point() and k in ("pixel_values", "pixel_values_videos", "images_sam") else v.to(dev)
        elif isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            out[k] = [t.to(dev) for t in v]
        else:
            out[k] = v
    return out


def _iou(a, b):
    a, b = a.cpu().bool(), b.cpu().bool()
    u = (a | b).sum().item()
    return 1.0 if u == 0 else (a & b).sum().item() / u


@pytest.mark.parametrize("video_seg", [True, False])
def test_unigr_model_forward_image_sample(joint, dev, G, video_seg):
    """model_forward on B = 2: an image sample with [SEG] (its one SAM frame repeated T_SAM times) and a video sample with or without [SEG], against the oracle's
    model_forward with the same pixel inputs.

    loss and ce_loss: the test_model_forward_loss_dict bound.  The mask losses are pinned where their error arises, at the logits: for every sample with [SEG]
    the product's [SEG] embedding and its high-resolution mask logits on the training path (SAM2 image encoder -> inject_language_embd_train) against the oracle's
    (oracle.sam2 on the same frames, with the oracle's embedding) at rel-L2 <= 2e-2, and the product's mask_bce / mask_dice / mask_loss equal to the oracle's loss
    functions evaluated on those product logits (1e-4 relative).  Why not the loss bound itself: a confidently segmented object (|logit| ~ 7 over most of the
    frame) makes the BCE an exponential of the margin -- d softplus(-z)/dz = -sigmoid(-z), and sigmoid(-z) <= softplus(-z), so the RELATIVE change of the BCE is
    up to the ABSOLUTE change of the logits.  bf16 logits of that size carry absolute errors of ~0.04 (measured: rel-L2 5.8e-3 of the high-res logits, as for
    the video samples, 4.6 - 5.6e-3), hence 2 - 6 % on the mask losses of these samples, whose losses (bce 0.05 - 0.11) are large enough that the 2e-3 floor
    of that bound no longer absorbs it (the video samples of test_model_forward_loss_dict sit at 0.01 - 0.02)."""
    from tests.unigr_tiny import SEG, make_image_video_batch, params, sam_cfg
    import torch.nn.functional as F
    from oracle import sam2 as S
    from rga3.hip import ops

    b = make_image_video_batch(video_seg, seed=21 + int(video_seg))
    Pq, PS = params(G, bf16_round=True)
    d = _to_dev(b, dev)
    with torch.no_grad():
        ref = U.model_forward(Pq, PS, oracle_cfg(), sam_cfg(), b, (1.0, 0.5, 2.0), SEG)
        out = joint(**d, inference=False)
        # the product's internals of the same forward, recomputed: [SEG] embeddings from its hidden states, then its SAM2 training path per sample
        lm = joint(input_ids=d["input_ids"], attention_mask=d["attention_mask"], past_key_values=None, pixel_values=d["pixel_values"],
                   image_grid_thw=d["image_grid_thw"], pixel_values_videos=d["pixel_values_videos"], video_grid_thw=d["video_grid_thw"],
                   second_per_grid_ts=d["second_per_grid_ts"], output_hidden_states=True)
        e_p, counts = joint._seg_embeddings(lm.hidden_states[-1], joint._shifted_seg_mask(b["labels"].numpy(), SEG))
    assert set(out) == {"loss", "ce_loss", "mask_bce_loss", "mask_dice_loss", "mask_loss"}
    assert int(ref["seg_token_offset"][-1]) == 1 + int(video_seg) and counts.tolist() == [1, int(video_seg)]
    for k in ("loss", "ce_loss"):
        r = float(ref[k])
        assert abs(float(out[k]) - r) <= 1e-2 * abs(r) + 2e-3, (k, float(out[k]), r)
    e_o = ref["pred_embeddings"]
    assert rel_l2(e_p, e_o) < 2e-2
    gm, T = joint.grounding_encoder, b["images_sam"].shape[1]
    bce = dice = 0.0
    for i in range(2):
        if counts[i] == 0:
            continue
        with torch.no_grad():
            st = gm.get_sam2_embeddings_train(d["images_sam"][i])
            _, high_p = gm.inject_language_embd_train(st, e_p[i:i + 1][None].expand(T, -1, -1))
            hw = tuple(b["label_list"][i].shape)
            pred_p = ops.bilinear(high_p[:, 0].contiguous(), hw).float().cpu()
            feats = S.prepare_backbone_features(S.image_encoder_forward(PS, b["images_sam"][i].float(), sam_cfg()))
            _, high_o, _ = S.inject_language_embd_train(PS, feats, e_o[i:i + 1][None].expand(T, -1, -1), sam_cfg())
        assert rel_l2(high_p[:, 0], high_o[:, 0]) < 2e-2, (i, rel_l2(high_p[:, 0], high_o[:, 0]))
        gt = b["masks_list"][i]
        bce += float(U.sigmoid_ce_loss(pred_p, gt, gt.shape[0])) * gt.shape[0]
        dice += float(U.dice_loss(pred_p, gt, gt.shape[0])) * gt.shape[0]
    n = sum(m.shape[0] for m in b["masks_list"])
    want = {"mask_bce_loss": 2.0 * bce / n, "mask_dice_loss": 0.5 * dice / n}
    want["mask_loss"] = want["mask_bce_loss"] + want["mask_dice_loss"]
    for k, w in want.items():
        assert abs(float(out[k]) - w) <= 1e-4 * abs(w), (k, float(out[k]), w)


def test_unigr_evaluate_image(joint, dev, G):
    """evaluate() on an image sample (pixel_values / image_grid_thw, no video), its frame repeated T_SAM times: bool masks bit-exact with the oracle outside the
    band at the object's edge, IoU >= 0.99."""
    from tests.unigr_tiny import LABEL_HW, SEG, make_image_video_batch, params, sam_cfg

    full = make_image_video_batch(True, seed=23)
    n = int(full["attention_mask"][0].sum())
    b = dict(input_ids=full["input_ids"][:1, :n], attention_mask=full["attention_mask"][:1, :n], pixel_values=full["pixel_values"],
             image_grid_thw=full["image_grid_thw"], images_sam=full["images_sam"][:1], resize_list=full["resize_list"][:1])
    Pq, PS = params(G, bf16_round=True)
    d = _to_dev(b, dev)
    with torch.no_grad():
        _, rmasks, _, rlogits = U.evaluate(Pq, PS, oracle_cfg(), sam_cfg(), b, SEG, [LABEL_HW])
        _, masks = joint.evaluate(d["input_ids"], d["attention_mask"], d["pixel_values"], None, d["image_grid_thw"], None, None, d["images_sam"],
                                  d["resize_list"], [LABEL_HW])
    assert len(masks) == len(rmasks) == 1 and masks[0].dtype == torch.bool and masks[0].shape == rmasks[0].shape
    margin = rlogits[0].abs() > 0.05 * rlogits[0].abs().max()
    assert margin.float().mean() > 0.97
    assert torch.equal(masks[0].cpu()[margin], rmasks[0][margin])
    assert _iou(masks[0], rmasks[0]) >= 0.99


# ------------------------------------------------------------------------------------------------ vision prefetch and plan cache
def test_vision_prefetch_image_and_video_slots(model, dev, gi):
    """prefetch_vision with images AND videos caches one entry per slot; the next forward consumes both, bit-identical to a forward without prefetch.  Pixels
    prefetched in the image slot are never served to the video slot, even for the same tensor and grid."""
    _, _, kw, _ = mix_inputs(gi, dev)
    kw.pop("labels")
    vis = list(model.visual.parameters())
    flags = [p.requires_grad for p in vis]
    for p in vis:
        p.requires_grad_(False)
    try:
        with torch.no_grad():
            ref = model(**kw).logits.clone()
            model.prefetch_vision(**kw)
            cache = model.__dict__["_pf_cache"]
            assert sorted(k[0] for k in cache) == ["image", "video"]
            out = model(**kw).logits
            assert len(cache) == 0                                   # both consumed
            assert torch.equal(ref, out)
            # the video pixels (with the video grid) announced in the IMAGE slot: the video slot of the forward must miss and compute its own features
            model.prefetch_vision(pixel_values=kw["pixel_values_videos"], image_grid_thw=kw["video_grid_thw"])
            key = ("image", kw["pixel_values_videos"].data_ptr())
            assert list(cache) == [key]
            out = model(**kw).logits
            assert list(cache) == [key]                              # still there: nobody took it
            assert torch.equal(ref, out)
            cache.clear()
    finally:
        for p, f in zip(vis, flags):
            p.requires_grad_(f)


def test_vision_plan_cache_is_bounded(model, dev):
    """A run over images of many sizes: the tower's per-grid plan cache stays within its stated bound (least recently used out), and a grid that was evicted
    and comes back gives bit-identical features."""
    vt = model.visual
    cap = type(vt).PLAN_CACHE_SIZE
    assert 8 <= cap <= 64
    grids = [np.array([[1, 2 * h, 2 * w]]) for h in range(1, 17) for w in range(1, 17)]     # 256 distinct image grids
    first = grids[0]
    px0 = torch.randn(int(np.prod(first)), 1176, generator=torch.Generator().manual_seed(3)).to(BF).to(dev)
    with torch.no_grad():
        y0 = vt(px0, first).clone()
        for g in grids:
            vt(torch.randn(int(np.prod(g)), 1176, generator=torch.Generator().manual_seed(1)).to(BF).to(dev), g)
            assert len(vt._plans) <= cap
        assert len(vt._plans) == cap
        assert all(k[0] != tuple(map(tuple, first.tolist())) for k in vt._plans)   # evicted
        y1 = vt(px0, first)
    assert torch.equal(y0, y1)
