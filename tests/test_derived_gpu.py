"""Operands derived from weights (rga3.hip.derived) on the tiny models: every source tensor of every pack is in its key.

Stale-cache cases: run the smallest forward that reaches the site, update ONE source in place, run again -- the result must be bit-identical to a fresh instance
loaded with the updated state dict (so the pack was rebuilt) and differ from the first result (so the source is read at all).  One source at a time: an
all-at-once update hides a source that is missing from a key.  All under no_grad with more than 16 token rows: the norm-folded routes run.

Outputs compare with torch.equal because no timing decision enters: the shapes are the smallest the tiny fixtures allow, but ops.gemm tunes its RMSNorm-folded
form at any size and the memory encoder's fuser MLP of the tiny SAM2 (64 x 1024 x 256) sits exactly at ops._TUNE_WORK, so every test runs under
tuner.force(-1): the library's own tiling for every product."""
import pytest
import torch

from tests import qwen_tiny, sam2_tiny
from tests.test_sam2_gpu import TINY

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_tuner():
    from rga3.hip import tuner

    with tuner.force(-1):
        yield


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _stale(model, src, forward, fresh):
    with torch.no_grad():
        first = forward(model)
        keep = src.detach().clone()
        try:
            src.mul_(1.5)
            second = forward(model)
            want = forward(fresh(model))
        finally:
            src.copy_(keep)
    assert _same(second, want), "a pack built from the old value of this source was used"
    assert not _same(second, first), "the forward does not read this source"


def _entries(model):
    return {(n, k): e[1] for n, mod in model.named_modules() for k, e in mod.__dict__.get("_wt_cache", {}).items()}


def _no_rebuild(model, forward):
    with torch.no_grad():
        forward(model)
        one = _entries(model)
        forward(model)
        two = _entries(model)
    assert one and one.keys() == two.keys()
    assert all(two[k] is v for k, v in one.items()), [k for k, v in one.items() if two[k] is not v]
    return {k for _, k in one}


# ------------------------------------------------------------------------------------------------ Qwen2.5-VL
def _make_qwen(dev, sd):
    from rga3.model.qwen2_5_vl import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    m = Qwen2_5_VLForConditionalGeneration(Qwen2_5_VLConfig(**qwen_tiny.product_cfg_kwargs()))
    m.load_state_dict(sd, strict=True)
    return m.to(torch.bfloat16).to(dev).eval()


@pytest.fixture(scope="module")
def qwen(dev):
    return _make_qwen(dev, qwen_tiny.det_params(qwen_tiny.gold(), bf16_round=False))


@pytest.fixture(scope="module")
def qwen_forward(dev):
    from oracle.detweights import det_tensor

    g = qwen_tiny.gold()
    # the first sample of the fixture batch alone (one clip: the patch embedding is 192 x 64 x 1216)
    px = det_tensor("pixel_values_full0", (192, 1176), 1.0, seed=5).to(torch.bfloat16).to(dev)
    ids, am = torch.from_numpy(g["full_input_ids"][:1]).to(dev), torch.from_numpy(g["full_attention_mask"][:1]).to(dev)
    grid = torch.from_numpy(g["full_grid"][:1])
    assert int(am.sum()) >= 17 and px.shape[0] >= 17          # the folded routes need more than 16 rows

    def forward(m):
        return (m(input_ids=ids, attention_mask=am, pixel_values_videos=px, video_grid_thw=grid, second_per_grid_ts=torch.tensor([1.0])).logits,)
    return forward


# block / layer 1: the first one of a tower normalises its input itself, from the second on the norm is folded into q|k|v
QWEN_SOURCES = {
    "GatedMLP.gate_proj.weight": lambda m: m.visual.blocks[1].mlp.gate_proj.weight,
    "GatedMLP.up_proj.weight": lambda m: m.visual.blocks[1].mlp.up_proj.weight,
    "GatedMLP.down_proj.weight": lambda m: m.visual.blocks[1].mlp.down_proj.weight,
    "GatedMLP.gate_proj.bias": lambda m: m.visual.blocks[1].mlp.gate_proj.bias,
    "GatedMLP.fold.norm": lambda m: m.model.layers[1].post_attention_layernorm.weight,
    "Attention.fold.norm": lambda m: m.model.layers[1].input_layernorm.weight,
    "Attention.q_proj.weight": lambda m: m.model.layers[1].self_attn.q_proj.weight,
    "Attention.k_proj.weight": lambda m: m.model.layers[1].self_attn.k_proj.weight,
    "Attention.v_proj.weight": lambda m: m.model.layers[1].self_attn.v_proj.weight,
    "Attention.q_proj.bias": lambda m: m.model.layers[1].self_attn.q_proj.bias,
    "Attention.k_proj.bias": lambda m: m.model.layers[1].self_attn.k_proj.bias,
    "Attention.v_proj.bias": lambda m: m.model.layers[1].self_attn.v_proj.bias,
    "VisionPatchEmbed.proj.weight": lambda m: m.visual.patch_embed.proj.weight,
    "VisionAttention.qkv.weight": lambda m: m.visual.blocks[1].attn.qkv.weight,
    "VisionAttention.norm1.weight": lambda m: m.visual.blocks[1].norm1.weight,
}


@pytest.mark.parametrize("site", list(QWEN_SOURCES))
def test_qwen_pack_follows_its_source(qwen, qwen_forward, dev, site):
    _stale(qwen, QWEN_SOURCES[site](qwen), qwen_forward, lambda m: _make_qwen(dev, m.state_dict()))


def test_qwen_steady_state_rebuilds_nothing(qwen, qwen_forward):
    names = _no_rebuild(qwen, qwen_forward)
    assert {"pack", "pack:fold", "wqkv:fold"} <= names, names


# ------------------------------------------------------------------------------------------------ SAM2
def _make_sam2(dev, sd):
    from rga3.model.sam2 import SAM2

    m = SAM2(**TINY)
    m.sam2_model.load_state_dict(sd, strict=True)
    return m.to(torch.bfloat16).to(dev).eval()


@pytest.fixture(scope="module")
def sam2(dev):
    return _make_sam2(dev, sam2_tiny.det_params(sam2_tiny.gold()))


def _fresh_sam2(dev):
    return lambda m: _make_sam2(dev, m.sam2_model.state_dict())


@pytest.fixture(scope="module")
def encode(dev):
    """Hiera trunk + neck of one frame."""
    img = sam2_tiny.images(1).to(torch.bfloat16).to(dev)

    def forward(m):
        f = m.sam2_model.forward_image(img)
        return f["feat"], f["feat_s1"], f["feat_s0"]
    return forward


@pytest.fixture(scope="module")
def track(dev):
    """Frame 0 prompted, frames 1 and 2 tracked: memory encoder, memory attention and the mask decoder on its constant tokens; frames encoded one at a time."""
    img, emb = sam2_tiny.images(3).to(torch.bfloat16).to(dev), sam2_tiny.lang(3).to(torch.bfloat16).to(dev)

    def forward(m):
        from rga3.model.sam2 import VideoSession

        sess = VideoSession(m.sam2_model, img, chunk=1)
        sess.add_language_embd(0, emb[0][None])
        res = sess.propagate()
        assert sess.counts["memattn"] == 2
        return tuple(mk for _, mk in res)
    return forward


SAM2_ENCODE_SOURCES = {
    "Hiera.norm1.weight": lambda s: s.image_encoder.trunk.blocks[1].norm1.weight,
    "Hiera.norm1.bias": lambda s: s.image_encoder.trunk.blocks[1].norm1.bias,
    "Hiera.qkv.bias": lambda s: s.image_encoder.trunk.blocks[1].attn.qkv.bias,
    "Hiera.fc1.weight": lambda s: s.image_encoder.trunk.blocks[1].mlp.layers[0].weight,
    "pos_embed": lambda s: s.image_encoder.trunk.pos_embed,
    "pos_embed_window": lambda s: s.image_encoder.trunk.pos_embed_window,      # not in the key before rga3.hip.derived: the update went unseen
}
SAM2_TRACK_SOURCES = {
    "ConvT.as_linear": lambda s: s.sam_mask_decoder.output_upscaling[0].weight,
    "mask_tokens.weight": lambda s: s.sam_mask_decoder.mask_tokens.weight,
    "memory_attention.v_proj.bias": lambda s: s.memory_attention.layers[0].cross_attn_image.v_proj.bias,
    "conv3x3s2.wide": lambda s: s.memory_encoder.mask_downsampler.encoder[6].weight,
}


@pytest.mark.parametrize("site", list(SAM2_ENCODE_SOURCES))
def test_sam2_encoder_pack_follows_its_source(sam2, encode, dev, site):
    _stale(sam2, SAM2_ENCODE_SOURCES[site](sam2.sam2_model), encode, _fresh_sam2(dev))


@pytest.mark.parametrize("site", list(SAM2_TRACK_SOURCES))
def test_sam2_tracking_pack_follows_its_source(sam2, track, dev, site):
    src = SAM2_TRACK_SOURCES[site](sam2.sam2_model)
    if site == "conv3x3s2.wide":
        assert src.shape[1] >= 16 and src.shape[1] % 8 == 0       # the im2col + GEMM stage, the one with a pack
    _stale(sam2, src, track, _fresh_sam2(dev))


def test_sam2_steady_state_rebuilds_nothing(sam2, encode, track):
    names = _no_rebuild(sam2, lambda m: encode(m) + track(m))
    assert {"fold:qkv", "fold:proj", "fold:fc1", "pos_tokens", "as_linear", "tokens", "packs"} <= names, names


# ------------------------------------------------------------------------------------------------ sites the tiny models do not reach
def test_hiera_mlp288_pack_follows_w2(dev):
    """ops.hiera_mlp at C = 288 streams packed chunk images of (wf, colc, biasf, w2); 70 rows leave a partial last workgroup."""
    from rga3.hip import ops

    C, M = 288, 70
    g = torch.Generator().manual_seed(288)
    r = lambda *shape, s=1.0: (torch.randn(*shape, generator=g) * s).to(torch.bfloat16).to(dev)
    x, w1, b1, w2, b2 = r(M, C, s=1.5), r(4 * C, C, s=0.06), r(4 * C, s=0.1), r(C, 4 * C, s=0.035), r(C, s=0.1)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(torch.bfloat16).to(dev), r(C, s=0.1)
    wf, colc, biasf = ops.fold_layernorm(w1, b1, gamma, beta)
    first = ops.hiera_mlp(x, wf, colc, biasf, w2, b2, 1e-6)
    assert torch.equal(first, ops.hiera_mlp(x, wf, colc, biasf, w2, b2, 1e-6))
    w2.mul_(1.5)
    second = ops.hiera_mlp(x, wf, colc, biasf, w2, b2, 1e-6)
    want = ops.hiera_mlp(x, wf.clone(), colc.clone(), biasf.clone(), w2.clone(), b2, 1e-6)     # other addresses: a pack of its own
    assert torch.equal(second, want) and not torch.equal(second, first)


def test_neg_table_follows_sin(dev):
    from rga3.model.qwen_train import _neg_table

    sin = torch.linspace(-1, 1, 40 * 16, device=dev).view(40, 16).sin()
    first = _neg_table(sin)
    assert _neg_table(sin) is first and torch.equal(first, -sin)
    sin.mul_(1.5)
    second = _neg_table(sin)
    assert torch.equal(second, (-sin.clone()).contiguous()) and not torch.equal(second, first)
    assert _neg_table(sin) is second
