#!/usr/bin/env python3
"""bench.py — RGA3 hot path on MI355X.

Default workload (`--mode headline`, the BASELINE.json metric "video-QA samples/sec (fwd+bwd) at 7B/16-frame"):
BASELINE.json configs[2] per GPU — the complete RGA3 training micro-step of reference train_joint.py:521-535 on one
synthetic sample per GPU: Qwen2.5-VL-7B ViT (frozen) + decoder forward/backward with LoRA r128 on q/v, lm_head and
embed_tokens trainable, SAM2-L on 16 frames 1024x1024 (frozen Hiera-L + FPN, trainable mask decoder + text_hidden_fcs,
BCE + dice), bucketed gradient exchange, AdamW.  A "step" is one such micro-step + optimizer step; `value` = samples/s
over all ranks.  The same process first times BASELINE.json configs[1] (ViT + LLM forward, S = 2112) on the same weights
(its in-situ tile refinement sets the tilings the training step then runs).

A plain run does only what `value` needs: it sets up, warms up, times the steps, writes --dump-outputs and prints the line,
whose `roofline` is then the whole-step algorithmic FLOPs / step time.  `--full` adds everything else, each part outside the
timed steps: the configs[1] `roofline` object (dominant kernel family = the bf16 MFMA GEMM, HIP events on the launch stream
around every GEMM launch; `whole_forward_frac` is the >= 40 % target of the north star) with its A/B variants, board sample
and output check against the tile-10 kernel; `roofline_fwd_bwd.gemm_family`, the same measurement for the training step;
the step variants; the exchange report of a multi-GPU run; and `cpu_baseline`, the fp32 oracle restatement (a "port": the
reference is Python and cannot travel) on the host cores on a bounded sample of the same workload.

`--gpus N` with N > 1 and no torchrun environment: this process launches N ranks of itself (one per GPU, RCCL) BEFORE
touching the GPU and exits with their code; with fewer than N visible GPUs it exits non-zero.  Under the driver's
`python -m torch.distributed.run ... bench.py --gpus N` the ranks read RANK / LOCAL_RANK / WORLD_SIZE as usual.
Only `tests/`, `smoke()` and this file's cpu_baseline leg import `oracle/`.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "rga3-release_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

# algorithmic FLOPs per sample, SURVEY.md 8(d) / BASELINE.md 3
GEMM_FLOPS = (10.33 + 0.0247 + 0.182 + 27.6 + 2.30) * 1e12   # ViT linear + patch + merger + LLM linear + lm_head
ATTN_FLOPS = (0.247 + 0.90) * 1e12
TOTAL_FLOPS = GEMM_FLOPS + ATTN_FLOPS                          # 41.6 T: configs[1] forward
PEAK_BF16 = 2.5e15                                             # dense MFMA peak, MI355X_MICROARCH.md
PEAK_HBM = 8.0e12


def train_flops(sam_frames):
    """Algorithmic FLOPs of one full RGA3 training sample as THIS build runs it: ViT fwd (frozen) + LLM fwd with the LM head on
    labelled rows only + LLM dX (activations are kept: nothing is recomputed) + frozen Hiera-L fwd + mask decoder fwd+bwd."""
    return (10.8 + 30.8 - 2.3 + 28.5 + 1.82 * sam_frames + 3 * 0.0036 * sam_frames) * 1e12


# ------------------------------------------------------------------------------------------------ models / inputs
def _init_params(model):
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() >= 2:
                p.normal_(0.0, 0.02)
            elif "norm" in n or "ln_q" in n:
                p.fill_(1.0)
            else:
                p.normal_(0.0, 0.02)


def build_model(dev):
    from rga3.model.qwen2_5_vl import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration

    cfg = Qwen2_5_VLConfig()  # public Qwen2.5-VL-7B dims are the defaults
    torch.manual_seed(1)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            model = Qwen2_5_VLForConditionalGeneration(cfg)
    finally:
        torch.set_default_dtype(old)
    _init_params(model)
    return model.eval(), cfg


def make_inputs(cfg, dev, seed=0, n_video=2048, grid=(8, 32, 32)):
    """template + n_video x video_token_id + 64 others (S = 2112); config 5: n_video 4096, grid [16,32,32] (S = 4160)."""
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(grid[0] * grid[1] * grid[2], 1176, generator=g).clamp_(-1.8, 2.2).to(torch.bfloat16).to(dev)
    text = torch.randint(0, 151643, (64,), generator=g)
    ids = torch.cat([text[:14], torch.tensor([cfg.vision_start_token_id]), torch.full((n_video,), cfg.video_token_id),
                     torch.tensor([cfg.vision_end_token_id]), text[16:]])[None]
    assert ids.shape[1] == n_video + 64
    return dict(input_ids=ids.to(dev), attention_mask=torch.ones_like(ids).to(dev), pixel_values_videos=px,
                video_grid_thw=torch.tensor([list(grid)]), second_per_grid_ts=torch.tensor([1.0]))


def build_full(dev, rank, sam_frames):
    """UniGRModel at 7B + SAM2-L (random init) and one synthetic training sample (SURVEY.md 8(d) config 3, B = 1 per GPU)."""
    from rga3.model.qwen_2_5_vl_sam2 import UniGRConfig, UniGRModel
    from rga3.utils.data import make_batch

    cfg = UniGRConfig(train_mask_decoder=True, out_dim=256, ce_loss_weight=1.0, dice_loss_weight=0.5, bce_loss_weight=2.0, seg_token_idx=151665)
    torch.manual_seed(1)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            model = UniGRModel(cfg)
            model.initialize_sam_modules(cfg)
    finally:
        torch.set_default_dtype(old)
    _init_params(model)
    batch = make_batch(cfg, dev, batch=1, frames_mllm=16, frames_sam=sam_frames, seed=rank)
    return model, cfg, batch


class BatchFeed:
    """What the timed loop feeds the model.  `fresh` (default): every step gets a sample it has not seen, as NEW tensor objects, the way
    train_joint.py:500-519 draws `next(train_iter)` and calls dict_to_cuda -- the integer tensors (token ids with fresh text, the [SEG] position moving inside the
    answer, labels, attention mask) are built on the CPU per step and moved inside the timed region; the pixel tensors rotate through a pool of `pool` distinct
    samples that already sit in HBM when the timed region starts (the bench contract: inputs resident; PCIe-inclusive rate in DESIGN.md).  `repeat`: one batch,
    the same tensor objects every step, host plan reused (round 2's measurement; kept as a secondary figure)."""

    def __init__(self, mode, cfg, dev, rank, first, kind, sam_frames=16, pool=4):
        from rga3.utils.data import make_batch
        self.mode, self.cfg, self.dev, self.rank, self.first, self.kind, self.j = mode, cfg, dev, rank, first, kind, 0
        self.pool = [first]
        if mode == "fresh":
            for i in range(1, pool):
                if kind == "full":
                    self.pool.append(make_batch(cfg, dev, batch=1, frames_mllm=16, frames_sam=sam_frames, seed=rank + 7919 * i))
                else:
                    n_video, grid = (first["input_ids"].shape[1] - 64, tuple(int(v) for v in first["video_grid_thw"][0]))
                    self.pool.append(dict(first, pixel_values_videos=make_inputs(cfg, dev, seed=rank + 7919 * i, n_video=n_video, grid=grid)["pixel_values_videos"]))

    def peek_pixels(self):
        """Pixel tensors of the sample the NEXT call of next() will return (for model.prefetch_vision)."""
        big = self.pool[self.j % len(self.pool)] if self.mode == "fresh" else self.first
        return {k: big[k] for k in ("pixel_values_videos", "video_grid_thw") if k in big}

    def peek_sam(self):
        """`images_sam` of the sample the NEXT call of next() will return (for model.prefetch_sam)."""
        big = self.pool[self.j % len(self.pool)] if self.mode == "fresh" else self.first
        return big.get("images_sam")

    def next(self):
        j, self.j = self.j, self.j + 1
        if self.mode != "fresh":
            return self.first
        from rga3.utils.data import make_batch
        from rga3.utils.staging import dict_to_cuda
        big = self.pool[j % len(self.pool)]
        if self.kind == "full":
            ints = make_batch(self.cfg, None, batch=1, seed=1000003 * (self.rank + 1) + j, seg_pos=-2 - (j % 4), ints_only=True)
        else:
            g = torch.Generator().manual_seed(1000003 * (self.rank + 1) + j)
            if not hasattr(self, "_cpu_ids"):
                self._cpu_ids = self.first["input_ids"].cpu()      # once, in the warmup
            ids = self._cpu_ids.clone()
            text = (ids != self.cfg.video_token_id) & (ids != self.cfg.vision_start_token_id) & (ids != self.cfg.vision_end_token_id)
            ids[text] = torch.randint(0, 151643, (int(text.sum()),), generator=g)
            labels = torch.full_like(ids, -100)
            labels[:, -6:] = ids[:, -6:]
            ints = dict(input_ids=ids, attention_mask=torch.ones_like(ids), labels=labels)
        return dict(big, **dict_to_cuda(ints, self.dev))


def make_trainable(model, full, reducer_kw=None):
    """LoRA + trainable set of reference train_joint.py:193-251 (r128 / alpha 256 / dropout 0.05 on q_proj, v_proj of the decoder; lm_head, embed_tokens,
    and on the full model the SAM2 mask decoder + text_hidden_fcs), the bucketed gradient exchange and the fused AdamW of :300-324."""
    from rga3.model.qwen_train import add_lora
    from rga3.parallel.ddp import FusedAdamW, GradBucketReducer, sparse_candidates

    add_lora(model, r=128, alpha=256, dropout=0.05, exclude=("sam_model", "grounding_encoder", "visual", "text_hidden_fcs"))
    model.train()
    for n, p in model.named_parameters():
        p.requires_grad_(("lora_" in n) or n in ("lm_head.weight", "model.embed_tokens.weight") or (full and ("sam_mask_decoder" in n or "text_hidden_fcs" in n)))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "lora_B" in n:
                p.normal_(0.0, 0.01)
    trainables = [p for p in model.parameters() if p.requires_grad]
    sparse = sparse_candidates(model)   # [] when the table is tied to the LM head: its gradient is then dense
    reducer = GradBucketReducer(trainables, bucket_mb=256.0, sparse_params=sparse, **(reducer_kw or {}))
    opt = FusedAdamW.for_reducer(reducer, lr=4e-5, betas=(0.9, 0.95), weight_decay=0.0, max_grad_norm=1.0)   # state laid out like the buckets: one launch per bucket
    return trainables, reducer, opt


class GemmTimer:
    """HIP events (torch.cuda.Event on the stream the kernels are launched on) around every GEMM-family launch of rga3.hip.ops."""

    def __init__(self, ops):
        self.ops, self.ev, self.flops, self.bytes = ops, [], 0.0, 0.0
        self._real = {}
        self.by_kind = {}     # "bf16" / "fp8" -> [events, flops]: the two families are priced against different peaks

    def _wrap(self, name, shape_of, w_index=1, takes_kw=False):
        real = getattr(self.ops, name)
        self._real[name] = real
        kind = "fp8" if name == "gemm_fp8" else "bf16"

        def timed(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = real(*a, **k)
            e.record()
            self.ev.append((s, e))
            sh = shape_of(a, k) if takes_kw else shape_of(a)
            fl = float(sh) if not isinstance(sh, tuple) else 2.0 * sh[0] * sh[1] * sh[2]
            self.flops += fl
            slot = self.by_kind.setdefault(kind, [[], 0.0])
            slot[0].append((s, e))
            slot[1] += fl
            outs = r if isinstance(r, (tuple, list)) else (r,)
            ins = [t for t in (a[0], a[w_index]) if torch.is_tensor(t)]
            self.bytes += sum(t.numel() * t.element_size() for t in ins) + sum(t.numel() * t.element_size() for t in outs)
            return r
        setattr(self.ops, name, timed)

    def __enter__(self):
        self._wrap("gemm", lambda a: (a[0].shape[0], a[1].shape[0], a[0].shape[1]))
        self._wrap("gemm_tn", lambda a: (a[0].shape[1], a[1].shape[1], a[0].shape[0]))
        self._wrap("gemm_fp8", lambda a: (a[0].shape[0], a[2].shape[0], a[0].shape[1]))
        self._wrap("gemm_ln", lambda a: (a[0].shape[0], a[2].shape[0], a[0].shape[1]), w_index=2)   # LayerNorm-folded products of the Hiera trunk
        self._wrap("gemm_swiglu_pre", lambda a: (a[0].shape[0], a[1].shape[0], a[0].shape[1]))
        self._wrap("gemm_lnsum", lambda a: (a[0].shape[0], a[1].shape[0], a[0].shape[1]))   # the Hiera trunk's residual-writing products (+ LayerNorm partial sums; round 6)
        # concatenated operands: [a | a2] [w | w2]^T and a wn^T from one launch (flop count of both sides)
        self._wrap("gemm_cat", lambda a, k: 2.0 * a[0].shape[0] * (a[1].shape[0] * (a[0].shape[1] + (k["a2"].shape[1] if k.get("a2") is not None else 0)) +
                                                                    (k["wn"].shape[0] * a[0].shape[1] if k.get("wn") is not None else 0)), takes_kw=True)
        self._wrap("gemm_tn_many", lambda a: sum(2.0 * x.shape[1] * y.shape[1] * x.shape[0] for x, y in a[0]), w_index=0)
        return self

    def __exit__(self, *exc):
        for n, f in self._real.items():
            setattr(self.ops, n, f)

    def total_ms(self):
        torch.cuda.synchronize()
        return sum(s.elapsed_time(e) for s, e in self.ev)

    def families(self, nst):
        """per arithmetic type: launches / ms / TFLOP/s per step and the fraction of THAT type's dense MFMA peak (fp8 e4m3: 2 x bf16)."""
        torch.cuda.synchronize()
        out = {}
        for kind, (ev, fl) in self.by_kind.items():
            ms = sum(s.elapsed_time(e) for s, e in ev) / nst
            peak = PEAK_BF16 * (2.0 if kind == "fp8" else 1.0)
            out[kind] = {"launches_per_step": len(ev) // nst, "ms_per_step": round(ms, 3), "achieved": round(fl / nst / (ms * 1e-3) / 1e12, 1) if ms > 0 else None,
                         "peak": peak / 1e12, "frac": round(fl / nst / (ms * 1e-3) / peak, 4) if ms > 0 else None}
        return out


PROFILE_ROUND = "r06"      # the counter profiles bench.py quotes: profiles/<round>_bench_<tag>_<family>_traffic.json, profiles/<round>_pmc_pipe_util.json


def _tree():
    from rga3.utils.fingerprint import tree_fingerprint
    return tree_fingerprint()


def _traffic(tag, family="gemm"):
    """HBM-side traffic per launch of a kernel family cannot be sampled inside the timed run (PMC needs rocprofv3): it comes from the committed two-pass
    FETCH_SIZE / WRITE_SIZE collection of this same command, summarised by tools/pmc_traffic.py -- and ONLY from a collection made on THIS tree: the profile records
    the fingerprint of the kernel sources + package it was measured on (rga3.utils.fingerprint), and a profile of another tree is refused.
    -> (bytes per launch or None, source text, stale flag)."""
    path = os.path.join(ROOT, "profiles", f"{PROFILE_ROUND}_bench_{tag}_{family}_traffic.json")
    if not os.path.exists(path):
        return None, None, False
    tj = json.load(open(path))
    if tj.get("tree") != _tree():
        return None, f"profiles/{os.path.basename(path)} REFUSED: collected on tree {tj.get('tree')}, running tree is {_tree()}", True
    if tj.get("launches_fetch_pass") == 0 or tj.get("launches_write_pass") == 0:     # a pass that recorded nothing (the profiler died): no figure, not a zero
        return None, f"profiles/{os.path.basename(path)}: the counter passes recorded no launches", False
    return round(tj["traffic_bytes_per_launch"]), f"profiles/{os.path.basename(path)} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command on tree {tj['tree']}, bytes per launch)", False


def _put_traffic(roof, tag, family="gemm"):
    tr, src, stale = _traffic(tag, family)
    roof["traffic"] = tr
    if src:
        roof["traffic_source"] = src
    if stale:
        roof["traffic_stale"] = True


def _mfma_busy(*needles):
    """Matrix-pipe utilisation of the shipped kernels (SQ_VALU_MFMA_BUSY_CYCLES / (kernel cycles x 1024 SIMDs)) cannot be sampled inside the timed run either: it
    comes from the committed rocprofv3 --pmc passes over tools/pmc_pipe_util.py (each kernel at its bench shape), profiles/<round>_pmc_pipe_util.json -- same tree only."""
    name = f"{PROFILE_ROUND}_pmc_pipe_util.json"
    path = os.path.join(ROOT, "profiles", name)
    if not os.path.exists(path):
        return None, None
    pj = json.load(open(path))
    if pj.get("_tree") != _tree():
        return None, f"profiles/{name} REFUSED: collected on tree {pj.get('_tree')}, running tree is {_tree()}"
    out = {}
    for k, v in pj.items():
        if isinstance(v, dict) and "mfma_busy" in v and (not needles or any(n in k for n in needles)):
            out[k] = v["mfma_busy"]
    return (out or None), f"profiles/{name} (rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES + GRBM_GUI_ACTIVE passes over tools/pmc_pipe_util.py on tree {pj['_tree']}, per kernel at its bench shape)"


# ------------------------------------------------------------------------------------------------ cpu baseline (oracle "port")
def _host_threads():
    """Threads for the CPU leg: all hardware threads oversubscribe the fp32 GEMMs on SMT hosts (round 1: 256 threads ran 2.6x slower than the
    reference stack on 8 cores) -- a 2048^3 product is timed at a few thread counts and the fastest is used."""
    n = os.cpu_count() or 1
    cands = sorted({c for c in (n, n // 2, 64, 32, 16, 8) if 1 <= c <= n}, reverse=True)
    a, b = torch.randn(2048, 2048), torch.randn(2048, 2048)
    best, best_t = cands[-1], float("inf")
    for c in cands:
        torch.set_num_threads(c)
        (a @ b)
        t0 = time.perf_counter()
        for _ in range(3):
            (a @ b)
        t = time.perf_counter() - t0
        if t < best_t:
            best, best_t = c, t
    torch.set_num_threads(best)
    return best


def _oracle_vit_params(R):
    P = {"visual.patch_embed.proj.weight": R(1280, 1176), "visual.merger.ln_q.weight": torch.ones(1280),
         "visual.merger.mlp.0.weight": R(5120, 5120), "visual.merger.mlp.0.bias": R(5120), "visual.merger.mlp.2.weight": R(3584, 5120),
         "visual.merger.mlp.2.bias": R(3584)}
    for i in range(2):
        p = f"visual.blocks.{i}."
        P.update({p + "norm1.weight": torch.ones(1280), p + "norm2.weight": torch.ones(1280), p + "attn.qkv.weight": R(3840, 1280),
                  p + "attn.qkv.bias": R(3840), p + "attn.proj.weight": R(1280, 1280), p + "attn.proj.bias": R(1280),
                  p + "mlp.gate_proj.weight": R(3420, 1280), p + "mlp.gate_proj.bias": R(3420), p + "mlp.up_proj.weight": R(3420, 1280),
                  p + "mlp.up_proj.bias": R(3420), p + "mlp.down_proj.weight": R(1280, 3420), p + "mlp.down_proj.bias": R(1280)})
    return P


def _oracle_layer_params(R, lora=False):
    p = "model.layers.0."
    L = {p + "input_layernorm.weight": torch.ones(3584), p + "post_attention_layernorm.weight": torch.ones(3584),
         p + "self_attn.q_proj.weight": R(3584, 3584), p + "self_attn.q_proj.bias": R(3584), p + "self_attn.k_proj.weight": R(512, 3584),
         p + "self_attn.k_proj.bias": R(512), p + "self_attn.v_proj.weight": R(512, 3584), p + "self_attn.v_proj.bias": R(512),
         p + "self_attn.o_proj.weight": R(3584, 3584), p + "mlp.gate_proj.weight": R(18944, 3584), p + "mlp.up_proj.weight": R(18944, 3584),
         p + "mlp.down_proj.weight": R(3584, 18944), "model.norm.weight": torch.ones(3584)}
    if lora:
        L["lora_scaling"] = 2.0
        for nm, o in (("q_proj", 3584), ("v_proj", 512)):
            L[p + f"self_attn.{nm}.lora_A.default.weight"] = R(128, 3584).requires_grad_(True)
            L[p + f"self_attn.{nm}.lora_B.default.weight"] = R(o, 128).requires_grad_(True)
    return L


def cpu_baseline(train: bool, sam_frames: int = 16, seq: int = 2112, grid_t: int = 8, micro_steps: int = 1):
    """Oracle (fp32 restatement of the reference's algorithm, 'port') on the host cores, bounded sample: one windowed + one full ViT block, one decoder
    layer and a 1/16 lm_head slice at 7B dims (train: + their backward as the reference runs it under gradient checkpointing, + one SAM2-L frame
    through Hiera-L/FPN and the mask decoder fwd+bwd), extrapolated to a whole sample (28 + 4 ViT blocks, 28 layers, lm_head, sam_frames frames)."""
    from oracle import qwen25vl as Q

    cores = _host_threads()
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g) * 0.02
    tc = Q.TextCfg(num_hidden_layers=1, vocab_size=152064 // 16)
    P = _oracle_vit_params(R)
    px = torch.randn(grid_t * 1024, 1176, generator=g)
    grid = np.array([[grid_t, 32, 32]])

    def vit_time(depth, full):
        with torch.no_grad():
            t0 = time.perf_counter()
            Q.vit_forward(P, px, grid, Q.QwenCfg(vision=Q.VisionCfg(depth=depth, fullatt_block_indexes=full), text=tc))
            return time.perf_counter() - t0

    t_em = vit_time(0, ())
    t_win = vit_time(1, ()) - t_em
    t_full = vit_time(2, (1,)) - t_em - t_win
    t_vit = t_em + 28 * t_win + 4 * t_full
    cfg1 = Q.QwenCfg(vision=Q.VisionCfg(depth=0, fullatt_block_indexes=()), text=tc)
    L = _oracle_layer_params(R, lora=train)
    x = torch.randn(1, seq, 3584, generator=g)
    pos = torch.arange(seq)[None, None].expand(3, 1, -1)
    with torch.no_grad():
        t0 = time.perf_counter()
        h = Q.llm_forward(L, x, pos, None, cfg1)
        t_layer_f = time.perf_counter() - t0
    wl = R(152064 // 16, 3584)
    with torch.no_grad():
        t0 = time.perf_counter()
        (h[0] @ wl.t()).float()
        t_lm_f = (time.perf_counter() - t0) * 16
    parts = f"patch-embed+merger {t_em:.2f}s, 1 windowed ViT block {t_win:.2f}s, 1 full-attention ViT block {t_full:.2f}s, 1 decoder layer S={seq} fwd {t_layer_f:.2f}s, lm_head fwd (1/16 slice x16) {t_lm_f:.2f}s"
    if not train:
        total = t_vit + 28 * t_layer_f + t_lm_f
        return {"value": round(1.0 / total, 6), "unit": "samples/s", "cores": cores, "kind": "port",
                "sample": f"oracle fp32 at 7B dims on {cores} host threads: {parts}; extrapolated 28+4 blocks, 28 layers -> {total:.1f}s per forward"}
    # ---- backward legs, as the reference runs them: checkpointed layer = forward (no grad) + recompute + backward (train_joint.py:188)
    xg = x.clone().requires_grad_(True)
    t0 = time.perf_counter()
    hh = Q.llm_forward(L, xg, pos, None, cfg1)
    hh.square().mean().backward()
    t_layer_fb = time.perf_counter() - t0
    wlg = wl.clone().requires_grad_(True)
    hg = h[0].clone().requires_grad_(True)
    t0 = time.perf_counter()
    torch.logsumexp((hg @ wlg.t()).float(), -1).mean().backward()
    t_lm_fb = (time.perf_counter() - t0) * 16
    if sam_frames == 0:     # configs[4]: the LoRA step has no mask path; micro_steps micro-batches per optimizer step
        total = t_vit + 28 * (t_layer_f + t_layer_fb) + t_lm_fb
        return {"value": round(1.0 / total, 6), "unit": "samples/s", "cores": cores, "kind": "port",
                "sample": (f"oracle fp32 at 7B dims on {cores} host threads (of {os.cpu_count()}): {parts}, decoder layer recompute+backward {t_layer_fb:.2f}s, lm_head+CE fwd+bwd "
                           f"(1/16 slice x16) {t_lm_fb:.2f}s; extrapolated to 28+4 ViT blocks (fwd, frozen), 28 checkpointed layers, full-logits CE -> {total:.1f}s per sample "
                           f"({micro_steps} samples per optimizer step = {micro_steps * total:.1f}s); the CPU leg runs fp32 (the reference's CPU path has no e4m3 arithmetic); +-2x with host load")}
    # ---- SAM2-L: one frame through the frozen Hiera-L + FPN, mask decoder fwd+bwd
    from oracle import sam2 as S
    from rga3.model.sam2 import SAM2
    torch.manual_seed(1)
    sm = SAM2()
    PS = {}
    with torch.no_grad():
        for k, v in sm.sam2_model.state_dict().items():
            PS[k] = (torch.randn(v.shape, generator=g) * 0.02) if v.dim() >= 2 else (torch.ones(v.shape) if "norm" in k and k.endswith("weight") else torch.zeros(v.shape))
    del sm
    scfg = S.Sam2Cfg()
    img = torch.randn(1, 3, 1024, 1024, generator=g)
    with torch.no_grad():
        t0 = time.perf_counter()
        bo = S.image_encoder_forward(PS, img, scfg)
        t_enc = time.perf_counter() - t0
    for k in PS:
        if k.startswith("sam_mask_decoder."):
            PS[k].requires_grad_(True)
    feats = S.prepare_backbone_features(bo)
    emb = torch.randn(1, 1, 256, generator=g, requires_grad=True)
    t0 = time.perf_counter()
    out = S.inject_language_embd_train(PS, feats, emb, scfg)
    (out[1] if isinstance(out, (tuple, list)) else out).float().square().mean().backward()
    t_dec = time.perf_counter() - t0
    total = t_vit + 28 * (t_layer_f + t_layer_fb) + t_lm_fb + sam_frames * (t_enc + t_dec)
    return {"value": round(1.0 / total, 6), "unit": "samples/s", "cores": cores, "kind": "port",
            "sample": (f"oracle fp32 at 7B / SAM2-L dims on {cores} host threads (of {os.cpu_count()}): {parts}, decoder layer recompute+backward {t_layer_fb:.2f}s, "
                       f"lm_head+CE fwd+bwd (1/16 slice x16) {t_lm_fb:.2f}s, 1 SAM2-L frame Hiera-L+FPN {t_enc:.2f}s, mask decoder fwd+bwd {t_dec:.2f}s; extrapolated to "
                       f"28+4 ViT blocks (fwd, frozen), 28 checkpointed layers (fwd + recompute + bwd), full-logits CE, {sam_frames} SAM2 frames -> {total:.1f}s per training sample"),
            "reference_stack_note": "SURVEY.md 8(d): the reference itself (transformers 5.15 + model/sam2.py, fp32, 8 cores of the survey container) ran the same forward in about 195 s; "
                                    "its Python cannot travel to this box"}


def cpu_baseline_stream():
    """configs[3] on the host: the oracle's memory path for ONE steady-state frame at SAM2-L dims -- memory attention (4 layers, 4096 queries x 7 x 4096 + 64 keys), mask
    decoder heads, memory encoder -- with image features given (as in the timed GPU stream)."""
    from oracle import sam2 as S
    from rga3.model.sam2 import SAM2

    cores = _host_threads()
    g = torch.Generator().manual_seed(0)
    sm = SAM2()
    PS = {}
    with torch.no_grad():
        for k, v in sm.sam2_model.state_dict().items():
            PS[k] = (torch.randn(v.shape, generator=g) * 0.02) if v.dim() >= 2 else (torch.ones(v.shape) if "norm" in k and k.endswith("weight") else torch.zeros(v.shape))
    del sm
    cfg = S.Sam2Cfg()
    nq, nk, nptr = 4096, 7 * 4096 + 64, 64
    R = lambda *s: torch.randn(*s, generator=g)
    with torch.no_grad():
        t0 = time.perf_counter()
        pix = S.memory_attention(PS, R(nq, 1, 256), R(nq, 1, 256), R(nk, 1, 64), R(nk, 1, 64), nptr, cfg)
        t_ma = time.perf_counter() - t0
        pixm = pix.permute(1, 2, 0).reshape(1, 256, 64, 64)
        high = [R(1, 32, 256, 256), R(1, 64, 128, 128)]
        t0 = time.perf_counter()
        o = S.forward_sam_heads(PS, pixm, high, None, cfg, True)
        t_dec = time.perf_counter() - t0
        t0 = time.perf_counter()
        S.memory_encoder(PS, R(1, 256, 64, 64), o["high_res_masks"], cfg)
        t_me = time.perf_counter() - t0
    total = t_ma + t_dec + t_me
    return {"value": round(1.0 / total, 4), "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": (f"oracle fp32 at SAM2-L dims on {cores} host threads (of {os.cpu_count()}), ONE steady-state frame with image features given: memory attention over "
                       f"28 736 keys {t_ma:.2f}s, mask decoder heads {t_dec:.2f}s, memory encoder {t_me:.2f}s -> {total:.2f}s per frame; +-2x with host load")}


# ------------------------------------------------------------------------------------------------ --dump-outputs
DUMP_CAP = 1 << 20           # elements per written array: a larger output is written as a fixed, seeded sample of this many elements
DUMP_BUDGET = 64 << 20       # bytes over all arrays of one run
_dumped = [0]


def _sample(t, cap=DUMP_CAP):
    """`t` itself when it has at most `cap` elements, else the same `cap` (sorted) flat positions of it in every run."""
    t = t.detach()
    if t.numel() <= cap:
        return t
    idx = torch.randint(0, t.numel(), (cap,), generator=torch.Generator().manual_seed(0)).sort().values
    return t.reshape(-1)[idx.to(t.device)]


def dump_outputs(args, arrays, cap=DUMP_CAP):
    """--dump-outputs DIR: {name: tensor} of the last timed step as DIR/<name>.npy, float32 (a tensor of more than `cap` elements sampled by _sample)."""
    if not args.dump_outputs:
        return
    os.makedirs(args.dump_outputs, exist_ok=True)
    host = {k: _sample(v, cap).float().cpu().numpy() for k, v in arrays.items()}
    _dumped[0] += sum(a.nbytes for a in host.values())
    assert _dumped[0] <= DUMP_BUDGET, f"--dump-outputs: {_dumped[0]} bytes, over the {DUMP_BUDGET}-byte budget"
    for k, a in host.items():
        np.save(os.path.join(args.dump_outputs, k + ".npy"), a)


# ------------------------------------------------------------------------------------------------ launcher
def launch_ranks(args):
    """Parent of a multi-GPU run: never touches the GPU (torch.cuda.device_count() does not initialise it on this image), starts N ranks of this file
    through torch.distributed.run and exits with their code (reference launcher: run_torchrun.sh:6-12,23)."""
    if args.mode != "ddp_selftest" and not os.environ.get("RGA3_BENCH_SHARE_GPU"):
        n_vis = torch.cuda.device_count()
        if n_vis < args.gpus:
            print(f"bench.py: {args.gpus} GPUs requested, {n_vis} visible", file=sys.stderr)
            sys.exit(2)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


def ddp_selftest(args, rank, world):
    """CPU / gloo run of the same launcher, rendezvous, gradient-exchange and timing code with a toy torch module in place of the model (no HIP kernels:
    tests/test_bench_launcher.py drives `bench.py --gpus 2 --mode ddp_selftest` here, where there is no GPU).  Not a benchmark line."""
    import torch.distributed as dist
    from rga3.parallel.ddp import GradBucketReducer

    if world > 1:
        dist.init_process_group(backend="gloo")
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.ReLU(), torch.nn.Linear(256, 8))
    params = list(net.parameters())
    reducer = GradBucketReducer(params, bucket_mb=0.02)
    x = torch.randn(32, 64, generator=torch.Generator().manual_seed(rank))

    def step():
        reducer.begin_step()
        reducer.begin_micro_step()
        net(x).square().mean().backward()
        reducer.finish()

    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if world > 1:
        dist.barrier()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    g0 = reducer.grad_view(params[0]).clone()
    same = True
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
        gs = [torch.empty_like(g0) for _ in range(world)]
        dist.all_gather(gs, g0)
        same = all(torch.equal(gs[0], t) for t in gs)
    if rank == 0:
        dump_outputs(args, {"grad_param0": g0})
        print(json.dumps({"selftest": True, "metric": "ddp launcher self-test (toy module, CPU, gloo)", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(float(el) / args.steps * 1e3, 3), "replicas_agree": bool(same), "buckets": len(reducer.buckets)}), flush=True)
    if world > 1:
        dist.destroy_process_group()
    sys.exit(0 if same else 1)


# ------------------------------------------------------------------------------------------------ sam2 stream (configs[3])
def sam2_stream(args, dev, rank, world, dist):
    """BASELINE configs[3]: one step = one 32-frame ref-VOS stream through SAM2-L's memory path -- language
    prompt on frame 0 only, then propagate (memory attention over the growing bank, mask decoder, memory encoder per frame).
    `value` counts the stream with the per-frame image features already computed ("memory-attention mask-decoder only"); the
    encoder-inclusive rate is reported beside it."""
    from rga3.model import sam2 as sam2_mod
    from rga3.model.sam2 import SAM2, MultiObjectSession, VideoSession

    NOBJ = max(1, int(args.objects))
    if args.no_rowchain:
        sam2_mod._ROWCHAIN = False      # A/B: the row-wise steps of the memory-attention layers as separate launches
    T = args.stream_frames
    torch.manual_seed(1)
    m = SAM2().to(torch.bfloat16).to(dev).eval()
    with torch.no_grad():
        for n, p_ in m.named_parameters():
            if p_.dim() >= 2:
                p_.normal_(0, 0.02)
    g = torch.Generator().manual_seed(rank)
    vid = torch.randn(T, 3, 1024, 1024, generator=g).to(torch.bfloat16).to(dev)
    emb = torch.randn(1, 1, 256, generator=g).to(torch.bfloat16).to(dev)
    embs_obj = [emb] + [torch.randn(1, 1, 256, generator=g).to(torch.bfloat16).to(dev) for _ in range(NOBJ - 1)]

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    with torch.no_grad():
        s0 = VideoSession(m.sam2_model, vid)
        feats = s0._ensure_feats()          # image encoder, once (kept across steps: the timed region is the memory path)

        def step(use_graph=True, nobj=NOBJ, concurrent=True):
            if nobj > 1:   # --objects N: N objects prompted on frame 0 and tracked together on the shared features (reference: batch_size = n_obj per frame, sam2.py:3977-4132)
                ms_ = MultiObjectSession(m.sam2_model, vid, nobj, feats=feats)
                for o in range(nobj):
                    ms_.add_language_embd(0, o, embs_obj[o])
                return ms_.sessions[0], ms_.propagate(use_graph=use_graph and not args.no_graph, concurrent=concurrent)
            sess = VideoSession(m.sam2_model, vid, feats=feats)
            sess.add_language_embd(0, emb)
            return sess, sess.propagate(use_graph=use_graph and not args.no_graph)   # steady-state frames (16..) replay one captured hipGraph

        for _ in range(args.warmup):
            step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            sess, res = step()
        barrier()
        elapsed = time.perf_counter() - t0
        if rank == 0:
            dump_outputs(args, {"stream_masks": torch.stack([m_ for _, m_ in res])})
        # a plain run, and profiling runs: nothing after the timed stream (the variants below would end the trace)
        timed_only = bool(os.environ.get("RGA3_BENCH_TIMED_ONLY")) or not args.full
        multi = None
        if NOBJ > 1 and not timed_only:   # the same objects one after the other on one stream, and ONE object: what tracking them together buys
            def timed(**kw):
                step(**kw)
                barrier()
                t_ = time.perf_counter()
                for _ in range(args.steps):
                    step(**kw)
                barrier()
                return (time.perf_counter() - t_) / args.steps
            t_seq, t_one = timed(concurrent=False), timed(nobj=1)
            multi = {"objects": NOBJ, "object_frames_per_s": round(NOBJ * T / (elapsed / args.steps), 2),
                     "object_frames_per_s_objects_one_after_the_other": round(NOBJ * T / t_seq, 2), "single_object_frames_per_s": round(T / t_one, 2),
                     "vs_single_object": round(NOBJ * t_one / (elapsed / args.steps), 3)}
        # encoder-inclusive variant (fresh features every stream), same number of steps
        barrier()
        t1 = time.perf_counter()
        for _ in range(0 if timed_only else args.steps):
            se = VideoSession(m.sam2_model, vid)
            se.add_language_embd(0, emb)
            se.propagate()
        barrier()
        elapsed_enc = max(time.perf_counter() - t1, 1e-9)
        # reference-usage variant: language prompt on EVERY frame (what evaluate() does, reference
        # qwen_2_5_vl_sam2.py:378-404): mask decoder per frame, no memory attention, no memory encoder; features precomputed
        embs = [[emb[0]] for _ in range(T)]
        if not timed_only:
            sess_p = VideoSession(m.sam2_model, vid, feats=feats)
            m.language_embd_inference(sess_p, embs)
        barrier()
        t2 = time.perf_counter()
        for _ in range(0 if timed_only else args.steps):
            sess_p = VideoSession(m.sam2_model, vid, feats=feats)
            m.language_embd_inference(sess_p, embs)
        barrier()
        elapsed_prompt = max(time.perf_counter() - t2, 1e-9)
    # ---- dominant kernel of the stream, live: HIP events around every memory cross-attention launch of one EAGER stream (events cannot sit inside a replayed graph;
    # same kernel, same operands), algorithmic flops / bytes of the launched shapes
    dom = None
    if rank == 0 and not timed_only:
        from rga3.hip import ops as _ops
        real, evs, acc = _ops.memattn_cross, [], [0.0, 0.0]

        def timed(q, k, mm, scale, nsplit=0, **kw):
            s_, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s_.record()
            r_ = real(q, k, mm, scale, nsplit, **kw)
            e_.record()
            evs.append((s_, e_))
            acc[0] += 2.0 * q.shape[0] * k.shape[0] * (256 + 64)                               # QK^T over 256 + PM over 64
            acc[1] += 2.0 * (q.numel() + k.numel() + mm.numel() + q.shape[0] * 64)             # q, k, memory read once, PM written (bf16)
            return r_
        _ops.memattn_cross = timed
        try:
            with torch.no_grad():
                step(use_graph=False)
            torch.cuda.synchronize()
        finally:
            _ops.memattn_cross = real
        tot = sum(a.elapsed_time(b) for a, b in evs)
        n = len(evs)
        dom = {"bound": "mfma", "kernel": ("memattn_cross_kernel + memattn_combine_kernel" if args.no_rowchain else "memattn_cross_kernel (its key slices are merged by the consumer, memlayer_rows_kernel)")
               + " (csrc/memattn.hip: 32x32x16 bf16 MFMA, values kept in the 64-wide memory space)",
               "launches_per_stream": n, "avg_launch_ms": round(tot / max(n, 1), 5), "achieved": round(acc[0] / (tot * 1e-3) / 1e12, 1), "peak": PEAK_BF16 / 1e12,
               "unit": "TFLOP/s", "frac": round(acc[0] / (tot * 1e-3) / PEAK_BF16, 4), "algorithmic_flops_per_launch": acc[0] / max(n, 1),
               "algorithmic_bytes_per_launch": acc[1] / max(n, 1),
               "note": "flops as THIS kernel computes them (2 Nq Nk (256 + 64)); the reference's formulation (values projected to 256 first) would be 2 Nq Nk 512"}
        _put_traffic(dom, "sam2_stream", "memattn")
    if dist is not None:
        t = torch.tensor([elapsed, elapsed_enc, elapsed_prompt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, elapsed_enc, elapsed_prompt = float(t[0]), float(t[1]), float(t[2])
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        fps = world * NOBJ * T / (elapsed / args.steps)     # object-frames per second (= frames/s for the single object of configs[3])
        # algorithmic FLOPs per frame of the memory path: memory attention <= 0.61 T (cross-attention grows with the bank:
        # 4.19 M x KV, KV = 4096 x min(t, 7) + 4 x min(t, 16) pointer tokens), memory encoder 11.6 G, mask decoder 3.6 G
        fl, by = 0.0, 0.0
        for tt in range(1, T):
            kv = 4096 * min(tt, 7) + 4 * min(tt, 16)
            fl += 54.8e9 + 68.7e9 + 4.19e6 * kv + 11.6e9 + 3.6e9
            # algorithmic HBM bytes per frame (SURVEY.md 8(d) "Algorithmic bytes"): frame features in (64x64x256 + 128x128x64 + 256x256x32 bf16 = 7.3 MB), the bank
            # (64-d bf16 memory + its position table, min(t, 7) slots) read once per frame, the new memory slot written (0.52 MB), the selected
            # 1024x1024 f32 mask written (4.2 MB) and re-read by the memory encoder, weights of the three modules (11.5 M params bf16 = 23 MB, L2/MALL-resident)
            by += 7.3e6 + 2 * (64 * 4096 * 2) * min(tt, 7) + 0.52e6 + 2 * 4.2e6 + 23e6
        fl, by = fl * NOBJ, by * NOBJ - (NOBJ - 1) * (T - 1) * (7.3e6 + 23e6)     # per object; the frame's features and the weights are read once for all objects
        sec = elapsed / args.steps
        line = {"metric": "SAM2-L memory-attention mask-decoder stream, frames/sec (32-frame 1024x1024 ref-VOS stream, prompt on frame 0)", "value": round(fps, 2),
                "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                "config": {"workload": f"BASELINE.json configs[3]: SAM2-L (random init) memory path over {T} frames 1024x1024: frame 0 prompted with a language "
                                       "embedding, frames 1.. propagate (memory attention over <= 7 memory frames + <= 16 object pointers, mask decoder, "
                                       "memory encoder); image features precomputed outside the timed region", "frames": T, "parallelism": f"replicas x{world}",
                           "prompt_every_frame_frames_per_s": None if timed_only else round(world * T / (elapsed_prompt / args.steps), 2),
                           "encoder_inclusive_frames_per_s": None if timed_only else round(world * T / (elapsed_enc / args.steps), 2), "counts": sess.counts, "objects": NOBJ, "multi_object": multi},
                "roofline": dom if dom is not None else {"bound": "mfma", "achieved": None, "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s", "frac": None, "traffic": None},
                "roofline_stream": {"bound": "mfma", "achieved": round(fl / sec / 1e12, 1), "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s",
                                    "frac": round(fl / sec / PEAK_BF16, 4), "traffic": None,
                                    "note": "whole-stream algorithmic FLOPs (SURVEY.md 8(d) formulation: values projected to 256) / stream time; the attention cores are MFMA-bound, "
                                            "the streaming stages HBM-bound (report both roofs)"},
                "roofline_hbm": {"bound": "hbm", "achieved": round(by / sec / 1e9, 1), "peak": PEAK_HBM / 1e9, "unit": "GB/s", "frac": round(by / sec / PEAK_HBM, 4), "traffic": None,
                                 "algorithmic_bytes_per_frame": round(by / (T - 1)),
                                 "note": "whole-stream algorithmic HBM bytes (frame features, bank + position table once per frame, new memory slot, selected mask write + re-read, "
                                         "module weights) / stream time"},
                "cpu_baseline": None if (args.no_cpu_baseline or world > 1 or timed_only) else cpu_baseline_stream()}
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()


_PROFILER_ENV = ("LD_PRELOAD", "ROCP_TOOL_LIBRARIES", "ROCP_TOOL_LIB", "HSA_TOOLS_LIB", "ROCPROFILER_", "ROCPROF_", "ROCP_")


def _under_profiler():
    """True when a profiler's preload environment is present: a child started from here would inherit it (and a '#!/usr/bin/env python3' child such as rocm-smi
    would then take an exec hop with the GPU already initialised by the preloaded library -- forbidden on this pool)."""
    return any(k == p or (p.endswith("_") and k.startswith(p)) for k in os.environ for p in _PROFILER_ENV)


def _sysfs_board():
    """[(power file, clock file)] of every amdgpu card the kernel exposes: hwmon power1_average / power1_input (microwatts) and freq1_input (Hz) -- plain file
    reads inside this process, nothing is spawned."""
    import glob
    cards = []
    for hw in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")):
        pw = next((os.path.join(hw, n) for n in ("power1_average", "power1_input") if os.path.exists(os.path.join(hw, n))), None)
        fq = os.path.join(hw, "freq1_input")
        if pw is not None:
            cards.append((pw, fq if os.path.exists(fq) else None))
    return cards


def _read_number(path):
    try:
        with open(path) as f:
            return float(f.read().split()[0])
    except Exception:   # noqa: BLE001
        return None


def _board_sample(step, seconds=3.0):
    """Board power / shader clock WHILE `step` runs in a loop (outside the timed region): every GEMM tiling of this model runs at the board's power cap (DESIGN.md
    lesson 7), so the clock the run held is part of the measurement.  Read from sysfs in-process (hwmon power1_average, freq1_input) by a side thread; with several
    cards visible in sysfs the busiest one (highest power under this load) is reported.  rocm-smi is only a fallback, never under a profiler, and its child gets an
    environment without the profiler's variables.  None when neither source says anything."""
    import re
    import subprocess
    import threading
    samples, stop = [], [False]
    cards = _sysfs_board()
    profiled = _under_profiler()
    if not cards and profiled:
        return None

    def poll_sysfs():
        time.sleep(0.4)
        while not stop[0] and len(samples) < 6:
            best = None
            for pw, fq in cards:
                w = _read_number(pw)
                if w is not None and (best is None or w > best[0]):
                    best = (w, _read_number(fq) if fq else None)
            if best is not None:
                samples.append({"power_w": round(best[0] / 1e6, 1), "sclk_mhz": None if best[1] is None else int(best[1] / 1e6)})
            time.sleep(0.4)

    def poll_smi():
        time.sleep(0.4)
        env = {k: v for k, v in os.environ.items() if not any(k == p or (p.endswith("_") and k.startswith(p)) for p in _PROFILER_ENV)}
        while not stop[0] and len(samples) < 3:
            try:
                out = subprocess.run(["rocm-smi", "--showpower", "--showclocks"], capture_output=True, text=True, timeout=15, env=env).stdout
            except Exception:   # noqa: BLE001
                return
            d = {}
            m = re.search(r"(?:Average|Current Socket) Graphics Package Power \(W\):\s*([\d.]+)", out)
            if m:
                d["power_w"] = float(m.group(1))
            m = re.search(r"sclk clock level:\s*\d+:?\s*\((\d+)Mhz\)", out)
            if m:
                d["sclk_mhz"] = int(m.group(1))
            if d:
                samples.append(d)

    try:
        th = threading.Thread(target=poll_sysfs if cards else poll_smi, daemon=True)
        th.start()
        t0 = time.perf_counter()
        while th.is_alive() and time.perf_counter() - t0 < seconds:
            step()
            torch.cuda.synchronize()
        stop[0] = True
        th.join(timeout=20)
    except Exception:   # noqa: BLE001
        return None
    if not samples:
        return None
    return {"power_w": [x.get("power_w") for x in samples], "sclk_mhz": [x.get("sclk_mhz") for x in samples], "source": "sysfs hwmon" if cards else "rocm-smi",
            "note": "sampled while the timed forward repeats (after the timed region); idle: ~310 W at 2400 MHz; the bf16 peak of the roofline (2.5 PFLOP/s) is the 2400 MHz figure"}


# ------------------------------------------------------------------------------------------------ main
def _median_unless_above(step, reps, bar):
    """tuner._time_step's median of `reps` timed steps, or inf as soon as that median can no longer fall below `bar`: with k of the reps known, the median
    is at least their (reps // 2 - (reps - k))-th fastest, whatever the runs still to come give."""
    ts = []
    for k in range(1, reps + 1):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        step()
        en.record()
        en.synchronize()
        ts.append(st.elapsed_time(en))
        ts.sort()
        lo = reps // 2 - (reps - k)
        if k < reps and lo >= 0 and ts[lo] >= bar:
            return float("inf")
    return ts[reps // 2]


def refine_tilings(step, reps=5, within=1.5, min_gain=0.002):
    """tuner.refine with the same decision rule (a candidate tiling replaces the current one when the step's median of `reps` runs beats the best so far by
    `min_gain`), but a candidate is dropped after the runs that already rule it out: a clearly slower tiling costs 3 runs of 5, not 5."""
    from rga3.hip import tuner
    if not tuner._enabled:
        return {}
    step()
    torch.cuda.synchronize()
    changed = {}
    base = tuner._time_step(step, reps)
    for key in list(tuner._cache):
        tm = tuner._times.get(key)
        if not tm:
            continue
        cur = tuner._cache[key]
        lim = min(tm.values()) * within
        best_t, best_ms = cur, base
        for cand in sorted((t for t in tm if t != cur and tm[t] <= lim), key=lambda t: tm[t]):
            tuner._cache[key] = cand
            ms = _median_unless_above(step, reps, best_ms * (1.0 - min_gain))
            if ms < best_ms * (1.0 - min_gain):
                best_t, best_ms = cand, ms
        tuner._cache[key] = best_t
        if best_t != cur:
            changed[key] = (cur, best_t)
            base = best_ms
    return changed


def measure_forward(model_fwd, inputs, args, rank, refine=True):
    """configs[1]: K timed forwards (+ the GEMM-family instrumented pass and the output check on rank 0).  Returns (ms per step, roofline dict, verify dict)."""
    from rga3.hip import ops, tuner

    def step():
        with torch.no_grad():
            return model_fwd(**inputs)

    if refine and not args.no_refine:
        rw, rr = (os.environ.get("RGA3_REFINE", "1.5,5").split(",") + ["5"])[:2]
        ch = refine_tilings(step, reps=int(rr), within=float(rw))
        if rank == 0 and ch:
            print("tuner.refine changed %d shape(s): %s" % (len(ch), {str(k[:3]): v for k, v in ch.items()}), file=sys.stderr)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    if rank == 0:
        dump_outputs(args, {"forward_logits": out.logits})
    if rank != 0 or os.environ.get("RGA3_BENCH_TIMED_ONLY"):   # (the env switch ends the process after the timed steps: rocprofv3 timeline captures)
        return ms, None, None
    if not args.full:       # a plain run: the roofline, variants and output check below are --full only
        assert ops.gemm_stream_k_timeouts() == 0, "stream-K hand-off timed out: results of this run are not trustworthy"
        return ms, None, None
    # ---- same process, same board, interleaved: the two round-4 changes of this path switched off one at a time (boards differ by +-2 %: only an A/B inside
    #      one process prices a 1 - 2 % change).  Tilings stay as decided above; the unfolded route launches the same product shapes.
    import rga3.model.qwen2_5_vl as _QM

    def timed_ms(n):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t1) / n * 1e3

    ab = {"as_timed": [], "no_rmsnorm_fold": [], "general_causal_attention": [], "query_rope_standalone": []}
    nab = max(4, args.steps // 2)
    for _ in range(2):
        ab["as_timed"].append(timed_ms(nab))
        _QM.set_rms_fold(False); step(); ab["no_rmsnorm_fold"].append(timed_ms(nab)); _QM.set_rms_fold(True)
        # (rope-in-attention off too: its entry point has no switch and would keep the long causal rows on the same kernel as 'as_timed')
        ops.set_causal32(False); _QM.set_rope_in_attn(False); step(); ab["general_causal_attention"].append(timed_ms(nab)); ops.set_causal32(True); _QM.set_rope_in_attn(True)
        _QM.set_rope_in_attn(False); step(); ab["query_rope_standalone"].append(timed_ms(nab)); _QM.set_rope_in_attn(True)
    step()
    variants_fwd = {k: round(min(v), 3) for k, v in ab.items()}
    variants_fwd["note"] = "ms per forward, min of 2 interleaved rounds of %d steps in this process: RMSNorm folded into the neighbouring products off; long causal rows on the general attention kernel (queries rotated by the stand-alone pass, as that kernel needs); decoder queries rotated by the stand-alone RoPE pass instead of inside the attention kernel" % nab
    with GemmTimer(ops) as gt:
        for _ in range(args.steps):
            step()
        tot_ms = gt.total_ms()
    n_launch = len(gt.ev) // args.steps
    gemm_ms_step = tot_ms / args.steps
    achieved = GEMM_FLOPS / (gemm_ms_step * 1e-3) / 1e12
    roof = {"bound": "mfma", "kernel": "gemm_nt_* family: gemm_nt_pp_kernel / gemm_nt_sk_kernel / gemm_nt_kernel (bf16 16x16x32 MFMA)",
            "workload": "BASELINE.json configs[1]: Qwen2.5-VL-7B ViT+LLM forward, 16 frames 448x448 (grid [8,32,32]), S=2112, bf16 (measured in this process on the same weights)",
            "achieved": round(achieved, 1), "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s", "frac": round(achieved * 1e12 / PEAK_BF16, 4), "traffic": None,
            "launches_per_step": n_launch, "avg_launch_ms": round(gemm_ms_step / max(n_launch, 1), 5), "gemm_ms_per_step": round(gemm_ms_step, 3),
            "forward_ms_per_step": round(ms, 3), "forward_samples_per_s": round(1e3 / ms, 3),
            "whole_forward_frac": round(TOTAL_FLOPS / (ms * 1e-3) / PEAK_BF16, 4), "flops_per_forward": TOTAL_FLOPS,
            "algorithmic_bytes_per_launch": round(gt.bytes / max(len(gt.ev), 1)), "variants_ms": variants_fwd}
    _put_traffic(roof, "forward")
    board = None if getattr(args, "no_board", False) else _board_sample(step)
    if board is not None:
        roof["board"] = board
    mb, msrc = _mfma_busy("gemm_nt", "attn_causal32", "attn_win")
    if msrc is not None:
        roof["mfma_busy"], roof["mfma_busy_source"] = mb, msrc
    # ---- the timed output is checked.  (a) every distinct GEMM shape of the timed forward is re-run, on the same operands, on the first-generation
    #      single-phase 256x256 tiling (id 10) and must agree to bf16 rounding (stream-K / split-K tilings only reorder the f32 sums);
    #      (b) the whole forward on tile 10 is reported beside it: random-init 28-layer stacks amplify one-ulp differences, so that figure is loose.
    lg = out.logits.float()
    assert torch.isfinite(lg).all(), "non-finite logits"
    real_gemm, seen, worst = ops.gemm, {}, [0.0, None]

    def checked_gemm(a, w, bias=None, residual=None, act="none", out_dtype=torch.bfloat16, out=None, tile=-1, colscale=None, rms_in=None, rms_out=None):
        r = real_gemm(a, w, bias, residual=residual, act=act, out_dtype=out_dtype, out=out, tile=tile, colscale=colscale, rms_in=rms_in, rms_out=rms_out)
        key = (a.shape[0], w.shape[0], a.shape[1], act, bias is not None, residual is not None)
        if key not in seen and out is None and tile == -1 and a.shape[0] > 4:
            # (the reference launch takes the same row sums in, but must not ADD its own into the caller's buffer a second time)
            r10 = real_gemm(a, w, bias, residual=residual, act=act, out_dtype=out_dtype, tile=10, colscale=colscale, rms_in=rms_in)
            e = float((r.float() - r10.float()).norm() / (r10.float().norm() + 1e-30))
            seen[key] = e
            if e > worst[0]:
                worst[0], worst[1] = e, key
        return r

    ops.gemm = checked_gemm
    try:
        step()
    finally:
        ops.gemm = real_gemm
    with tuner.force(10):
        ref = step().logits.float()
    rel = float((lg - ref).norm() / ref.norm())
    verify = {"gemm_shapes_checked_vs_tile10": len(seen), "gemm_worst_rel_l2_vs_tile10": round(worst[0], 6), "gemm_worst_shape": str(worst[1]),
              "logits_rel_l2_vs_all_tile10_forward": round(rel, 5), "logits_abs_sum": round(float(lg.abs().sum()), 3),
              "logits_argmax_sum": int(lg.argmax(-1).sum()), "stream_k_timeouts": ops.gemm_stream_k_timeouts()}
    assert len(seen) >= 8 and worst[0] < 2e-3, f"a timed GEMM disagrees with the tile-10 reference kernel: {worst}"
    assert rel < 0.15, f"timed forward far from the all-tile-10 forward: rel-L2 {rel}"
    assert verify["stream_k_timeouts"] == 0, "stream-K hand-off timed out: results of this run are not trustworthy"
    return ms, roof, verify


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond `value`, after the timed steps: CPU baseline, configs[1] forward roofline with its variants, "
                         "board sample and tile-10 output check, the training step's GEMM-family pass and variants, the multi-GPU exchange report, the "
                         "sam2_stream variants and dominant-kernel pass.  Off: set up, warm up, time the steps, --dump-outputs, print the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-board", action="store_true", help="--full without the board power / shader clock sample (roofline.board)")
    ap.add_argument("--mode", choices=["headline", "forward", "train", "train_full", "sam2_stream", "lora_fp8", "ddp_selftest"], default="headline",
                    help="headline (default) = BASELINE metric: configs[2] per GPU, full RGA3 (Qwen2.5-VL-7B + SAM2-L, 16 SAM frames) fwd+bwd + AdamW as `value`, plus (--full) the "
                         "configs[1] forward roofline in the same line; forward = configs[1] only; train = LLM-side LoRA step without SAM2; train_full = headline without "
                         "the forward leg; lora_fp8 = configs[4]: LoRA step, 32 frames 448x448 (S = 4160), grad-accum 4, e4m3 GEMMs for the frozen decoder weights; "
                         "sam2_stream = configs[3]: SAM2-L memory-attention mask-decoder stream over 32 frames 1024x1024, prompt on frame 0; "
                         "ddp_selftest = launcher / gradient-exchange self-test on CPU with gloo (tests only)")
    ap.add_argument("--stream-frames", type=int, default=32)
    ap.add_argument("--grad-accum", type=int, default=4)
    ap.add_argument("--no-fp8", action="store_true", help="lora_fp8 mode with bf16 GEMMs (A/B)")
    ap.add_argument("--no-rowchain", action="store_true", help="sam2_stream mode: A/B of csrc/memlayer.hip (the row-wise steps between the attention kernels as separate launches)")
    ap.add_argument("--objects", type=int, default=1, help="sam2_stream mode: objects tracked per clip on shared image features (value = object-frames/s; 1 = configs[3])")
    ap.add_argument("--no-graph", action="store_true", help="sam2_stream mode: run every frame eagerly (A/B of the hipGraph replay)")
    ap.add_argument("--no-refine", action="store_true", help="skip the in-situ tile refinement of the forward leg (A/B)")
    ap.add_argument("--refine", action="store_true", help="training modes, 1 GPU: run the in-situ tile refinement before the warmup")
    ap.add_argument("--dense-embed-grad", action="store_true", help="exchange embed_tokens' gradient as a dense bucket (A/B of the sparse row exchange)")
    ap.add_argument("--sam-frames", type=int, default=16)
    ap.add_argument("--sam-prefetch-layer", type=int, default=7, help="training modes: the next sample's SAM2 encoder is launched when the backward reaches this decoder layer")
    ap.add_argument("--no-sam-prefetch", action="store_true", help="training modes: do not run the frozen SAM2 image encoder of the next sample beside the optimizer step (A/B)")
    ap.add_argument("--no-prefetch", action="store_true", help="training modes: do not run the frozen vision tower of the next sample one step ahead on a side stream (A/B)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32; a large "
                                                             "output as a fixed, seeded sample; at most 64 MB in all): inputs are seeded, so two builds compare output for output")
    ap.add_argument("--batches", choices=["fresh", "repeat"], default="fresh",
                    help="training modes: fresh = a new sample (new tensor objects, new token ids, [SEG] position, pixel tensors from a resident pool of 4) every step, as a "
                         "training loop feeds it; repeat = the same tensor objects every step with the host plan reused (round 2's measurement)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return launch_ranks(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    if args.mode == "ddp_selftest":
        return ddp_selftest(args, rank, world)
    # RGA3_BENCH_SHARE_GPU=1 (+ RGA3_BENCH_BACKEND=gloo): every rank on GPU 0 -- a functional check of the multi-rank code path (hooks, bucket order, sparse row
    # exchange, side streams) on a 1-GPU box; RCCL itself refuses two ranks on one device, so this is never a measurement
    share = bool(os.environ.get("RGA3_BENCH_SHARE_GPU"))
    n_vis = torch.cuda.device_count()
    if not share and n_vis < max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world))):
        print(f"bench.py: {args.gpus} GPUs requested, {n_vis} visible", file=sys.stderr)
        sys.exit(2)
    if share:
        local = 0
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        backend = os.environ.get("RGA3_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)

    from rga3.hip import lib, ops
    lib.load()  # fail loudly if the HIP extension is missing
    if args.mode == "sam2_stream":
        return sam2_stream(args, dev, rank, world, dist)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    full = args.mode in ("headline", "train_full")
    fwd_roof = fwd_verify = None
    fwd_ms = None
    if full:
        model, cfg, inputs = build_full(dev, rank, args.sam_frames)
    else:
        model, cfg = build_model(dev)
        inputs = make_inputs(cfg, dev, seed=rank, n_video=4096, grid=(16, 32, 32)) if args.mode == "lora_fp8" else make_inputs(cfg, dev, seed=rank)

    # ---- configs[1] forward leg (before LoRA is attached: the plain Qwen2.5-VL-7B forward on the very weights the training step then uses)
    if args.mode in ("headline", "forward"):
        from rga3.model.qwen2_5_vl import Qwen2_5_VLForConditionalGeneration
        fin = make_inputs(cfg, dev, seed=rank)
        model.eval()
        fwd_ms, fwd_roof, fwd_verify = measure_forward(lambda **kw: Qwen2_5_VLForConditionalGeneration.forward(model, **kw), fin, args, rank)
        del fin
        if args.mode == "forward":
            barrier()
            t = torch.tensor([fwd_ms], device=dev, dtype=torch.float64)
            if dist is not None:
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ms = float(t.item())
            if rank == 0:
                cpu = None if (not args.full or args.no_cpu_baseline or world > 1) else cpu_baseline(train=False)
                if fwd_roof is None:    # a plain run: whole-forward algorithmic FLOPs / forward time (no run of its own)
                    fwd_roof = {"bound": "mfma", "achieved": round(TOTAL_FLOPS / (ms * 1e-3) / 1e12, 1), "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s",
                                "frac": round(TOTAL_FLOPS / (ms * 1e-3) / PEAK_BF16, 4), "traffic": None, "flops_per_forward": TOTAL_FLOPS,
                                "note": "whole-forward algorithmic FLOPs / forward time; the GEMM-family figures need --full"}
                line = {"metric": "video-QA samples/sec at 7B/16-frame (configs[1]: visual-encoder+LLM forward)", "value": round(world * 1e3 / ms, 4),
                        "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3),
                        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                        "config": {"workload": "BASELINE.json configs[1]: Qwen2.5-VL-7B ViT+LLM forward, 16 frames 448x448 (grid [8,32,32]), S=2112, "
                                               "bf16, 1 sample/GPU, random-init weights", "per_gpu_batch": 1, "seq_len": 2112, "parallelism": f"replicas x{world}",
                                   "flops_per_sample": TOTAL_FLOPS},
                        "roofline": fwd_roof, "verify": fwd_verify, "cpu_baseline": cpu}
                print(json.dumps(line), flush=True)
                if os.environ.get("RGA3_TUNE_SAVE"):
                    from rga3.hip import tuner
                    tuner.save(os.environ["RGA3_TUNE_SAVE"])
            if dist is not None:
                dist.destroy_process_group()
            return

    # ---- training step
    accum = args.grad_accum if args.mode == "lora_fp8" else 1
    trainables, reducer, opt = make_trainable(model, full, reducer_kw={"sparse": not args.dense_embed_grad})
    if not full:
        labels = torch.full_like(inputs["input_ids"], -100)
        labels[:, -6:] = inputs["input_ids"][:, -6:]
        inputs["labels"] = labels
    if args.mode == "lora_fp8" and not args.no_fp8:
        from rga3.model.qwen_train import set_fp8_frozen_gemms
        set_fp8_frozen_gemms(True)
    losses = []
    feed = BatchFeed(args.batches, cfg, dev, rank, inputs, "full" if full else "llm", sam_frames=args.sam_frames)
    prefetch = not args.no_prefetch and args.batches == "fresh"
    sam_prefetch = not args.no_sam_prefetch
    sam_pf_param = None
    if full:
        lay = model.model.layers[min(args.sam_prefetch_layer, len(model.model.layers) - 1)].self_attn.q_proj
        sam_pf_param = next((p_ for p_ in lay.parameters() if p_.requires_grad), None)      # its LoRA factor: the gradient arrives when that layer's backward is done
    model.reuse_host_plan(args.batches == "repeat")

    def step(sync=True, keep=None):
        reducer.begin_step()
        for mi in range(accum):   # gradient accumulation: gradients are exchanged once per optimizer step (DDP no_sync)
            reducer.begin_micro_step()
            cur = feed.next()
            pf = prefetch and feed.mode == "fresh"
            if pf and full:      # the next sample's pixels are announced; the model launches its frozen ViT on a side stream where this step's mask path begins
                model.prefetch_next(**feed.peek_pixels())
            out = model(**cur)
            loss = out["loss"] if isinstance(out, dict) else out.loss
            if keep is not None:    # --dump-outputs: what this step hands its caller (the last micro-step's outputs)
                items = out.items() if isinstance(out, dict) else (("loss", out.loss), ("logits", out.logits))
                keep.update((k, v.detach()) for k, v in items if isinstance(v, torch.Tensor))
            if pf and not full:  # no mask path in this mode: behind the forward, beside the backward / optimizer
                model.prefetch_vision(**feed.peek_pixels())
            if pf and sam_prefetch and full and mi + 1 == accum:
                # the next sample's FROZEN SAM2 encoder goes out on a side stream when the backward has `sam_pf_layer` decoder layers left: its bandwidth-bound first
                # stages run beside the last dX products, its matrix-bound stage 3 beside the HBM-bound optimizer, the rest beside the next forward's products
                model.prefetch_sam(feed.peek_sam(), after=sam_pf_param)
            if mi + 1 < accum or not sync:
                with reducer.no_sync():
                    (loss / accum).backward()
            else:
                (loss / accum).backward()
        if sync:
            reducer.finish()
        else:
            with reducer.no_sync():
                reducer.finish()
        opt.step(reducer.grad_view, reducer.flat_grads())
        losses.append(loss.detach())
        return loss

    if args.refine and world == 1:
        refine_tilings(step, reps=3, within=1.5)
    for _ in range(args.warmup):
        step()
    barrier()
    del losses[:]
    last = {} if args.dump_outputs else None
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(keep=last if i == args.steps - 1 else None)
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and last is not None:      # the step's outputs and the trainable weights its optimizer step left (before any untimed step below moves them)
        dump_outputs(args, {"train_" + k: v for k, v in last.items()})
        per = min(16384, (4 << 20) // len(trainables))
        dump_outputs(args, {"train_trainable_params": torch.cat([_sample(p_, per).reshape(-1).float() for p_ in trainables])}, cap=4 << 20)
    lv = torch.stack([l.float().reshape(()) for l in losses]).cpu()
    assert torch.isfinite(lv).all(), "non-finite loss"
    if rank == 0 and os.environ.get("RGA3_BENCH_ATEN_CENSUS"):
        # measurement aid (tools/gpu_r6.sh atencensus): the framework kernels (everything that is not rga3::) inside steady-state steps, with the aten op and shapes that launch them
        from collections import defaultdict
        N = 3
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA, torch.profiler.ProfilerActivity.CPU], record_shapes=True) as prof:
            for _ in range(N):
                step()
            torch.cuda.synchronize()
        kk = defaultdict(lambda: [0, 0.0])
        for e in prof.events():
            if e.device_type == torch.autograd.DeviceType.CUDA:
                kk[e.name][0] += 1
                kk[e.name][1] += e.device_time if hasattr(e, "device_time") else e.cuda_time
        fw = {n: v for n, v in kk.items() if "rga3::" not in n}
        with open(os.environ["RGA3_BENCH_ATEN_CENSUS"], "w") as fcen:
            fcen.write(f"all kernels {sum(v[1] for v in kk.values()) / N:.0f} us per step; non-rga3 {sum(v[1] for v in fw.values()) / N:.0f} us per step in {sum(v[0] for v in fw.values()) / N:.1f} launches\n")
            for n, v in sorted(fw.items(), key=lambda kv: -kv[1][1])[:30]:
                fcen.write(f"  {v[1] / N:8.1f} us  {v[0] / N:5.1f} x  {n[:150]}\n")
            ops_ = defaultdict(lambda: [0.0, 0])
            for e in prof.key_averages(group_by_input_shape=True):
                if e.key.startswith("aten::") and (getattr(e, "device_time_total", 0) or getattr(e, "cuda_time_total", 0)):
                    ent = ops_[(e.key, str(e.input_shapes)[:110])]
                    ent[0] += (getattr(e, "self_device_time_total", None) or getattr(e, "self_cuda_time_total", 0)) / N
                    ent[1] += e.count / N
            for (n, sh), (t, c) in sorted(ops_.items(), key=lambda kv: -kv[1][0])[:40]:
                if t > 2:
                    fcen.write(f"  op {t:8.1f} us {c:6.1f} x  {n:28s} {sh}\n")
    ms = elapsed / args.steps * 1e3
    value = world * accum / (elapsed / args.steps)

    # ---- communication report (N > 1): step time without the exchange, stand-alone bus bandwidth of the buckets
    comm = None
    if world > 1 and args.full:
        barrier()
        t0 = time.perf_counter()
        for _ in range(max(3, args.steps // 2)):
            step(sync=False)
        barrier()
        local_ms = (time.perf_counter() - t0) / max(3, args.steps // 2) * 1e3
        nbytes = sum(f.numel() * f.element_size() for f in reducer.flat)
        barrier()
        t0 = time.perf_counter()
        for _ in range(3):
            for f in reducer.flat:
                dist.all_reduce(f)
        barrier()
        ar_s = (time.perf_counter() - t0) / 3
        tt = torch.tensor([local_ms, ar_s], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        local_ms, ar_s = float(tt[0]), float(tt[1])
        # what the communicator itself saw: a device-side all-reduce of ones (= the number of ranks RCCL connected), one id per rank gathered through it, and
        # the library version -- so a SCALE record shows that the collective really ran over N ranks
        cdev = dev if dist.get_backend() == "nccl" else torch.device("cpu")     # (gloo -- functional runs only -- gathers on the host)
        ones = torch.ones(1, device=cdev, dtype=torch.float32)
        dist.all_reduce(ones)
        ranks_seen = torch.empty(world, dtype=torch.int64, device=cdev)
        dist.all_gather_into_tensor(ranks_seen, torch.tensor([rank], dtype=torch.int64, device=cdev))
        try:
            ccl_version = ".".join(str(v) for v in torch.cuda.nccl.version()) if dist.get_backend() == "nccl" else None
        except Exception:   # noqa: BLE001
            ccl_version = None
        comm = {"backend": dist.get_backend(), "rccl_version": ccl_version, "communicator_ranks_by_device_allreduce": int(round(float(ones.item()))),
                "ranks_gathered": [int(v) for v in ranks_seen.tolist()], "world_size": dist.get_world_size(),
                "dense_bucket_bytes_per_step": nbytes, "sparse_rows_bytes_per_step": reducer.sparse_bytes_last, "buckets": len(reducer.flat),
                "allreduce_standalone_ms": round(ar_s * 1e3, 3), "bus_GB_per_s": round(2 * (world - 1) / world * nbytes / ar_s / 1e9, 1),
                "step_ms_without_exchange": round(local_ms, 3), "exposed_comm_ms": round(ms - local_ms, 3),
                "xgmi_peak_GB_per_s_per_gpu": 7 * 153}

    # a plain run, and profiling runs: nothing after the timed steps (the instrumented pass and the variants would end the trace)
    timed_only = bool(os.environ.get("RGA3_BENCH_TIMED_ONLY")) or not args.full
    # ---- GEMM-family instrumented pass over the same step (rank 0)
    roof_tr = None
    if rank == 0 and world == 1 and not timed_only:
        pf_saved, prefetch = prefetch, False      # the per-launch GEMM timings are taken without the side-stream ViT running beside them (events would time the overlap)
        with GemmTimer(ops) as gt:
            for _ in range(max(2, args.steps // 2)):
                step()
            tot_ms = gt.total_ms()
        prefetch = pf_saved
        nst = max(2, args.steps // 2)
        g_ms = tot_ms / nst
        fams = gt.families(nst)
        # the family's peak is the FLOP-weighted mix of its launches' peaks (an e4m3 launch is priced against 5 PF, a bf16 one against 2.5 PF): with bf16 only
        # this is the plain bf16 fraction; VERDICT r3 weak 6: the fp8 step's family was divided by the bf16 peak
        peak_mix = gt.flops / sum(slot[1] / (PEAK_BF16 * (2.0 if k_ == "fp8" else 1.0)) for k_, slot in gt.by_kind.items()) if gt.flops > 0 else PEAK_BF16
        roof_tr = {"launches_per_step": len(gt.ev) // nst, "gemm_ms_per_step": round(g_ms, 3), "gemm_flops_per_step": gt.flops / nst,
                   "achieved": round(gt.flops / nst / (g_ms * 1e-3) / 1e12, 1), "peak": round(peak_mix / 1e12, 1), "frac": round(gt.flops / nst / (g_ms * 1e-3) / peak_mix, 4),
                   "by_arithmetic": fams,
                   "note": "all GEMM-family launches of the training step (NT, TN weight-gradient, split-K, e4m3), FLOPs = sum of 2*M*N*K of the launched shapes; "
                           "peak = FLOP-weighted harmonic mix of the launches' dense MFMA peaks (bf16 2.5 PF, e4m3 5 PF)"}
    if rank == 0:
        assert ops.gemm_stream_k_timeouts() == 0, "stream-K hand-off timed out: results of this run are not trustworthy"
    n_train = sum(p.numel() for p in trainables)
    rows_updated = int(sum(int(m.sum()) for m in getattr(opt, "_row_mask", {}).values())) or None

    # ---- what the two exact shortcuts of the measurement are worth: the same step (a) on ONE repeated batch with the host plan reused,
    # (b) on fresh batches with every embedding row marked "has gradient history" -- where the row-masked AdamW ends up after long training
    variants = None
    if world == 1 and rank == 0 and not timed_only:
        nv = max(3, args.steps // 2)

        def timed():
            step()
            barrier()
            t0 = time.perf_counter()
            for _ in range(nv):
                step()
            barrier()
            return round((time.perf_counter() - t0) / nv * 1e3, 3)

        variants = {"steps_each": nv}
        if prefetch:      # the same fresh-batch step with the next sample's frozen ViT computed inside its own forward instead of one step ahead on a side stream
            prefetch = False
            variants["fresh_batch_no_vision_prefetch_ms"] = timed()      # (neither tower ahead of time)
            prefetch = True
            if sam_prefetch and full:   # ... and with only the SAM2 image encoder computed in line (the ViT still one step ahead)
                sam_prefetch = False
                variants["fresh_batch_no_sam_prefetch_ms"] = timed()
                sam_prefetch = True
        if args.batches == "fresh":
            feed.mode = "repeat"
            model.reuse_host_plan(True)
            variants["repeat_batch_ms"] = timed()
            feed.mode = "fresh"
            model.reuse_host_plan(False)
        if getattr(opt, "_row_mask", None):
            for m in opt._row_mask.values():
                m.fill_(1)
            variants["fresh_batch_all_embed_rows_touched_ms"] = timed()
        del losses[:]

    if rank == 0 and args.mode == "lora_fp8":
        fl = accum * (21.6 + 62.6 - 4.6 + 57.9) * 1e12   # ViT fwd + LLM fwd (labelled-row LM head) + dX at S = 4160; activations are kept, nothing is recomputed
        peak = PEAK_BF16 if args.no_fp8 else 2 * PEAK_BF16
        line = {"metric": "video-QA samples/sec (fwd+bwd) at 7B/32-frame -- LoRA fine-tune step, grad-accum %d, %s GEMMs for the frozen decoder weights" % (
                    accum, "bf16" if args.no_fp8 else "fp8 e4m3"), "value": round(value, 4), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "bf16" if args.no_fp8 else "fp8(e4m3)+bf16", "data": "synthetic",
                "config": {"workload": "BASELINE.json configs[4] per GPU: Qwen2.5-VL-7B, 32 frames 448x448 (grid [16,32,32], S = 4160), ViT fwd (frozen) and decoder "
                                       "fwd (activations kept in HBM) + bwd with the frozen qkv / o / proj / gate-up / down contractions in e4m3 (per-token / per-row scales), "
                                       "LoRA r128 (dropout 0.05) + lm_head + embed_tokens + norms + attention in bf16, %d micro-steps per optimizer step, "
                                       "one bucketed RCCL all-reduce per optimizer step, AdamW" % accum,
                           "per_gpu_batch": 1, "grad_accum": accum, "seq_len": 4160, "parallelism": f"dp{world}", "trainable_params": n_train,
                           "approx_flops_per_step": fl, "batches": args.batches, "adamw_embed_rows_updated": rows_updated, "variants": variants},
                "roofline": {"bound": "mfma", "achieved": round(fl / (ms * 1e-3) / 1e12, 1), "peak": peak / 1e12, "unit": "TFLOP/s", "frac": round(fl / (ms * 1e-3) / peak, 4),
                             "traffic": None, "gemm_family": roof_tr, "note": "whole-step algorithmic FLOPs / step time against the dense fp8 (5 PF) or bf16 (2.5 PF) MFMA peak"},
                "loss_first_last": [round(float(lv[0]), 5), round(float(lv[-1]), 5)], "comm": comm,
                "cpu_baseline": None if (not args.full or args.no_cpu_baseline or world > 1) else cpu_baseline(train=True, sam_frames=0, seq=4160, grid_t=16, micro_steps=accum)}
        _put_traffic(line["roofline"], "lora_fp8", "gemm")
        print(json.dumps(line), flush=True)
    elif rank == 0:
        fl = train_flops(args.sam_frames) if full else (10.8 + 30.8 - 2.3 + 28.5) * 1e12
        rfb = {"bound": "mfma", "achieved": round(fl / (ms * 1e-3) / 1e12, 1), "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s", "frac": round(fl / (ms * 1e-3) / PEAK_BF16, 4),
               "traffic": None, "flops_per_step": fl, "gemm_family": roof_tr, "note": "whole-step algorithmic FLOPs (SURVEY.md 8(d); activations kept, nothing recomputed) / step time"}
        _put_traffic(rfb, "train_full")
        cpu = None
        if full and world == 1 and args.full and not args.no_cpu_baseline:
            cpu = cpu_baseline(train=True, sam_frames=args.sam_frames)
        line = {"metric": ("video-QA samples/sec (fwd+bwd) at 7B/16-frame — full RGA3 training step (Qwen2.5-VL-7B + SAM2-L + mask losses + AdamW)" if full
                           else "video-QA samples/sec (fwd+bwd) at 7B/16-frame — LLM-side LoRA training step (no SAM2 mask path)"), "value": round(value, 4),
                "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                "config": {"workload": ("BASELINE.json configs[2] per GPU: " if full else "") +
                                       "Qwen2.5-VL-7B ViT fwd (frozen) + decoder fwd+bwd (layer activations kept in HBM, no recompute), LoRA r128 (alpha 256, dropout 0.05) q/v + lm_head + embed_tokens "
                                       "trainable, AdamW step (weight decay 0 as in the reference; embed_tokens rows that never received a gradient -- g = m = v = 0, exactly unchanged by "
                                       "AdamW -- are not streamed), bucketed RCCL all-reduce (embed_tokens rows exchanged sparsely); 16 frames 448x448, S=2112, 1 sample/GPU" +
                                       (f"; SAM2-L on {args.sam_frames} frames 1024x1024 (frozen encoder, trainable mask decoder + text_hidden_fcs, BCE+dice)" if full else "") +
                                       ("; the FROZEN towers of the NEXT sample (ViT, SAM2 image encoder) are launched one step ahead on side streams -- every step runs exactly one pass of "
                                        "each, same kernels, same values (config.variants times the step without them)" if prefetch else ""),
                           "per_gpu_batch": 1, "seq_len": 2112, "parallelism": f"dp{world}", "trainable_params": n_train, "flops_per_sample": fl,
                           "batches": args.batches, "vision_prefetch": bool(prefetch), "sam_encoder_prefetch": bool(prefetch and sam_prefetch and full), "adamw_embed_rows_updated": rows_updated, "variants": variants},
                "roofline": fwd_roof if fwd_roof is not None else rfb, "roofline_fwd_bwd": rfb,
                "verify": dict(fwd_verify or {}, loss_first_last=[round(float(lv[0]), 5), round(float(lv[-1]), 5)]),
                "comm": comm, "cpu_baseline": cpu}
        print(json.dumps(line), flush=True)
    if rank == 0 and os.environ.get("RGA3_TUNE_SAVE"):   # decisions of this run, for rocprofv3 --pmc passes without trial launches (RGA3_TUNE_LOAD)
        from rga3.hip import tuner
        tuner.save(os.environ["RGA3_TUNE_SAVE"])
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
