"""Decode-step rate of generate() at 7B dims (random weights): prefill S = 2112 (16 frames), then N new tokens.
python tools/generate_probe.py [N] [--decode-weights bf16|e4m3] [--decode-attn varlen|cache] [--batch B] [--repetition-penalty P] [--top-k K] [--top-p P] [--sample]
--batch B repeats the bench sample B times along the batch; the third line's ms/token is per step (all B sequences), ms/token/seq divides it by B.
--repetition-penalty / --top-k / --top-p / --sample go to generate() as given (a penalty != 1, or --sample with a top-k, picks tokens with ops.select_token; --sample draws
with seed 0); without them the call is the plain greedy one."""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "rga3-release_amd"))
import bench
args = sys.argv[1:]


def opt(name, default):
    if name not in args:
        return default
    i = args.index(name)
    v = args[i + 1]
    del args[i:i + 2]
    return v


kind = opt("--decode-weights", "bf16")
attn = opt("--decode-attn", "varlen")
B = int(opt("--batch", "1"))
sel = {}
for name, key, conv in (("--repetition-penalty", "repetition_penalty", float), ("--top-k", "top_k", int), ("--top-p", "top_p", float)):
    v = opt(name, None)
    if v is not None:
        sel[key] = conv(v)
if "--sample" in args:
    args.remove("--sample")
    sel.update(do_sample=True, seed=0)
sel.setdefault("do_sample", False)
N = int(args[0]) if args else 64
dev = torch.device("cuda:0")
model, cfg = bench.build_model(dev)
inputs = bench.make_inputs(cfg, dev)
if B > 1:
    inputs = dict(input_ids=inputs["input_ids"].repeat(B, 1), attention_mask=inputs["attention_mask"].repeat(B, 1),
                  pixel_values_videos=inputs["pixel_values_videos"].repeat(B, 1), video_grid_thw=inputs["video_grid_thw"].repeat(B, 1),
                  second_per_grid_ts=inputs["second_per_grid_ts"].repeat(B))
if kind != "bf16":
    model.set_decode_weights(kind)
    print(f"decode weights: {model.decode_weights}", flush=True)
if attn != "varlen":
    model.set_decode_attention(attn)
if attn != "varlen" or B > 1:
    print(f"decode attention: {model.decode_attention}; batch {B}", flush=True)
if len(sel) > 1:
    print("token selection: " + ", ".join(f"{k}={v}" for k, v in sorted(sel.items())), flush=True)
with torch.no_grad():
    for n in (8, N, N):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = model.generate(**inputs, max_new_tokens=1, eos_token_id=-1, **sel)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        out = model.generate(**inputs, max_new_tokens=n + 1, eos_token_id=-1, **sel)    # (no EOS: random weights cannot end a run early)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        per = ((t2 - t1) - (t1 - t0)) * 1e3 / n
        print(f"prefill+1: {(t1-t0)*1e3:.1f} ms; {n} more tokens: {per:.2f} ms/token" + (f" ({per / B:.2f} ms/token/seq)" if B > 1 else "")
              + f"; out {tuple(out.shape)}", flush=True)
