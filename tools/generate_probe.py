"""Decode-step rate of generate() at 7B dims (random weights): prefill S = 2112 (16 frames), then N new tokens.
python tools/generate_probe.py [N] [--decode-weights bf16|e4m3]"""
import os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "rga3-release_amd"))
import bench
args = sys.argv[1:]
kind = "bf16"
if "--decode-weights" in args:
    i = args.index("--decode-weights")
    kind = args[i + 1]
    del args[i:i + 2]
N = int(args[0]) if args else 64
dev = torch.device("cuda:0")
model, cfg = bench.build_model(dev)
inputs = bench.make_inputs(cfg, dev)
if kind != "bf16":
    model.set_decode_weights(kind)
    print(f"decode weights: {model.decode_weights}", flush=True)
with torch.no_grad():
    for n in (8, N, N):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = model.generate(**inputs, max_new_tokens=1, do_sample=False, eos_token_id=-1)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        out = model.generate(**inputs, max_new_tokens=n + 1, do_sample=False, eos_token_id=-1)    # (no EOS: random weights cannot end a run early)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        print(f"prefill+1: {(t1-t0)*1e3:.1f} ms; {n} more tokens: {((t2-t1)-(t1-t0))*1e3/n:.2f} ms/token; out {tuple(out.shape)}", flush=True)
