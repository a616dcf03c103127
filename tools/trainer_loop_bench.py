#!/usr/bin/env python
"""Step time of the PUBLIC training loop, `Utils.training.Trainer.train_step`, in its three forms -- eager (inputs from torch's generator),
eager with device-made inputs, and graphed (staged hipGraph replay over device-made inputs) -- on BASELINE config 2 at its bench batch
size in bf16, beside bench.py's step on the same box (this tree, and a parent tree when one is given).

    python tools/trainer_loop_bench.py [--steps 50] [--blocks 5] [--warmup 5] [--parent-tree DIR] [--out profiles/r10_trainer_graphed.json]

Each timing is the median over `--blocks` blocks of the block's ms/step (`--steps` steps, one synchronize at the end of the block); the host
time to enqueue a step is measured inside the same blocks.  The bench.py legs run first, each in a child process of its own.  What the
graphed step costs beyond bench.py's replay is the optimizer, the input generator and the two copies into the static buffers."""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def bench_leg(tree, steps, warmup, repeats):
    """bench.py's ms/step in `tree`, `repeats` child processes: (median, [every run], host enqueue ms of the median run)."""
    runs = []
    for _ in range(repeats):
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline",
                              "--no-roofline", "--no-sampler", "--no-fp32-trunk-leg"], cwd=tree, check=True, capture_output=True, text=True, timeout=420).stdout
        line = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
        host = line.get("host_enqueue_ms_per_step")
        if host is None:
            host = next((v.get("host_enqueue_ms_per_step") for v in line.values() if isinstance(v, dict) and "host_enqueue_ms_per_step" in v), None)
        runs.append((line["ms_per_step"], host))
    runs.sort(key=lambda r: r[0])
    med = runs[len(runs) // 2]
    return dict(ms_per_step=med[0], runs=[r[0] for r in runs], spread=round(runs[-1][0] - runs[0][0], 3), host_enqueue_ms_per_step=med[1])


def trainer_leg(mode, args):
    import torch
    import hdmoe_hip
    from Utils import configs, training
    from models import model_config1, model_config2
    bc = configs.BASELINE_CONFIGS[2]
    dev = torch.device("cuda", 0)
    hdmoe_hip.set_compute_dtype(torch.bfloat16 if bc["dtype"] == "bf16" else torch.float32)
    hdmoe_hip.manual_seed(4321)
    torch.manual_seed(1234)
    model = (model_config1 if bc["module"] == 1 else model_config2).preconditioned_HDMOEM(**configs.model_kwargs(**bc["over"]))
    with torch.no_grad():                                       # as bench.py: zero-inits would make the experts' output identically 0
        for n, p in model.named_parameters():
            if n.endswith("out_gain"):
                p.fill_(0.5)
            elif n.endswith("alpha_txt"):
                p.fill_(0.3)
    model = model.to(dev).train()
    mcfg = dict(configs.model_configs, **bc["over"])
    kw = {"eager": {}, "eager_device_inputs": dict(device_inputs=True, seed=99), "graphed": dict(graphed=True, seed=99)}[mode]
    if args.cond_dropout > 0:                                   # text-conditioning dropout with a random null row (tools/cond_dropout_bench.py)
        kw = dict(kw, cond_dropout=args.cond_dropout, null_text_emb=torch.randn(77, mcfg["text_emb_dim"], generator=torch.Generator().manual_seed(7)))
    if args.skip_nonfinite:                                     # the device-side non-finite guard (tools/health_bench.py)
        kw = dict(kw, skip_nonfinite=True)
    if args.balance_rate > 0:                                   # the routers' selection bias (tools/balance_bench.py)
        kw = dict(kw, balance_rate=args.balance_rate)
    tr = training.Trainer(model, mcfg, configs.optim_configs, configs.loss_configs, configs.mask_configs, configs.zeta_configs, **kw)
    B = args.batch or bc["batch"]
    g = torch.Generator(device=dev).manual_seed(1234)
    lat = 0.5 * torch.randn(B, mcfg["img_channels"], mcfg["img_resolution"], mcfg["img_resolution"], device=dev, generator=g)
    text = torch.randn(B, 77, mcfg["text_emb_dim"], device=dev, generator=g)
    for _ in range(args.warmup):
        res = tr.train_step(lat, text)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    blocks, hosts = [], []
    for _ in range(args.blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = 0.0
        for _ in range(args.steps):
            h0 = time.perf_counter()
            res = tr.train_step(lat, text)
            host += time.perf_counter() - h0
        torch.cuda.synchronize()
        blocks.append(1e3 * (time.perf_counter() - t0) / args.steps)
        hosts.append(1e3 * host / args.steps)
    gc.enable()
    loss = float(res["loss"]["loss"])
    out = dict(ms_per_step=round(statistics.median(blocks), 3), blocks_ms_per_step=[round(b, 3) for b in blocks],
               host_enqueue_ms_per_step=round(statistics.median(hosts), 3), steps_per_block=args.steps, batch=B, final_loss=round(loss, 5),
               loss_finite=loss == loss and abs(loss) != float("inf"))
    if tr.inputs is not None:                                   # the generator alone: GPU time between two events, host time of the call
        src = tr._lat if mode == "graphed" else lat
        gpu_us, host_us = [], []
        for i in range(20):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h0 = time.perf_counter()
            e0.record()
            tr.inputs.generate(src, tr.step_idx)
            e1.record()
            host_us.append(1e6 * (time.perf_counter() - h0))
            torch.cuda.synchronize()
            gpu_us.append(1e3 * e0.elapsed_time(e1))
        out["generator"] = dict(gpu_us=round(statistics.median(gpu_us), 1), host_call_us=round(statistics.median(host_us), 1), launches=2)
    if mode == "graphed":
        out["graphs"] = len(tr._staged.graphs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--bench-steps", type=int, default=50)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: bench.py runs there too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_trainer_graphed.json"))
    ap.add_argument("--cond-dropout", type=float, default=0.0, help="Trainer(cond_dropout=...) in every trainer leg")
    ap.add_argument("--skip-nonfinite", action="store_true", help="Trainer(skip_nonfinite=True) in every trainer leg")
    ap.add_argument("--balance-rate", type=float, default=0.0, help="Trainer(balance_rate=...) in every trainer leg")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)       # one trainer leg in this (child) process
    args = ap.parse_args()
    if args.steps < 50:
        ap.error("--steps must be at least 50")
    if args.leg:
        print("LEG " + json.dumps(trainer_leg(args.leg, args)), flush=True)
        return
    res = {"workload": "BASELINE config 2 (model_config1, 4 experts top-2, 4x32x32 latents), bf16, Trainer.train_step incl. clip + AdamW + scheduler",
           "timing": f"median over {args.blocks} blocks of {args.steps} steps, one synchronize per block; every leg in a process of its own"}
    res["bench_py"] = {"this_commit": bench_leg(ROOT, args.bench_steps, args.warmup, args.bench_repeats)}
    if args.parent_tree:
        res["bench_py"]["parent"] = bench_leg(os.path.abspath(args.parent_tree), args.bench_steps, args.warmup, args.bench_repeats)
    for mode in ("eager", "eager_device_inputs", "graphed"):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", mode, "--steps", str(args.steps), "--blocks", str(args.blocks),
                              "--warmup", str(args.warmup), "--batch", str(args.batch), "--cond-dropout", str(args.cond_dropout), "--balance-rate", str(args.balance_rate)] + (["--skip-nonfinite"] if args.skip_nonfinite else []), check=True, capture_output=True, text=True, timeout=420).stdout
        res[mode] = json.loads([l for l in out.splitlines() if l.startswith("LEG ")][-1][4:])
        print(f"[trainer_loop_bench] {mode}: {res[mode]['ms_per_step']} ms/step, host {res[mode]['host_enqueue_ms_per_step']} ms/step", file=sys.stderr, flush=True)
    res["graphed_over_eager"] = round(res["graphed"]["ms_per_step"] / res["eager"]["ms_per_step"], 4)
    res["graphed_minus_bench_py_ms"] = round(res["graphed"]["ms_per_step"] - res["bench_py"]["this_commit"]["ms_per_step"], 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
