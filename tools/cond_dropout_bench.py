#!/usr/bin/env python
"""What text-conditioning dropout (`Trainer(cond_dropout=p)`, hdmoe_text_dropout) costs, at the bench size of BASELINE config 2:

1. the kernel on (256, 77, 768) fp32 text at p = 0.1 against the `torch.Tensor.copy_` between the same two buffers that it replaces in the
   graphed step -- one process, alternating rounds, each round `--launches` back-to-back launches between two device events;
2. `Trainer(graphed=True)` ms/step with `cond_dropout` = p and = 0 (and, once, the eager device-input trainer), every leg a child process
   of tools/trainer_loop_bench.py, the two settings alternating.

    python tools/cond_dropout_bench.py [--p 0.1] [--rounds 3] [--out profiles/r11_cond_dropout.json]

A difference counts when it exceeds the spread (max - min) of the side it is compared with."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def summary(us):
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2), spread_us=round(max(us) - min(us), 2),
                rounds_us=[round(v, 2) for v in us])


def kernel_leg(args):
    import torch
    from hdmoe_hip import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    text = torch.randn(args.batch, 77, 768, device=dev, generator=g)
    null = torch.randn(77, 768, device=dev, generator=g)
    out, keep = torch.empty_like(text), torch.empty(args.batch, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.launches):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.launches

    drop = lambda i: ops.text_dropout(out, keep, text, null, 99, i, args.p)
    copy = lambda i: out.copy_(text)
    for fn in (drop, copy):                                     # code objects loaded, clocks up
        timed(fn)
    k_us, c_us, kept = [], [], []
    for r in range(args.kernel_rounds):
        k_us.append(timed(drop))
        kept.append(float(keep.mean()))
        c_us.append(timed(copy))
    nbytes = text.numel() * 4
    res = dict(shape=list(text.shape), dtype="float32", p=args.p, launches_per_round=args.launches, rounds=args.kernel_rounds,
               text_dropout=summary(k_us), copy_=summary(c_us), kept_share_last_step_of_round=round(statistics.mean(kept), 4))
    res["text_dropout"]["bytes_moved"] = int(nbytes * (1 + statistics.mean(kept))) + null.numel() * 4
    res["copy_"]["bytes_moved"] = 2 * nbytes
    for k in ("text_dropout", "copy_"):
        res[k]["tb_per_s"] = round(res[k]["bytes_moved"] / res[k]["median_us"] * 1e-6, 3)
    res["kernel_minus_copy_us"] = round(res["text_dropout"]["median_us"] - res["copy_"]["median_us"], 2)
    res["within_copy_spread"] = res["kernel_minus_copy_us"] <= res["copy_"]["spread_us"]
    return res


def trainer_leg(mode, p, args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trainer_loop_bench.py"), "--leg", mode, "--steps", str(args.steps), "--blocks",
                          str(args.blocks), "--warmup", str(args.warmup), "--batch", str(args.batch), "--cond-dropout", str(p)], check=True,
                         capture_output=True, text=True, timeout=420).stdout
    leg = json.loads([l for l in out.splitlines() if l.startswith("LEG ")][-1][4:])
    print(f"[cond_dropout_bench] {mode} p={p}: {leg['ms_per_step']} ms/step {leg['blocks_ms_per_step']}", file=sys.stderr, flush=True)
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--kernel-rounds", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the graphed trainer legs")
    ap.add_argument("--eager-rounds", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_cond_dropout.json"))
    ap.add_argument("--kernel-leg", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernel_leg:
        print("LEG " + json.dumps(kernel_leg(args)), flush=True)
        return
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-leg", "--p", str(args.p), "--batch", str(args.batch), "--launches",
                          str(args.launches), "--kernel-rounds", str(args.kernel_rounds)], check=True, capture_output=True, text=True, timeout=300).stdout
    res = {"kernel_vs_copy": json.loads([l for l in out.splitlines() if l.startswith("LEG ")][-1][4:])}
    print(f"[cond_dropout_bench] kernel {res['kernel_vs_copy']['text_dropout']} copy_ {res['kernel_vs_copy']['copy_']}", file=sys.stderr, flush=True)
    for mode, rounds in (("graphed", args.rounds), ("eager_device_inputs", args.eager_rounds)):
        legs = {"off": [], "on": []}
        for _ in range(rounds):
            legs["off"].append(trainer_leg(mode, 0.0, args))
            legs["on"].append(trainer_leg(mode, args.p, args))
        if rounds:
            ms = {k: [l["ms_per_step"] for l in v] for k, v in legs.items()}
            res[mode] = dict(cond_dropout=args.p, ms_per_step_off=ms["off"], ms_per_step_on=ms["on"],
                             median_off=round(statistics.median(ms["off"]), 3), median_on=round(statistics.median(ms["on"]), 3),
                             spread_off=round(max(ms["off"]) - min(ms["off"]), 3), blocks_off=[l["blocks_ms_per_step"] for l in legs["off"]],
                             blocks_on=[l["blocks_ms_per_step"] for l in legs["on"]], batch=legs["on"][0]["batch"],
                             final_loss_on=legs["on"][-1]["final_loss"], final_loss_off=legs["off"][-1]["final_loss"])
            res[mode]["on_minus_off_ms"] = round(res[mode]["median_on"] - res[mode]["median_off"], 3)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
