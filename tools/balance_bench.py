#!/usr/bin/env python
"""What the routers' selection bias (`Trainer(balance_rate=r)`, hdmoe_router_head_bias_fwd + hdmoe_balance_bias_update) costs, at the
bench size of BASELINE config 2:

1. the head with a bias and with the accumulators against the plain head on (256, 4) logits, k = 2, with noise and mask, and the update
   launch alone -- one process, alternating rounds, each round `--launches` back-to-back launches between two device events;
2. `Trainer(graphed=True)` ms/step with the feature on and off, every leg a child process of tools/trainer_loop_bench.py, the settings
   alternating; with `--parent-tree DIR` (a built checkout of the parent commit) the parent's graphed step joins the alternation, run by
   the parent's own tools/trainer_loop_bench.py.

    python tools/balance_bench.py [--rate 0.001] [--rounds 3] [--parent-tree DIR] [--out profiles/r16_router_balance.json]

The design adds no launch to the forward (the head is replaced) and two small launches per step behind the optimizer (one per router).  A
difference counts when it exceeds the spread (max - min) of the side it is compared with."""
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
    B, E, k = args.batch, 4, 2
    logits = torch.randn(B, E, device=dev, generator=g)
    noise = 0.1 * torch.randn(B, E, device=dev, generator=g)
    mask = (torch.rand(B, E, device=dev, generator=g) < 0.8).float()
    mask[:, 0] = 1.0
    bias = torch.tensor([0.05, -0.05, 0.02, -0.02], device=dev)
    load, target = torch.zeros(E, dtype=torch.int64, device=dev), torch.zeros(E, dtype=torch.int64, device=dev)
    ll, lt = torch.zeros_like(load), torch.zeros_like(load)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / args.launches

    with torch.no_grad():
        legs = {"plain_head": lambda: ops.router_head(logits, noise, mask, k),
                "bias_head": lambda: ops.router_head(logits, noise, mask, k, sel_bias=bias),
                "bias_head_counting": lambda: ops.router_head(logits, noise, mask, k, sel_bias=bias, accum=(load, target)),
                "bias_update": lambda: ops.balance_bias_update(bias, load, target, ll, lt, None, args.rate, 8.0)}
        for fn in legs.values():                                # code objects loaded, clocks up
            timed(fn)
        us = {name: [] for name in legs}
        for _ in range(args.kernel_rounds):
            for name, fn in legs.items():
                us[name].append(timed(fn))
        # the same launches as they run in the captured step: `--launches` of them in one graph, replayed -- no host work between them
        graphs = {}
        for name, fn in legs.items():
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                for _ in range(args.launches):
                    fn()
        torch.cuda.synchronize()

        def replayed(gr):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            return 1e3 * e0.elapsed_time(e1) / args.launches

        for gr in graphs.values():
            replayed(gr)
        rus = {name: [] for name in legs}
        for _ in range(args.kernel_rounds):
            for name, gr in graphs.items():
                rus[name].append(replayed(gr))
    res = dict(shape=[B, E], k=k, launches_per_round=args.launches, rounds=args.kernel_rounds,
               note="eager: back-to-back launches of a few-microsecond kernel from Python, the figure is the host's launch rate (four "
                    "output allocations per head call included); graph_replay: the same chain of dependent launches inside one graph, "
                    "per launch -- what the captured step pays",
               **{name: summary(v) for name, v in us.items()}, graph_replay={name: summary(v) for name, v in rus.items()})
    res["graph_replay"]["bias_head_counting_minus_plain_us"] = round(res["graph_replay"]["bias_head_counting"]["median_us"]
                                                                       - res["graph_replay"]["plain_head"]["median_us"], 2)
    res["bias_head_counting_minus_plain_us"] = round(res["bias_head_counting"]["median_us"] - res["plain_head"]["median_us"], 2)
    res["within_plain_spread"] = res["bias_head_counting_minus_plain_us"] <= res["plain_head"]["spread_us"]
    return res


def trainer_leg(tree, rate, args):
    cmd = [sys.executable, os.path.join(tree, "tools", "trainer_loop_bench.py"), "--leg", "graphed", "--steps", str(args.steps), "--blocks",
           str(args.blocks), "--warmup", str(args.warmup), "--batch", str(args.batch)]
    if rate > 0:
        cmd += ["--balance-rate", str(rate)]
    out = subprocess.run(cmd, cwd=tree, check=True, capture_output=True, text=True, timeout=420).stdout
    leg = json.loads([l for l in out.splitlines() if l.startswith("LEG ")][-1][4:])
    print(f"[balance_bench] {tree} rate={rate}: {leg['ms_per_step']} ms/step {leg['blocks_ms_per_step']}", file=sys.stderr, flush=True)
    return leg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, default=0.001)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--kernel-rounds", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the graphed trainer legs")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: its graphed step joins the alternation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_router_balance.json"))
    ap.add_argument("--kernel-leg", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernel_leg:
        print("LEG " + json.dumps(kernel_leg(args)), flush=True)
        return
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-leg", "--rate", str(args.rate), "--batch", str(args.batch), "--launches",
                          str(args.launches), "--kernel-rounds", str(args.kernel_rounds)], check=True, capture_output=True, text=True, timeout=300).stdout
    res = {"kernels": json.loads([l for l in out.splitlines() if l.startswith("LEG ")][-1][4:])}
    print(f"[balance_bench] kernels {json.dumps({k: v['median_us'] for k, v in res['kernels'].items() if isinstance(v, dict) and 'median_us' in v})} "
          f"graph replay {json.dumps({k: v['median_us'] for k, v in res['kernels']['graph_replay'].items() if isinstance(v, dict)})}",
          file=sys.stderr, flush=True)
    sides = [("off", ROOT, 0.0), ("on", ROOT, args.rate)]
    if args.parent_tree:
        sides.insert(0, ("parent", os.path.abspath(args.parent_tree), 0.0))
    legs = {name: [] for name, _, _ in sides}
    for _ in range(args.rounds):
        for name, tree, rate in sides:
            legs[name].append(trainer_leg(tree, rate, args))
    ms = {k: [l["ms_per_step"] for l in v] for k, v in legs.items()}
    g = dict(workload="BASELINE config 2 (model_config1, 4 experts top-2, 4x32x32 latents), bf16, Trainer(graphed=True).train_step",
             timing=f"median over {args.blocks} blocks of {args.steps} steps per leg, every leg a process of its own, sides alternating",
             balance_rate=args.rate, batch=legs["on"][0]["batch"])
    for name in legs:
        g[f"ms_per_step_{name}"] = ms[name]
        g[f"median_{name}"] = round(statistics.median(ms[name]), 3)
        g[f"spread_{name}"] = round(max(ms[name]) - min(ms[name]), 3)
        g[f"blocks_{name}"] = [l["blocks_ms_per_step"] for l in legs[name]]
        g[f"final_loss_{name}"] = legs[name][-1]["final_loss"]
    g["on_minus_off_ms"] = round(g["median_on"] - g["median_off"], 3)
    g["on_over_off"] = round(g["median_on"] / g["median_off"], 4)
    if "parent" in legs:
        g["on_minus_parent_ms"] = round(g["median_on"] - g["median_parent"], 3)
        g["on_over_parent"] = round(g["median_on"] / g["median_parent"], 4)
        g["off_over_parent"] = round(g["median_off"] / g["median_parent"], 4)
    res["graphed"] = g
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
