#!/usr/bin/env python
"""Cost of the gradient-health pass and of the guarded update, on the parameter table of the BASELINE configs[1] model, one GPU.

    python tools/health_bench.py [--parent-tree DIR] [--out profiles/r15_health.json]

Four legs alternate in one process, each replayed from a captured single-stream graph (so that none pays host launch time), device events
around windows of --replays replays, --rounds windows per leg after 20 warm-up replays; the figures are the median and the range of the
windows:
  sumsq     hdmoe_mt_sumsq over every gradient                                        4 N bytes
  stats     hdmoe_mt_stats over every gradient (GradHealth.measure, with the verdict) 4 N bytes: the yardstick is `sumsq` in the same run
  update    the unguarded update side: sumsq + clip + AdamW, then the EMA (2 profiles)
  guarded   the guarded update side: stats + clip + AdamW behind the verdict, then the EMA behind the verdict
The update sides move 4 N (norm pass) + 28 N_opt (g read; p, m, v read and written) + 20 N (EMA: p read, 2 profiles read and written).
With --parent-tree (a built checkout of the parent commit) the `update` leg also runs in child processes that import that tree's package,
alternating with children of this tree (the first pair is a warm-up and is dropped): the unguarded side is the same code and has to sit
inside the parent's run-to-run range.
Last, `Trainer(graphed=True)`'s step with the guard off and on, by tools/trainer_loop_bench.py's method (child processes, alternating)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def setup(tree):
    for p in (os.path.join(tree, "heterogeneous-moe-for-diffusion-models_amd"), tree):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("health_bench needs a GPU: a CPU run measures nothing")
    from Utils import configs, training
    from hdmoe_hip.ema import WeightEMA
    from models import model_config1, model_config2
    bc = configs.BASELINE_CONFIGS[1]
    cls = (model_config1 if bc["module"] == 1 else model_config2).preconditioned_HDMOEM
    torch.manual_seed(0)
    model = cls(**configs.model_kwargs(**bc["over"])).to("cuda")
    params = list(model.parameters())
    gen = torch.Generator(device="cuda").manual_seed(1)
    for p in params:
        p.grad = 1e-3 * torch.randn(p.shape, device="cuda", generator=gen)
    opt = training.build_optimizer(model, configs.optim_configs)
    ema = WeightEMA(model, sigma_rels=(0.05, 0.10))
    return torch, model, params, opt, ema


def windows(torch, legs, replays, rounds):
    """{leg: [us per call per window]}: every leg captured once, then the legs alternate window by window."""
    graphs = {}
    for name, fn in legs.items():
        fn()                                                    # builds the tables (host work, outside the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                               # one stream, no parallel branches
            fn()
        for _ in range(20):
            g.replay()
        torch.cuda.synchronize()
        graphs[name] = g
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / replays)
    return times


def summary(ts, nbytes):
    med = statistics.median(ts)
    return {"median_us": round(med, 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3), "bytes": nbytes,
            "GB_per_s": round(nbytes / (med * 1e-6) / 1e9, 1), "windows_us": [round(t, 3) for t in ts]}


def update_leg(args):
    """The unguarded update side alone, with only what the parent commit has too (a child process per tree)."""
    torch, model, params, opt, ema = setup(args.tree)

    def update():
        opt.step(clip=(params, 1.0))
        ema.update()

    ts = windows(torch, {"update": update}, args.replays, args.rounds)["update"]
    print("LEG " + json.dumps({"median_us": statistics.median(ts), "windows_us": ts}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit: the unguarded update side runs there too")
    ap.add_argument("--ab-repeats", type=int, default=5)
    ap.add_argument("--trainer-repeats", type=int, default=2)
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_health.json"))
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg == "update":
        return update_leg(args)

    torch, model, params, opt, ema = setup(ROOT)
    from hdmoe_hip._lib import call
    from hdmoe_hip.optim import GradHealth, _Table, health_groups
    names, group_of = health_groups(model)
    health = GradHealth(params, group_of, names)
    tab = _Table([(p, p.grad, None, None, 0) for p in params])
    ss = torch.empty(1, dtype=torch.float32, device="cuda")

    def update():
        opt.step(clip=(params, 1.0))
        ema.update()

    def guarded():
        health.measure(0)
        opt.step(clip=(params, 1.0), health=health)
        ema.update(ok=health.ok)

    legs = {"sumsq": lambda: call("hdmoe_mt_sumsq", ss, tab.descs, tab.chunks, tab.n, tab.ws), "stats": lambda: health.measure(0),
            "update": update, "guarded": guarded}
    times = windows(torch, legs, args.replays, args.rounds)
    assert int(health.ok.item()) == 1 and torch.equal(health.total_sumsq, ss)
    n = sum(p.numel() for p in params)
    n_opt = sum(p.numel() for g in opt.param_groups for p in g["params"])
    side = 4 * n + 28 * n_opt + ema.num_bytes_per_update()
    res = {"model": "BASELINE configs[1]", "device": torch.cuda.get_device_name(0), "tensors": len(params), "parameters": n,
           "optimised_parameters": n_opt, "chunks": tab.n, "groups": len(names), "replays_per_window": args.replays, "windows": args.rounds,
           "legs": {"sumsq": summary(times["sumsq"], 4 * n), "stats": summary(times["stats"], 4 * n),
                    "update": summary(times["update"], side), "guarded": summary(times["guarded"], side)}}
    L = res["legs"]
    res["stats_over_sumsq"] = round(L["stats"]["median_us"] / L["sumsq"]["median_us"], 4)
    res["sumsq_spread_us"] = round(L["sumsq"]["max_us"] - L["sumsq"]["min_us"], 3)
    res["stats_within_sumsq_spread"] = L["stats"]["median_us"] <= L["sumsq"]["median_us"] + res["sumsq_spread_us"]
    res["guarded_over_update"] = round(L["guarded"]["median_us"] / L["update"]["median_us"], 4)
    print(json.dumps({k: v for k, v in res.items() if k != "legs"}), flush=True)
    for k, v in L.items():
        print(k, {a: b for a, b in v.items() if a != "windows_us"}, flush=True)
    del health, opt, ema, model, params, tab
    torch.cuda.empty_cache()

    def child(cmd, tag, timeout=600):
        out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=timeout).stdout
        return json.loads([l for l in out.splitlines() if l.startswith(tag)][-1][len(tag):])

    if args.parent_tree:                                        # same code on both sides: this tree / parent, alternating
        ab = {"this_commit": [], "parent": []}
        for it in range(args.ab_repeats + 1):
            for key, tree in (("this_commit", ROOT), ("parent", os.path.abspath(args.parent_tree))):
                r = child([sys.executable, os.path.abspath(__file__), "--leg", "update", "--tree", tree, "--replays", str(args.replays),
                           "--rounds", str(args.rounds)], "LEG ")
                if it > 0:                                      # the first pair only warms the box up
                    ab[key].append(round(r["median_us"], 3))
        res["update_vs_parent"] = {k: {"runs_us": v, "median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in ab.items()}
        pa, th = res["update_vs_parent"]["parent"], res["update_vs_parent"]["this_commit"]
        res["update_vs_parent"]["not_slower_than_parent_range"] = th["median_us"] <= pa["max_us"]
        print("update_vs_parent", res["update_vs_parent"], flush=True)
    else:
        res["update_vs_parent"] = "not measured: no --parent-tree given"

    if not args.no_trainer:                                     # Trainer(graphed=True).train_step, guard off / on, alternating children
        tl = {"guard_off": [], "guard_on": []}
        for _ in range(args.trainer_repeats):
            for key, extra in (("guard_off", []), ("guard_on", ["--skip-nonfinite"])):
                r = child([sys.executable, os.path.join(HERE, "trainer_loop_bench.py"), "--leg", "graphed"] + extra, "LEG ")
                tl[key].append({"ms_per_step": r["ms_per_step"], "blocks_ms_per_step": r["blocks_ms_per_step"],
                                "host_enqueue_ms_per_step": r["host_enqueue_ms_per_step"]})
        res["trainer_graphed_step"] = {k: {"runs": v, "median_ms_per_step": statistics.median(x["ms_per_step"] for x in v),
                                           "min_block_ms": min(min(x["blocks_ms_per_step"]) for x in v),
                                           "max_block_ms": max(max(x["blocks_ms_per_step"]) for x in v)} for k, v in tl.items()}
        print("trainer_graphed_step", {k: {a: b for a, b in v.items() if a != "runs"} for k, v in res["trainer_graphed_step"].items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
