#!/usr/bin/env python
"""What tiled sampling adds to a denoiser evaluation (csrc/tiles.hip; EDM_Sampler.sample(tile=...)), at BASELINE configs[4]'s latent size
R = 64: B = `--batch` latents (4, 2R, 2R) fp32 in 3 x 3 tiles of (R, R), overlap R / 2, feather window.

  (a) `ops.tile_gather` and `ops.tile_blend` against the plain-torch composition they replace: for gather, slicing plus `stack`; for
      blend, `zeros`, then T weighted slice `add_`s, then a divide by the summed weights (T + 2 launches, T + 1 passes over the output);
  (b) the two kernels' achieved bytes per second against the bytes they must move (x read once and the tile batch written; the tile
      batch read once and the latent written -- the weight tables are a few KiB);
  (c) one tiled evaluation with T = 1 (tile = the model's own size) beside the untiled one, both the captured evaluation of an
      EDM_Sampler (its "eval" stage state) on the bench model (model_config2, bf16, B = 128), replayed.

One process, the sides of a comparison alternating; each round is `--launches` consecutive calls between two device events with the
device idle before it, and a host clock around the enqueue of the same calls.  `device_us` is event time per call (launch gaps included:
where the host is the slower side it is the host's time), `host_us` the enqueue time per call.  (a) and (b) are also taken with the
`--launches` calls of a side captured as one graph and replayed ("graph_replay"), which is how the sampler's stages run them and takes
the enqueue out of the figure; the bytes per second of (b) come from there.  (a) and (b) run once per `--batch` value.

    python tools/tile_bench.py [--batch 16 128] [--rounds 20] [--launches 50] [--out profiles/sampler_tiles.json]

A difference counts where the two sides' ranges (min .. max over the rounds) are apart."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd")
for p in (PKG, os.path.join(PKG, "Utils"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def summary(us):
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2), spread_us=round(max(us) - min(us), 2),
                rounds_us=[round(v, 2) for v in us])


def timed(fn, launches):
    import torch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(launches):
        fn(i)
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches, 1e6 * (t1 - t0) / launches


def compare(sides, args):
    """{name: {device_us, host_us}} for the callables of `sides`, alternating over the rounds, after one warm-up window each."""
    for fn in sides.values():
        timed(fn, args.launches)
    dev_us, host_us = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            d, h = timed(fn, args.launches)
            dev_us[name].append(d)
            host_us[name].append(h)
    return {name: dict(device_us=summary(dev_us[name]), host_us=summary(host_us[name])) for name in sides}


def compare_replayed(sides, args):
    """{name: {device_us}}: every side's `--launches` calls captured as ONE graph and replayed, so that the device, not the enqueue, sets
    the pace: event time of a replay over the calls in it (the gaps between graph nodes included), sides alternating."""
    import torch
    graphs = {}
    for name, fn in sides.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn(0)
        torch.cuda.current_stream().wait_stream(side)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for i in range(args.launches):
                fn(i)
    for g in graphs.values():
        g.replay()
    dev_us = {k: [] for k in sides}
    for _ in range(args.rounds):
        for name, g in graphs.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            dev_us[name].append(1e3 * e0.elapsed_time(e1) / args.launches)
    return {name: dict(device_us=summary(dev_us[name])) for name in sides}


def apart(res, a, b, kinds=("device_us", "host_us")):
    out = {}
    for kind in kinds:
        x, y = res[a][kind], res[b][kind]
        out[kind + "_ranges_apart"] = x["max_us"] < y["min_us"] or y["max_us"] < x["min_us"]
        out[f"{kind}_{b}_over_{a}"] = round(y["median_us"] / x["median_us"], 2)
    return out


def kernels(args, B):
    import torch
    from hdmoe_hip import ops
    dev = torch.device("cuda", 0)
    C, R = 4, args.resolution
    plan = ops.tile_plan(2 * R, 2 * R, R, R, R // 2, "feather")
    g = torch.Generator(device=dev).manual_seed(1234)
    x = torch.randn(B, C, 2 * R, 2 * R, device=dev, generator=g)
    tiles = torch.randn(B * plan.T, C, R, R, device=dev, generator=g)
    tiles_out, out = torch.empty_like(tiles), torch.empty_like(x)
    plan.device(dev)
    origins = [(ky, kx, a, b) for ky, a in enumerate(plan.oy.tolist()) for kx, b in enumerate(plan.ox.tolist())]
    i = torch.arange(R, device=dev)
    w1 = torch.minimum(torch.minimum(i + 1, R - i), torch.tensor(R // 2, device=dev)).float() / (R // 2)      # the raw feather window
    w2 = (w1[:, None] * w1[None, :]).contiguous()
    wsum = torch.zeros(2 * R, 2 * R, device=dev)                             # static, like the plan's tables: made once, outside the timing
    for _, _, a, b in origins:
        wsum[a:a + R, b:b + R] += w2
    tv = tiles.view(B, plan.T, C, R, R)

    def gather(i):
        ops.tile_gather(x, plan, out=tiles_out)

    def gather_torch(i):
        torch.stack([x[:, :, a:a + R, b:b + R] for _, _, a, b in origins], dim=1)

    def blend(i):
        ops.tile_blend(tiles, plan, B, out=out)

    def blend_torch(i):
        acc = torch.zeros_like(x)
        for k, (_, _, a, b) in enumerate(origins):
            acc[:, :, a:a + R, b:b + R].addcmul_(tv[:, k], w2)
        return acc.div_(wsum)

    gather(0)
    same = torch.equal(tiles_out, torch.stack([x[:, :, a:a + R, b:b + R] for _, _, a, b in origins], 1).flatten(0, 1))
    blend(0)
    diff = float((out - blend_torch(0)).abs().max())
    sides = {"tile_gather": gather, "torch_gather": gather_torch, "tile_blend": blend, "torch_blend": blend_torch}
    res = compare(sides, args)
    torch.cuda.synchronize()
    res["gather"] = apart(res, "tile_gather", "torch_gather")
    res["blend"] = apart(res, "tile_blend", "torch_blend")
    rep = compare_replayed(sides, args)
    rep["gather"] = apart(rep, "tile_gather", "torch_gather", ("device_us",))
    rep["blend"] = apart(rep, "tile_blend", "torch_blend", ("device_us",))
    nb_x, nb_t = x.numel() * 4, tiles.numel() * 4
    for name in ("tile_gather", "tile_blend"):                                # (b): the bytes the pass must move over its device time
        rep[name]["bytes_moved"] = nb_x + nb_t
        rep[name]["achieved_GBps"] = round((nb_x + nb_t) / rep[name]["device_us"]["median_us"] * 1e-3, 1)
    res["graph_replay"] = rep
    res["checks"] = dict(gather_equals_slicing=bool(same), blend_max_abs_diff_to_torch=diff)
    res["shapes"] = dict(batch=B, latent=[C, 2 * R, 2 * R], tile=[R, R], overlap=R // 2, tiles=[plan.Ty, plan.Tx], window="feather",
                         latent_bytes=nb_x, tile_batch_bytes=nb_t, torch_blend="zeros, T addcmul_ on slices, div_ by the static weight sum: T + 2 launches")
    return res


def evaluation(args):
    """BASELINE configs[4]'s model (bench.py's sampler leg) behind two samplers' captured evaluations: untiled, and tiled with T = 1."""
    import torch
    import hdmoe_hip
    from Utils import configs
    from EDM_sampler import EDM_Sampler
    from models import model_config2
    dev = torch.device("cuda", 0)
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    kw = configs.model_kwargs(**configs.BASELINE_CONFIGS[4]["over"])
    R, B = kw["IN_img_resolution"], args.model_batch
    torch.manual_seed(0)
    model = model_config2.preconditioned_HDMOEM(**kw).to(dev).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("out_gain"):
                p.fill_(0.5)
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.randn(B, 4, R, R, device=dev, generator=g)
    text = torch.randn(B, 77, kw["text_emb_dim"], device=dev, generator=g)
    sides, outs = {}, {}
    with torch.no_grad():
        for name, spec in (("untiled", None), ("tiled_T1", (R, R))):
            s = EDM_Sampler(model, Guide_net=model, num_solve_steps=40, guidance=1.0, use_graph=True)
            st = s._stage_state("eval", x, *s._inputs(x, text, -1.2, 1.2, None, (spec, 0, "feather", None)))
            st["sig"].fill_(1.3)
            sides[name] = (lambda i, gr=st["g_eval"][0]: gr.replay())
            outs[name] = st
        res = compare(sides, args)
        torch.cuda.synchronize()
        same = torch.equal(outs["untiled"]["out"], outs["tiled_T1"]["out"])
    res["overhead"] = apart(res, "untiled", "tiled_T1")
    res["overhead"]["device_us_added"] = round(res["tiled_T1"]["device_us"]["median_us"] - res["untiled"]["device_us"]["median_us"], 2)
    res["same_bits"] = bool(same)
    res["model"] = "BASELINE configs[4]: model_config2 preconditioned_HDMOEM, bf16 compute, eval mode, B = %d, latents 4x%dx%d fp32" % (B, R, R)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[16, 128], help="large latents of (a) / (b), one run per value; the tile batch has 9 x as many rows")
    ap.add_argument("--resolution", type=int, default=64, help="the tile size R of (a) / (b)")
    ap.add_argument("--model-batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="skip (c), the captured evaluation of the bench model")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampler_tiles.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    res = {"note": "tools/tile_bench.py on one MI355X, one process, sides alternating; device_us is event time per call with launch gaps, "
                   "host_us the enqueue time per call.  Every figure in this file was measured by that run."}
    res["kernels"] = {}
    for B in args.batch:
        k = res["kernels"][f"B{B}"] = kernels(args, B)
        r = k["graph_replay"]
        print(f"[tile_bench] B = {B}: eager gather {k['tile_gather']['device_us']['median_us']} us (torch {k['torch_gather']['device_us']['median_us']}), "
              f"blend {k['tile_blend']['device_us']['median_us']} us (torch {k['torch_blend']['device_us']['median_us']}); replayed gather "
              f"{r['tile_gather']['device_us']['median_us']} us (torch {r['torch_gather']['device_us']['median_us']}), blend "
              f"{r['tile_blend']['device_us']['median_us']} us (torch {r['torch_blend']['device_us']['median_us']}): "
              f"{r['tile_gather']['achieved_GBps']} / {r['tile_blend']['achieved_GBps']} GB/s", file=sys.stderr, flush=True)
    if not args.no_model:
        res["evaluation"] = evaluation(args)
        e = res["evaluation"]
        print(f"[tile_bench] evaluation untiled {e['untiled']['device_us']['median_us']} us, tiled T = 1 {e['tiled_T1']['device_us']['median_us']} us",
              file=sys.stderr, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
