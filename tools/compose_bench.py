"""Dev tool: cost of ONE composed-guidance evaluation under graph replay, at the shape of bench.py's sampler leg (BASELINE configs[4]
per-GPU share: B = 128, the config's 4 x R x R float32 latents, 8 experts, bf16 compute), guidance 2.0, for K = 1 .. 4 conditions with
stripe masks and weights 1 / K:
  shared    one model.forward_composed pass (routing once, K + 1 text variants through the banks and the tail, D_c in the egress kernel);
  two_pass  K model passes + one of the guide network + ONE hdmoe_guide_compose launch;
  plain     K + 1 replays of the captured plain model() evaluation (guidance 1), what a caller looping over denoise() pays before any blend.
Each leg is the captured evaluation of its own EDM_Sampler (the "eval" stage state), replayed: no host work between the kernels.  One
process; after the warm-up replays the legs are timed interleaved, `--reps` windows of `--iters` replays each between device events, and
the median window is reported with the spread.  Also counts, from the binding's call log, the library calls of one eager evaluation.
Prints one JSON line and writes it to --out.
usage: compose_bench.py [--batch 128] [--kmax 4] [--reps 7] [--iters 5] [--out profiles/compose_eval.json]"""
import argparse
import collections
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"), os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils")]
import torch  # noqa: E402
import hdmoe_hip  # noqa: E402
from hdmoe_hip import _lib  # noqa: E402
from Utils import configs  # noqa: E402
from Utils.EDM_sampler import EDM_Sampler  # noqa: E402
from models import model_config2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--kmax", type=int, default=4)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--guidance", type=float, default=2.0)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compose_eval.json"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("needs a GPU")
B, G = args.batch, args.guidance
TP, SOFT = -1.2, 1.2
hdmoe_hip.set_compute_dtype(torch.bfloat16)
kw = configs.model_kwargs(**configs.BASELINE_CONFIGS[4]["over"])
R = kw["IN_img_resolution"]
torch.manual_seed(0)
model = model_config2.preconditioned_HDMOEM(**kw).cuda().eval()
with torch.no_grad():
    for n, p in model.named_parameters():
        if n.endswith("out_gain"):
            p.fill_(0.5)
gen = torch.Generator(device="cuda").manual_seed(7)
x = torch.randn(B, 4, R, R, device="cuda", generator=gen)
text = torch.randn(B, 77, kw["text_emb_dim"], device="cuda", generator=gen)
unc = torch.randn(B, 77, kw["text_emb_dim"], device="cuda", generator=gen)
more = torch.randn(args.kmax - 1, B, 77, kw["text_emb_dim"], device="cuda", generator=gen)


def compose_kw(K):
    masks = torch.zeros(K, R, R)
    for k in range(K):                                              # K vertical stripes, weight 1 / K each
        masks[k, :, k * R // K:(k + 1) * R // K] = 1.0
    return dict(compose_text=more[:K - 1], compose_weights=torch.full((K,), 1.0 / K), compose_masks=masks)


def captured(s, ckw):
    """The captured evaluation of sampler s (its "eval" stage state) on x at sigma 1.3: (graph, output getter)."""
    st = s._stage_state("eval", x, s._inputs(x, text, TP, SOFT, unc, **ckw)[0])
    st["sig"].fill_(1.3)
    return st["g_eval"][0], (lambda: st["out"])


legs, samplers = {}, []
launches = {}
sig = torch.tensor(1.3, device="cuda")
with torch.no_grad():
    s = EDM_Sampler(model, Guide_net=model, num_solve_steps=40, guidance=1.0, use_graph=True)
    samplers.append(s)
    plain_graph, plain_out = captured(s, {})
    for K in range(1, args.kmax + 1):
        ckw = compose_kw(K)
        for mode in ("shared", "two_pass"):
            s = EDM_Sampler(model, Guide_net=model, num_solve_steps=40, guidance=G, use_graph=True, shared_guidance=mode == "shared")
            samplers.append(s)
            graph, out = captured(s, ckw)
            legs[(K, mode)] = ([graph], out)
            e = EDM_Sampler(model, Guide_net=model, num_solve_steps=40, guidance=G, shared_guidance=mode == "shared")
            e.denoise(x, sig, text, TP, SOFT, unc, **ckw)              # the second eager call is logged: the first may prepare weight images
            _lib.CALL_LOG = []
            e.denoise(x, sig, text, TP, SOFT, unc, **ckw)
            log, _lib.CALL_LOG = collections.Counter(name for name, _ in _lib.CALL_LOG), None
            launches[f"K{K}_{mode}"] = dict(total=sum(log.values()), **{n: log[n] for n in (
                "hdmoe_router_head_fwd", "hdmoe_dispatch_plan", "hdmoe_gather_rows_paired", "hdmoe_nhwc_to_nchw", "hdmoe_guide_compose",
                "hdmoe_nhwc_to_nchw_compose")})
        legs[(K, "plain")] = ([plain_graph] * (K + 1), plain_out)
    times = {k: [] for k in legs}
    for k, (graphs, out) in legs.items():                              # warm-up replays of every leg
        for _ in range(3):
            for g in graphs:
                g.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(out()).all(), k
    for _ in range(args.reps):
        for k, (graphs, _) in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                for g in graphs:
                    g.replay()
            t1.record()
            torch.cuda.synchronize()
            times[k].append(t0.elapsed_time(t1) / args.iters)
    diff = {}
    for K in range(1, args.kmax + 1):                                  # the two modes compute the same thing (bf16 compute mode)
        a, b = legs[(K, "shared")][1]().float(), legs[(K, "two_pass")][1]().float()
        diff[K] = float(f"{float((a - b).abs().max() / b.abs().max()):.3e}")
table = []
for K in range(1, args.kmax + 1):
    row = dict(K=K)
    for mode in ("shared", "two_pass", "plain"):
        ts = times[(K, mode)]
        row[mode + "_ms"] = round(statistics.median(ts), 3)
        row[mode + "_spread_ms"] = round(max(ts) - min(ts), 3)
    row["shared_vs_two_pass"] = round(row["shared_ms"] / row["two_pass_ms"], 3)
    row["shared_vs_plain"] = round(row["shared_ms"] / row["plain_ms"], 3)
    row["shared_vs_two_pass_max_rel_diff"] = diff[K]
    table.append(row)
line = json.dumps(dict(metric="compose_eval: ms per composed evaluation, graph replay", B=B, latents=f"4x{R}x{R} float32", compute="bf16",
                       guidance=G, masks="K vertical stripes, weights 1/K", reps=args.reps, iters_per_window=args.iters,
                       plain="K + 1 replays of the captured plain model() evaluation", table=table, launches_per_eager_eval=launches))
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
