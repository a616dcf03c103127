"""Dev tool: cost of classifier-free guidance with EDM_Sampler at the BASELINE configs[4] per-GPU share (B = 128, 4x64x64 latents, 8 experts,
bf16, use_graph=True), N = 40, guidance 2.0 with a random unconditional embedding: guidance 1.0 (the floor: one evaluation per stage
evaluation), two-pass guidance (the reference's: the whole network twice + axpby) and shared guidance (shared_guidance=True: one pass with
shared routing, banks and tail on 2B rows, the lerp in the egress kernel), for Heun and DPM-Solver++(2M).  One process, each mode on its own
sampler (its own capture), timed runs interleaved.  Also counts, from the binding's call log, the library entry points one eager guided
evaluation goes through in both modes.  Prints one JSON line.
--root DIR --no-shared times the floor and the two-pass mode of another checkout of the repository (one without the shared mode, built in
place), for a same-box comparison in the manner of tools/ab_trees.sh.
--interval LO HI adds, per solver and guidance mode, a leg with guidance_interval=(LO, HI) (guided only where LO <= sigma <= HI, the plain
evaluation elsewhere), its counts of guided and plain evaluations, and the prediction n_guided t_guided + n_plain t_floor from the same
run's per-evaluation times of the always-guided and the floor leg.
--combine adds, per solver and guidance mode, three legs whose guided evaluations blend through the combine kernel (guidance rescale 0.7;
APG with eta 0, norm threshold 15, momentum -0.5; both), each next to the plain-guided leg of the same run: imgs/s against it, the extra
ms per evaluation, and the plain leg's spread over the repetitions, which is what that difference has to be read against.
usage: sampler_guidance_bench.py [--batch 128] [--steps 40] [--reps 3] [--guidance 2.0] [--interval LO HI] [--combine] [--root DIR]
       [--no-shared] [--out FILE]"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                                            # before the imports: which checkout they come from
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path[:0] = [os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"), os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils")]
import torch  # noqa: E402
import hdmoe_hip  # noqa: E402
from hdmoe_hip import _lib  # noqa: E402
from Utils import configs  # noqa: E402
from Utils.EDM_sampler import EDM_Sampler  # noqa: E402
from models import model_config2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--guidance", type=float, default=2.0)
ap.add_argument("--interval", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="add guidance-interval legs")
ap.add_argument("--combine", action="store_true", help="add guidance-rescale / APG legs (the combine kernel)")
ap.add_argument("--root", default=None, help="time the package of this checkout instead of the one the tool lives in")
ap.add_argument("--no-shared", action="store_true", help="floor and two-pass only (a checkout without shared_guidance)")
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("needs a GPU")
B, N, G = args.batch, args.steps, args.guidance
hdmoe_hip.set_compute_dtype(torch.bfloat16)
kw = configs.model_kwargs(**configs.BASELINE_CONFIGS[4]["over"])
torch.manual_seed(0)
model = model_config2.preconditioned_HDMOEM(**kw).cuda().eval()
with torch.no_grad():
    for n, p in model.named_parameters():
        if n.endswith("out_gain"):
            p.fill_(0.5)
gen = torch.Generator(device="cuda").manual_seed(0)
noise = torch.randn(B, 4, 64, 64, device="cuda", generator=gen)
text = torch.randn(B, 77, kw["text_emb_dim"], device="cuda", generator=gen)
unc = torch.randn(B, 77, kw["text_emb_dim"], device="cuda", generator=gen)
solvers = {"heun": (dict(), 2 * N - 1, "fused_heun"), "dpmpp_2m": (dict(solver="dpmpp_2m"), N, "fused_dpm")}
guides = {"floor": dict(guidance=1.0), "two_pass": dict(guidance=G), "shared": dict(guidance=G, shared_guidance=True)}
if args.no_shared:
    del guides["shared"]
if args.interval is not None:                                       # an interval leg behind each always-guided one
    guides.update({gm + "_interval": dict(gkw, guidance_interval=tuple(args.interval)) for gm, gkw in list(guides.items())
                   if gm != "floor"})
COMBINE = {"rescale": dict(guidance_rescale=0.7), "apg": dict(apg_eta=0.0, apg_norm_threshold=15.0, apg_momentum=-0.5)}
COMBINE["both"] = dict(COMBINE["rescale"], **COMBINE["apg"])
combine_legs = {}
if args.combine:                                                    # three combine legs behind each always-guided one
    combine_legs = {f"{gm}_{leg}": gm for gm in [gm for gm in ("two_pass", "shared") if gm in guides] for leg in COMBINE}
    guides.update({name: dict(guides[gm], **COMBINE[name[len(gm) + 1:]]) for name, gm in combine_legs.items()})
samplers = {(sv, gm): EDM_Sampler(model, Guide_net=model, num_solve_steps=N, use_graph=True, **skw, **gkw)
            for sv, (skw, _, _) in solvers.items() for gm, gkw in guides.items()}
times = {k: [] for k in samplers}
outs = {}
with torch.no_grad():
    for k, s in samplers.items():                                   # warm-up + capture
        outs[k] = s.sample(noise, text, -1.2, 1.2, unc)
        assert torch.isfinite(outs[k]).all(), k
        assert getattr(s, solvers[k[0]][2]), k
    for _ in range(args.reps):
        for k, s in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.sample(noise, text, -1.2, 1.2, unc)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    # library calls of ONE eager guided evaluation (the second one: the first may prepare weight images)
    launches = {}
    sig = torch.tensor(1.3, device="cuda")
    for gm in [gm for gm in ("two_pass", "shared", "two_pass_both", "shared_both") if gm in guides]:
        s = EDM_Sampler(model, Guide_net=model, num_solve_steps=N, **guides[gm])
        ms = dict(momentum_state=torch.zeros_like(noise)) if gm in combine_legs else {}
        s.denoise(noise, sig, text, -1.2, 1.2, unc, **ms)
        _lib.CALL_LOG = []
        s.denoise(noise, sig, text, -1.2, 1.2, unc, **ms)
        log, _lib.CALL_LOG = collections.Counter(name for name, _ in _lib.CALL_LOG), None
        launches[gm] = dict(total=sum(log.values()), **{n: log[n] for n in (
            "hdmoe_router_head_fwd", "hdmoe_dispatch_plan", "hdmoe_gather_rows", "hdmoe_gather_rows_paired", "hdmoe_nhwc_to_nchw",
            "hdmoe_nhwc_to_nchw_guided", "hdmoe_axpby", "hdmoe_conv_fwd", "hdmoe_guide_combine", "hdmoe_nhwc_to_nchw_guide_combine")})
res = {}
for sv, (_, n_eval, _) in solvers.items():
    r = {}
    for gm in guides:
        ts = times[(sv, gm)]
        dt = statistics.median(ts)
        r[gm] = dict(s=round(dt, 4), imgs_per_s=round(B / dt, 1), ms_per_eval=round(1e3 * dt / n_eval, 3),
                     spread_ms_per_eval=round(1e3 * (max(ts) - min(ts)) / n_eval, 3), runs_s=[round(t, 4) for t in ts])
    r["evals"] = n_eval
    for gm in [gm for gm in guides if gm.endswith("_interval")]:    # ms_per_eval of these legs is per evaluation of either kind
        ev = samplers[(sv, gm)].last_evaluations
        base = gm[:-len("_interval")]
        pred = (ev["guided"] * r[base]["ms_per_eval"] + ev["plain"] * r["floor"]["ms_per_eval"]) / 1e3
        r[gm].update(evaluations=ev, predicted_s=round(pred, 4), measured_vs_predicted=round(r[gm]["s"] / pred, 3),
                     vs_always_guided_s=round(r[gm]["s"] / r[base]["s"], 3))
    for gm, base in combine_legs.items():                           # next to the plain-guided leg of the same run
        r[gm].update(vs_plain_imgs_per_s=round(r[gm]["imgs_per_s"] / r[base]["imgs_per_s"], 4),
                     extra_ms_per_eval=round(r[gm]["ms_per_eval"] - r[base]["ms_per_eval"], 3),
                     plain_spread_ms_per_eval=r[base]["spread_ms_per_eval"])
        d = (outs[(sv, gm)] - outs[(sv, base)]).abs().max() / outs[(sv, base)].abs().max()
        r[gm]["vs_plain_max_rel_diff"] = float(f"{float(d):.3e}")
    r["two_pass_vs_floor_ms_per_eval"] = round(r["two_pass"]["ms_per_eval"] / r["floor"]["ms_per_eval"], 3)
    if "shared" in guides:
        r["shared_vs_two_pass_imgs_per_s"] = round(r["shared"]["imgs_per_s"] / r["two_pass"]["imgs_per_s"], 3)
        r["shared_vs_floor_ms_per_eval"] = round(r["shared"]["ms_per_eval"] / r["floor"]["ms_per_eval"], 3)
        d = (outs[(sv, "shared")] - outs[(sv, "two_pass")]).abs().max() / outs[(sv, "two_pass")].abs().max()
        r["shared_vs_two_pass_max_rel_diff"] = float(f"{float(d):.3e}")
    res[sv] = r
line = json.dumps(dict(metric="sampler_guidance", root=os.path.relpath(ROOT, os.getcwd()), B=B, N=N, guidance=G, interval=args.interval, combine=COMBINE if args.combine else None, reps=args.reps, launches_per_guided_eval=launches, **res))
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
