"""Dev tool: cost of stochastic sampling with EDM_Sampler at the BASELINE configs[4] per-GPU share (B = 128, 4x64x64 latents, 8 experts, bf16,
use_graph=True), N = 40: deterministic Heun, S_churn = 40 on the host-driven loop (the evaluation alone is a graph), S_churn = 40 on the
device (churn_on_device: whole stages are graphs), DPM-Solver++(2M) and DPM-Solver++(2M) SDE.  One process, each mode on its own sampler
(its own capture), timed runs interleaved.  Prints one JSON line.
usage: sampler_stochastic_bench.py [--batch 128] [--steps 40] [--reps 3] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"), os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd", "Utils")]
import torch  # noqa: E402
import hdmoe_hip  # noqa: E402
from Utils import configs  # noqa: E402
from Utils.EDM_sampler import EDM_Sampler  # noqa: E402
from models import model_config2  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("needs a GPU")
B, N = args.batch, args.steps
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
# mode -> (constructor keywords, evaluations per sample, the flag that must be set); S_churn = N: gamma = min(1, sqrt(2) - 1) on every stage
modes = {
    "heun": (dict(), 2 * N - 1, "fused_heun"),
    "churn_host": (dict(S_churn=float(N)), 2 * N - 1, None),
    "churn_device": (dict(S_churn=float(N), churn_on_device=True), 2 * N - 1, "fused_heun"),
    "dpmpp_2m": (dict(solver="dpmpp_2m"), N, "fused_dpm"),
    "dpmpp_2m_sde": (dict(solver="dpmpp_2m_sde"), N, "fused_dpm"),
}
samplers = {k: EDM_Sampler(model, Guide_net=model, guidance=1.0, num_solve_steps=N, use_graph=True, **ckw) for k, (ckw, _, _) in modes.items()}
times = {k: [] for k in modes}
with torch.no_grad():
    for k, s in samplers.items():                                   # warm-up + capture
        out = s.sample(noise, text, -1.2, 1.2)
        assert torch.isfinite(out).all(), k
        flag = modes[k][2]
        assert (getattr(s, flag) if flag else not (s.fused_heun or s.fused_dpm)), k
    for _ in range(args.reps):
        for k, s in samplers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.sample(noise, text, -1.2, 1.2)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
res = {}
for k, (_, n_eval, _) in modes.items():
    dt = statistics.median(times[k])
    res[k] = dict(evals=n_eval, s=round(dt, 4), imgs_per_s=round(B / dt, 1), ms_per_eval=round(1e3 * dt / n_eval, 3),
                  spread_ms_per_eval=round(1e3 * (max(times[k]) - min(times[k])) / n_eval, 3), runs_s=[round(t, 4) for t in times[k]])
res["churn_device_vs_host_imgs_per_s"] = round(res["churn_device"]["imgs_per_s"] / res["churn_host"]["imgs_per_s"], 3)
res["churn_device_minus_heun_ms_per_eval"] = round(res["churn_device"]["ms_per_eval"] - res["heun"]["ms_per_eval"], 3)
res["sde_minus_dpm_ms_per_eval"] = round(res["dpmpp_2m_sde"]["ms_per_eval"] - res["dpmpp_2m"]["ms_per_eval"], 3)
line = json.dumps(dict(metric="sampler_stochastic", B=B, N=N, reps=args.reps, **res))
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
