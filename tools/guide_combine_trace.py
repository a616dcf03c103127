"""Dev tool: the guidance-combine kernels next to the plain blends, for a kernel trace.  B = 128 samples of 4x64x64 (the BASELINE configs[4]
latent: the resident arm, 16-byte accesses), each entry point --iters times after a warm-up: hdmoe_guide_combine fp32 with and without
momentum, hdmoe_lerp_rows, hdmoe_nhwc_to_nchw_guide_combine on a bf16 F with momentum, hdmoe_nhwc_to_nchw_guided_rows.  Run it under
    rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv -- python tools/guide_combine_trace.py
and read the kernels' average times from NAME_kernel_stats.csv; the tool prints the algorithmic bytes of each call (reads + writes of
B * per elements, as the issue counts them) so that bytes / time is the achieved rate.
usage: guide_combine_trace.py [--batch 128] [--iters 50]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"))
import torch  # noqa: E402
from hdmoe_hip import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--iters", type=int, default=50)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("needs a GPU")
B, C, H, W = args.batch, 4, 64, 64
per = C * H * W
gen = torch.Generator(device="cuda").manual_seed(0)
dc = 0.5 * torch.randn(B, C, H, W, device="cuda", generator=gen)
du = dc + 0.1 * torch.randn(B, C, H, W, device="cuda", generator=gen)
state = torch.zeros_like(dc)
g = torch.full((B,), 2.0, device="cuda")
F = torch.randn(2 * B, H, W, C, device="cuda", generator=gen).bfloat16()
sf, sx = torch.rand(B, device="cuda", generator=gen) + 0.5, torch.rand(B, device="cuda", generator=gen)
apg = dict(eta=0.0, norm_threshold=15.0, rescale=0.7)
calls = {
    "guide_combine_fp32_momentum": (lambda: ops.guide_combine(du, dc, g, momentum=-0.5, state=state, **apg), 5 * 4),
    "guide_combine_fp32": (lambda: ops.guide_combine(du, dc, g, **apg), 3 * 4),
    "lerp_rows_fp32": (lambda: ops.lerp_rows(du, dc, g), 3 * 4),
    "egress_combine_bf16_momentum": (lambda: ops.nhwc_to_nchw_guide_combine(F, sf, dc, sx, g, momentum=-0.5, state=state, **apg), 2 * 2 + 4 * 4),
    "egress_guided_rows_bf16": (lambda: ops.nhwc_to_nchw_guided(F, sf, dc, sx, g), 2 * 2 + 2 * 4),
}
for name, (fn, _) in calls.items():
    for _ in range(5 + args.iters):
        fn()
    torch.cuda.synchronize()
print(json.dumps(dict(metric="guide_combine_trace", B=B, per=per, iters=args.iters, resident=per <= ops.GUIDE_COMBINE_RESIDENT,
                      algorithmic_bytes={name: B * per * bpe for name, (_, bpe) in calls.items()})))
