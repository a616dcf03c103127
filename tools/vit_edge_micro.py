"""dev tool: eager timings of the ViT bank's two edges, per expert over all rows (ops.VIT_BANK_ROWS = False) against each expert's own
row window, at the bench shapes (R = 512 routed rows of 32 x 32 x 32 bf16, E = 32, patches [4, 8, 8, 16], even routing) and at the
sampler's bank (8 experts).  HIP events around 20 repetitions after 5 warm-up ones; `bytes` = the image-sized tensors each pass has to
read or write (3 per expert in the forward of an edge: relayout in / out and the GEMM operand; 4 in its backward; the all-rows path adds
the select / fan-out passes), so TB/s compares the passes with what they must move.  usage: vit_edge_micro.py OUT.json"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "heterogeneous-moe-for-diffusion-models_amd"))
import hdmoe_hip                                             # noqa: E402
from hdmoe_hip import ops                                    # noqa: E402
import models.model_components as mc                         # noqa: E402

DEV = "cuda"


def timed(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main(out_path):
    hdmoe_hip.set_compute_dtype(torch.bfloat16)
    rows = []
    for patches in ([4, 8, 8, 16], [4, 4, 8, 8, 8, 16, 16, 16]):
        R, H, C, E, G = 512, 32, 32, 32, len(patches)
        torch.manual_seed(0)
        experts = torch.nn.ModuleList([mc.Vit_expert(num_heads=8, num_groups=4, in_channels=C, seq_ln=(H // p) ** 2, emb_dim=E, num_blocks=1,
                                                     patch_size=p, time_dim=64, text_dim=64) for p in patches]).to(DEV)
        seg = torch.tensor([R * g // G for g in range(G + 1)], dtype=torch.int32, device=DEV)
        rag = ops.RagLayout(seg, [(H // p) ** 2 for p in patches], R)
        x = torch.randn(R, H, H, C, device=DEV).to(torch.bfloat16).requires_grad_(True)
        tok = torch.randn(R, rag.Sp, E, device=DEV).to(torch.bfloat16).requires_grad_(True)
        gtok, gimg = torch.randn_like(tok), torch.randn_like(x)
        img = R * H * H * C * 2
        ws, bs, pos = [e.patch.weight for e in experts], [e.patch.bias for e in experts], [e.pos_emb for e in experts]
        us = [e.unpatch_proj.weights for e in experts]

        def embed_old():
            pes = [ops.patch_embed(xe, w, b) for xe, w, b in zip(ops.fanout(x, G), ws, bs)]
            return ops.rag_pack(pes, pos, rag)

        def embed_new():
            return ops.vit_bank_embed(x, ws, bs, pos, rag)

        def unpatch_old():
            outs = [ops.pixel_shuffle_tokens(e.unpatch_proj._fwd(part), H, H, C, p) for e, p, part in zip(experts, patches, ops.rag_unpack(tok, rag))]
            return ops.rag_select(outs, rag)

        def unpatch_new():
            return ops.vit_bank_unpatch(tok, us, rag, H, H, C, patches, training=True)

        for edge, old, new, g_out in (("embed", embed_old, embed_new, gtok), ("unpatch", unpatch_old, unpatch_new, gimg)):
            for label, fn, share in (("all rows", old, 1.0), ("own rows", new, 1.0 / G)):
                def fwd():
                    with torch.no_grad():
                        fn()

                def both():
                    fn().backward(g_out)
                    x.grad = tok.grad = None
                t_f, t_fb = timed(fwd), timed(both)
                extra_f = (G + 1) * img if (edge == "unpatch" and label == "all rows") else 0             # rag_select
                extra_b = (G + 1) * img if label == "all rows" else 0                                     # rag_select_bwd / the fan-out's sum
                bf, bb = int(3 * G * img * share + extra_f), int(4 * G * img * share + extra_b)
                rows.append(dict(bank=patches, edge=edge, path=label, fwd_us=round(t_f, 1), bwd_us=round(t_fb - t_f, 1), fwd_bytes=bf, bwd_bytes=bb,
                                 fwd_TBps=round(bf / t_f / 1e6, 3), bwd_TBps=round(bb / max(t_fb - t_f, 1e-3) / 1e6, 3)))
                print(rows[-1], flush=True)
    json.dump(rows, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1])
