/* libhdmoe_hip.so -- C ABI of the MI355X (gfx950) kernels behind the HDMOEM denoising hot path.
 *
 * The reference (cs2mosa/Heterogeneous-MOE-for-Diffusion-models) is pure PyTorch: it has no FFI / operator
 * registry, its "interface" for this path is the ATen call sequence inside models/model_internals.py,
 * models/model_components.py and models/model_config{1,2}.py.  Each entry point below replaces one such
 * sequence (cited as reference file:line); the Python nn.Module mirror in
 * heterogeneous-moe-for-diffusion-models_amd/models/ binds them with ctypes.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is DEVICE memory unless the comment says "host array".
 *   - activations are NHWC / [rows][C] contiguous; `dtype` (HDMOE_F32 | HDMOE_BF16) is their element type.
 *     Statistics, per-sample scalars, (B,F) embeddings, parameters and parameter gradients are fp32.
 *   - `stream` is a hipStream_t (void*); kernels are enqueued on it, nothing syncs, allocates or frees,
 *     so every call is hipGraph-capturable.  Scratch / accumulators are caller-provided.
 *   - return 0 on success, HDMOE_EINVAL / HDMOE_EDTYPE / HDMOE_ELAUNCH (<0) otherwise; never throws.
 *   - "grouped": rows of one launch belong to up to HDMOE_MAX_GROUPS experts; seg[g]..seg[g+1] (device int32)
 *     is the row range of expert g; per-group kernel sizes come as host arrays of length ngroups.
 */
#ifndef HDMOE_H
#define HDMOE_H
#ifdef __cplusplus
extern "C" {
#endif

#ifndef HDMOE_OK
#define HDMOE_OK 0
#define HDMOE_EINVAL (-1)
#define HDMOE_EDTYPE (-2)
#define HDMOE_ELAUNCH (-3)
#define HDMOE_F32 0
#define HDMOE_BF16 1
#define HDMOE_F16 3  /* hdmoe_cast only: fp16 tensors at the module boundary (`.half()` callers) are converted at ingest / egress */
#define HDMOE_F32S 2 /* fp32 activations computed as split bf16 (hi + lo, three MFMAs per product): weight images = bf16 [hi | lo] planes */
#define HDMOE_MAX_GROUPS 8
#endif

typedef void* hdmoe_stream_t; /* hipStream_t */
#ifdef __HIPCC__
#define HS hipStream_t
#else
#define HS hdmoe_stream_t
#endif

int hdmoe_version(void);

/* ---- K3: MP_Conv = weight prep + implicit-GEMM conv  (model_internals.py:253-275) ------------------------ */
/* w_raw/gain_ptr/kh/kw: host arrays [ngroups].  wf: [g][tap][O][Ipad]; wd (optional): [g][tap'][I][Opad]
 * (tap' flipped when flip=1: the dgrad operand).  normalize=0: plain nn.Conv2d weight (Vit_expert.patch).
 * mutate=1: training-mode forced weight normalisation, written back into w_raw (:254-256). */
int hdmoe_wprep_fwd(float* const* w_raw, const float* const* gain_ptr, float gain_val, const int* kh, const int* kw,
                    int ngroups, int O, int I, int Ipad, int Opad, void* wf, long wf_stride, void* wd, long wd_stride,
                    int normalize, int mutate, int flip, int dtype, HS stream);
/* G: per-group [tap][O][I] fp32 gradient w.r.t. the effective weight (from hdmoe_conv_wgrad);
 * dw: per-group (O,I,kh,kw) fp32; dgain: per-group scalar accumulators or NULL. */
int hdmoe_wprep_bwd(const float* const* w_raw, const float* const* gain_ptr, float gain_val, const float* const* G,
                    float* const* dw, float* const* dgain, const int* kh, const int* kw, int ngroups, int O, int I,
                    int normalize, HS stream);
/* y = alpha*conv(x, w) + beta*res.  x [N][H][W][Cphys]; logical Cin = Cphys (+1 implicit all-ones channel when
 * ones=1: Unet_expert's torch.cat([x, ones]), model_components.py:416); y [N][Ho][Wo][Cstore], Cstore <= Cout.
 * Also runs dgrad (w = wd, pads flipped) and every F.linear (H = W = 1 or N = 1). */
int hdmoe_conv_fwd(const void* x, const void* w, void* y, const void* res, float alpha, float beta, const int* seg,
                   int ngroups, long wstride, int N, int H, int W, int Ho, int Wo, int Cin, int Cphys, int Ipad, int Cout,
                   int Cstore, int stride, int ones, const int* kh, const int* kw, const int* pt, const int* pl, int dtype,
                   HS stream);
/* G[g] ([tap][Cout][Cin] fp32, pre-zeroed) += dy^T * shifted(x); G: host array of device pointers. */
int hdmoe_conv_wgrad(const void* x, const void* dy, float* const* G, const int* seg, int ngroups, int N, int H, int W,
                     int Ho, int Wo, int Cin, int Cphys, int Cout, int stride, int ones, const int* kh, const int* kw,
                     const int* pt, const int* pl, int dtype, HS stream);

/* Atomic-free weight gradient for the k x k (k = 3, 5) bf16 layers (csrc/wgrad6.hip): same contract as hdmoe_conv_wgrad plus a
 * caller-provided workspace of hdmoe_conv_wgrad6_ws_kib(...) KiB (0 = shape outside the kernel's domain).  hdmoe_conv_wgrad6
 * returns 1 without launching when it does not apply; the caller then uses hdmoe_conv_wgrad. */
int hdmoe_conv_wgrad6_ws_kib(int ngroups, int N, int H, int W, int Cin, int Cout, const int* kh, const int* kw, int dtype);
int hdmoe_conv_wgrad6(const void* x, const void* dy, float* const* G, const int* seg, int ngroups, int N, int H, int W, int Cin,
                      int Cout, const int* kh, const int* kw, const int* pt, const int* pl, void* ws, long ws_bytes, int dtype,
                      int defer, HS stream);
/* defer != 0: the partial slabs stay in `ws` (2 x ws_kib KiB: one region per kernel-size class) and are summed into G later by ONE
 * batched launch per 16 (layer, class) items.  Per deferred call i: G + 8 i = its per-expert slabs, seg[i], ws[i], and
 * dims + 16 i = {ngroups, N, H, W, Cin, Cout, dtype, 0, kh[0..7]}. */
/* Input gradient and (deferred) weight gradient of one grouped k x k bf16 layer with 3x3 and 5x5 experts in ONE launch (csrc/bwd6.hip):
 * dx = alpha * dgrad(dy, wd) like hdmoe_conv_fwd on the flipped image, partial dW slabs into ws like hdmoe_conv_wgrad6(defer = 1).
 * Returns 1 without launching when the layer is outside the domain. */
int hdmoe_conv_bwd6(const void* x, const void* dy, const void* wd, void* dx, float* const* G, const int* seg, int ngroups,
                    long wd_stride, int N, int H, int W, int Cin, int Cout, const int* kh, const int* kw, const int* pt,
                    const int* pl, float alpha, void* ws, long ws_bytes, int dtype, HS stream);
/* The same for a layer whose input is h = dropout_p(mp_silu(u * film_e[n][c])) and feeds nothing else (conv_res2 of Unet_block): the FiLM
 * backward runs in the dgrad program's epilogue.  dx receives du (bit-identical to hdmoe_conv_bwd6 + hdmoe_film_silu_drop_bwd), film_de
 * [N][Cin] fp32 the gradient of film_e (written, not accumulated; summed in a fixed order).  film_mask: the keep bytes of
 * hdmoe_film_silu_drop_fwd_mask, NULL exactly when film_p == 0.  Returns 1 without launching outside the epilogue's domain (bwd7 on
 * 32 x 32 maps; on 16 x 16 maps Cin % 64 == 0 and Cout % 64 == 0). */
int hdmoe_conv_bwd6_film(const void* x, const void* dy, const void* wd, void* dx, float* const* G, const int* seg, int ngroups,
                         long wd_stride, int N, int H, int W, int Cin, int Cout, const int* kh, const int* kw, const int* pt,
                         const int* pl, float alpha, void* ws, long ws_bytes, const void* film_u, const float* film_e,
                         const unsigned char* film_mask, float* film_de, float film_p, int dtype, HS stream);
/* Input gradient and weight gradient of one (grouped) POINTWISE bf16 layer (linear / 1x1, stride 1, no ones channel) in ONE launch
 * (csrc/pbwd.hip): x [N * HW][Cin], dy [N * HW][Cout], dx = alpha * dy * w from the flipped image wd ([g][Cin][Cout], wd_stride
 * elements per group), G[g] ([Cout][Cin] fp32) += dy^T x.  dy is read once.  Domain: Cin % 32 == 0, Cout % 32 == 0, both <= 128,
 * (Cin / 32) * (Cout / 32) <= 8.  Returns 1 without launching outside it; the caller then uses hdmoe_conv_fwd + hdmoe_conv_wgrad. */
int hdmoe_pw_bwd(const void* x, const void* dy, const void* wd, void* dx, float* const* G, const int* seg, int ngroups,
                 long wd_stride, int N, long HW, int Cin, int Cout, float alpha, int dtype, HS stream);
/* Two pointwise bf16 layers with 32 outputs each over the SAME input (the k / v projections of a cross-attention over a wide context),
 * one launch per direction, x read once (csrc/kgemm.hip, csrc/lwgrad.hip).  x [M][K]; w1 / w2 the prepared forward images [32][K].
 *   hdmoe_kgemm2_fwd: y1 = alpha1 x w1^T, y2 = alpha2 x w2^T ([M][32]), each bit-equal to hdmoe_conv_fwd of its layer (the long-
 *     contraction kernel: K % 64 == 0, K >= 512).
 *   hdmoe_lwgrad2: G1 ([32][K] fp32) += dy1^T x, G2 += dy2^T x, each workgroup's partial sums those of hdmoe_conv_wgrad of the layer.
 * Return 1 without launching outside the domain (bf16, K as above, 16-byte aligned x, images and dy). */
int hdmoe_kgemm2_fwd(const void* x, const void* w1, const void* w2, void* y1, void* y2, long M, int K, float alpha1, float alpha2,
                     int dtype, HS stream);
int hdmoe_lwgrad2(const void* x, const void* dy1, const void* dy2, float* G1, float* G2, long P, int Cin, int dtype, HS stream);
/* Fusion stage, the token-local chain in front of the first attention call in one launch per direction (csrc/fusion.hip).  All tensors
 * [rows][32] bf16, contiguous, 16-byte aligned; sw [rows / S] fp32 per-sample swap weights or NULL; wq / wk / wv the prepared FORWARD
 * images ([32][32]) of the three projections, wdq / wdk / wdv their flipped images, alpha_* the layers' output scales.
 *   fwd: query = fu + sw (fv - fu), ctx = fv - sw (fv - fu) (not written, and may be NULL, when sw is NULL: they are fu and fv),
 *        q = alpha_q Wq query, k = alpha_k Wk ctx, v = alpha_v Wv ctx.
 *   bwd: dfu, dfv from dq, dk, dv and the further gradients gquery / gctx of query / ctx (either may be NULL); dsw [rows / S] fp32
 *        accumulates (float atomics, as hdmoe_scale_rows_bwd); fu, fv, dsw are read only with sw.  No weight gradients: those are
 *        hdmoe_conv_wgrad's, from query / ctx and dq / dk / dv.
 * bf16 rounding at every point where the unfused chain (hdmoe_axpby, hdmoe_scale_rows_*, hdmoe_conv_fwd, hdmoe_pw_bwd, the sums of
 * two gradients) stores a tensor.  Returns 1 without launching outside the domain: dtype bf16, C == 32, aligned bases. */
int hdmoe_fusion_in_fwd(const void* fu, const void* fv, const float* sw, const void* wq, const void* wk, const void* wv,
                        void* query, void* ctx, void* q, void* k, void* v, long rows, long S, int C, float alpha_q,
                        float alpha_k, float alpha_v, int dtype, HS stream);
int hdmoe_fusion_in_bwd(const void* dq, const void* dk, const void* dv, const void* gquery, const void* gctx, const void* fu,
                        const void* fv, const float* sw, const void* wdq, const void* wdk, const void* wdv, void* dfu, void* dfv,
                        float* dsw, long rows, long S, int C, float alpha_q, float alpha_k, float alpha_v, int dtype, HS stream);
/* hdmoe_fusion_in_bwd with the three projections' weight gradients contracted in the same launch: Gq, Gk, Gv ([32][32] fp32, the
 * bank's [O][I] slab of a 1x1 layer as hdmoe_conv_wgrad fills it) += dq^T query, dk^T ctx, dv^T ctx, with query / ctx recomputed from
 * fu, fv, sw as the forward rounds them -- fu and fv are therefore read with and without sw.  dfu, dfv are bit-equal to
 * hdmoe_fusion_in_bwd's; the slabs (and dsw) are fp32 sums in another order (accumulated per wave over its tiles, the four waves of a
 * workgroup met in wave order, one float-atomic flush per workgroup).  max_wg: cap of the persistent grid, 0 = the default (512). */
int hdmoe_fusion_in_bwd_wg(const void* dq, const void* dk, const void* dv, const void* gquery, const void* gctx, const void* fu,
                           const void* fv, const float* sw, const void* wdq, const void* wdk, const void* wdv, void* dfu, void* dfv,
                           float* dsw, float* Gq, float* Gk, float* Gv, int max_wg, long rows, long S, int C, float alpha_q,
                           float alpha_k, float alpha_v, int dtype, HS stream);
/* The chain behind the text attention of the fusion stage, down to the gate, in one launch per direction (csrc/fusion.hip).  Row tensors
 * [rows][32] bf16 unless noted; alpha_txt the device scalar of lerp_param; wo / w1 / w2 the forward images of cross_attn_text.out_proj
 * ([32][32], output scale alpha_o, residual weight beta_o), gate1 ([32][64], alpha_1) and gate2 ([2][32], alpha_2), wdo / wd1 / wd2
 * their flipped images ([32][32], [64][32], [32][16]); wa, wb the weights of mp_cat.
 *   fwd: at = alpha_o Wo o2 + beta_o a; a2 = a + alpha_txt (at - a); cat = [wa U | wb a2] ([rows][64]); g1 = alpha_1 W1 cat;
 *        s = mp_silu(g1); gate = softmax(alpha_2 W2 s) ([rows][2] fp32); mixed = hdmoe_gate_mix_fwd(logits, U, a2).
 *        a2, g1 are what the backward reads, cat, s the x of hdmoe_conv_wgrad for gate1, gate2; all four NULL: not written
 *        (inference); cat and s alone NULL: those two not written (hdmoe_fusion_out_bwd_wg recomputes them).
 *   bwd: from dmixed and dgate (or NULL): do2, da (the lerp's and the residual's share, summed), dU (gate_mix's and mp_cat's share,
 *        summed), dalpha += (fp32, one atomic per workgroup), and dat, dg1, dl ([rows][2]): the dy of the three weight gradients
 *        (hdmoe_conv_wgrad with x = o2, cat, s).
 * bf16 rounding wherever the unfused ops store a tensor.  Returns 1 without launching outside the domain (bf16, C == 32, aligned). */
int hdmoe_fusion_out_fwd(const void* o2, const void* a, const void* U, const float* alpha_txt, const void* wo, const void* w1,
                         const void* w2, void* mixed, float* gate, void* a2, void* g1, void* cat, void* s, long rows, int C,
                         float alpha_o, float beta_o, float wa, float wb, float alpha_1, float alpha_2, int dtype, HS stream);
int hdmoe_fusion_out_bwd(const void* dmixed, const float* dgate, const float* gate, const void* U, const void* a2, const void* g1,
                         const void* o2, const void* a, const float* alpha_txt, const void* wo, const void* wdo, const void* wd1,
                         const void* wd2, void* do2, void* da, void* dU, void* dat, void* dg1, void* dl, float* dalpha, long rows,
                         int C, float alpha_o, float beta_o, float wa, float wb, float alpha_1, float alpha_2, int dtype, HS stream);
/* hdmoe_fusion_out_bwd with the three layers' weight gradients contracted in the same launch: Go ([32][32] fp32), G1 ([32][64]),
 * G2 ([2][32]), the bank's [O][I] slabs, += dat^T o2, dg1^T cat, dl^T s.  dat, dg1, dl are rounded to bf16 where hdmoe_fusion_out_bwd
 * stores them and are not written; cat and s are recomputed from U, a2, g1 with the forward's formula and rounding.  do2, da, dU are
 * bit-equal to hdmoe_fusion_out_bwd's; the slabs (and dalpha) are fp32 sums in another order, flushed as in hdmoe_fusion_in_bwd_wg.
 * max_wg: cap of the persistent grid, 0 = the default (512). */
int hdmoe_fusion_out_bwd_wg(const void* dmixed, const float* dgate, const float* gate, const void* U, const void* a2, const void* g1,
                            const void* o2, const void* a, const float* alpha_txt, const void* wo, const void* wdo, const void* wd1,
                            const void* wd2, void* do2, void* da, void* dU, float* dalpha, float* Go, float* G1, float* G2, int max_wg,
                            long rows, int C, float alpha_o, float beta_o, float wa, float wb, float alpha_1, float alpha_2, int dtype,
                            HS stream);
/* The chain between the fusion stage's two attention cores in one launch per direction (csrc/fusion.hip).  Row tensors [rows][32] bf16;
 * wo / wq the forward images of cross_attn.out_proj (output scale alpha_o, residual weight beta_o) and cross_attn_text.q_proj (alpha_q),
 * wdo / wdq their flipped images.
 *   fwd: a = alpha_o Wo o1 + beta_o query (rounded as hdmoe_conv_fwd's residual epilogue rounds it); q2 = alpha_q Wq a.
 *   bwd: da_t = da + alpha_q Wq^T dq2 (the gradient fan-in of a); do1 = alpha_o Wo^T da_t; dres = beta_o da_t (the residual's share of
 *        query's gradient); with Go, Gq ([32][32] fp32 slabs; both or neither): Go += da_t^T o1, Gq += dq2^T a, accumulated and flushed as
 *        in hdmoe_fusion_in_bwd_wg (max_wg likewise); a and o1 are read only then.
 * bf16 rounding wherever hdmoe_conv_fwd, hdmoe_pw_bwd, the bf16 sum of two gradients and hdmoe_axpby store a tensor: every bf16 output
 * is bit-equal to theirs.  Returns 1 without launching outside the domain (bf16, C == 32, aligned). */
int hdmoe_fusion_mid_fwd(const void* o1, const void* query, const void* wo, const void* wq, void* a, void* q2, long rows, int C,
                         float alpha_o, float beta_o, float alpha_q, int dtype, HS stream);
int hdmoe_fusion_mid_bwd(const void* da, const void* dq2, const void* a, const void* o1, const void* wdo, const void* wdq, void* do1,
                         void* dres, float* Go, float* Gq, int max_wg, long rows, int C, float alpha_o, float beta_o, float alpha_q,
                         int dtype, HS stream);
int hdmoe_conv_bwd6s(const void* x, const void* dy, const void* wd, void* dx, float* const* G, const int* seg, int ngroups,
                     long wd_stride, long wd_plane, int N, int H, int W, int Cin, int Cout, const int* kh, const int* kw,
                     const int* pt, const int* pl, float alpha, void* ws, long ws_bytes, const float* in_scale, const float* in_shift,
                     int in_relu, int hi_only, HS stream);   /* fp32 tensors, split bf16 (3x3); in_scale / in_shift (or NULL): x is relu(x * scale[n][c] + shift[n][c]);
                                                 hi_only = 1: bf16 operands (the hi halves) with fp32 accumulation -- one MFMA per product instead of three */
/* GroupNorm(1, C) + ReLU of the router trunks fused into the neighbouring convs (model_components.py:100-112): the conv writes per-sample
 * partial statistics of its output, hdmoe_gn1_finalize turns them into mean / rstd and a per-(sample, channel) scale / shift, the NEXT
 * conv (and its weight gradient, hdmoe_conv_bwd6s) apply relu(x * scale + shift) while staging x, hdmoe_gn1_relu_mean is the last
 * GroupNorm + ReLU + AdaptiveAvgPool2d(1). */
int hdmoe_conv_fwd_split_gn(const void* x, const void* w, void* y, const float* in_scale, const float* in_shift, int in_relu,
                            float* stats_ws, long wstride, long wplane, int N, int H, int W, int Cin, int Cout, float alpha, HS stream);
/* k x k bf16 expert conv with the FiLM of Unet_block (mp_silu(y * emb) + dropout, model_components.py:242-246) as a second output of its
 * epilogue; 1 = outside the fused kernel's domain, nothing launched. */
int hdmoe_conv_fwd_film(const void* x, const void* w, void* y, void* h, const float* e, unsigned long long seed,
                        const unsigned long long* seed_dev, float p, float alpha, const int* seg, int ngroups, long wstride, int N, int H, int W,
                        int Cin, int Cout, const int* kh, const int* kw, const int* pt, const int* pl, int dtype, HS stream);
int hdmoe_conv_split_stats_slots(int H, int W, int Cout);   /* partial-statistics slots per sample of hdmoe_conv_fwd_split_gn (0: outside its domain) */
int hdmoe_gn1_finalize(float* scale, float* shift, float* mean, float* rstd, const float* ws, const float* gamma, const float* beta,
                       int N, int slots, int C, long count, float eps, HS stream);
int hdmoe_gn1_relu_mean(float* out, const float* y, const float* scale, const float* shift, int N, long S, int C, HS stream);
int hdmoe_gn1_finalize_relu_mean(float* out, float* scale, float* shift, float* mean, float* rstd, const float* y, const float* ws,
                                 const float* gamma, const float* beta, int N, int slots, long S, int C, float eps, HS stream);   /* the two above in one launch */
int hdmoe_gn1_finalize_relu_mean_pq(float* out, float* scale, float* shift, float* mean, float* rstd, float* pcnt, float* qsum, const float* y,
                                    const float* ws, const float* gamma, const float* beta, int N, int slots, long S, int C, float eps, HS stream);
    /* the same, and pcnt / qsum [N][C]: the count of positions where the ReLU is open and the sum of (y - mean) * rstd over them (for hdmoe_gn1t_apply) */
int hdmoe_conv_wgrad6_reduce_batch(float* const* G, const int* const* seg, float* const* ws, const int* dims, int n, HS stream);

/* development hook of the conv6 kernels: `buf` = device array of 8 x 64 uint64 receiving workgroup 0's in-kernel clock stamps
 * (tag << 56 | s_memtime) of every later launch; NULL switches it off (tools/conv6_check.py --stamps). */
int hdmoe_conv6_debug_stamps(void* buf);

/* Kernel-selection counters: which conv program the host code chose, counted where it enqueues the launch (plain host
 * std::atomic<long long>, nothing is written to device memory).  Under stream / graph capture the count moves at the capture,
 * not at each replay.  counts: HOST array of n long longs receiving the first min(n, HDMOE_SEL_COUNT) counters (NULL: none);
 * reset != 0 zeroes all counters after the read.  Returns HDMOE_SEL_COUNT.  hdmoe_hip.ops.kernel_selections() names them. */
enum {
  HDMOE_SEL_CONV7_32 = 0,        /* conv7 forward / dgrad program (hdmoe_conv_fwd), 32 x 32 maps */
  HDMOE_SEL_CONV7_16 = 1,        /* the same, 16 x 16 maps (pairs of images) */
  HDMOE_SEL_CONV6 = 2,           /* conv6 (hdmoe_conv_fwd, hdmoe_conv_fwd_film) */
  HDMOE_SEL_CONV6S = 3,          /* split-bf16 conv6s (hdmoe_conv_fwd with HDMOE_F32S, hdmoe_conv_fwd_split_gn) */
  HDMOE_SEL_BWD7_32 = 4,         /* fused backward with the conv7 dgrad program, 32 x 32 maps */
  HDMOE_SEL_BWD7_32_WGRAD8 = 5,  /*   ... with a 3x3 expert: wgrad8 (chunk layouts below) */
  HDMOE_SEL_BWD7_32_WGRAD7 = 6,  /*   ... with a 5x5 expert: wgrad7 */
  HDMOE_SEL_BWD7_16_OT1 = 7,     /* fused backward with the conv7 dgrad program, 16 x 16 maps, wgrad6 programs with OT = 1 */
  HDMOE_SEL_BWD7_16_OT2 = 8,     /*   ... OT = 2 (Cout % 64 == 0) */
  HDMOE_SEL_BWD6 = 9,            /* fused backward with the conv6 dgrad program (hdmoe_conv_bwd6 outside conv7's domain) */
  HDMOE_SEL_BWD6S = 10,          /* fused split-bf16 backward (hdmoe_conv_bwd6s) */
  HDMOE_SEL_WGRAD6_DIRECT = 11,  /* hdmoe_conv_wgrad6, defer = 0 (wgrad6 + its own reduction) */
  HDMOE_SEL_WGRAD6_DEFER = 12,   /* hdmoe_conv_wgrad6, defer = 1 (partial slabs for hdmoe_conv_wgrad6_reduce_batch) */
  HDMOE_SEL_BLK6 = 13,           /* hdmoe_unet_block_fwd */
  HDMOE_SEL_WGRAD8_C11 = 14,     /* wgrad8 inside bwd7: icw x ocw = 1 x 1 channel chunks per workgroup */
  HDMOE_SEL_WGRAD8_C12 = 15,     /*   1 x 2 */
  HDMOE_SEL_WGRAD8_C21 = 16,     /*   2 x 1 */
  HDMOE_SEL_WGRAD8_C22 = 17,     /*   2 x 2 */
  HDMOE_SEL_PW_BWD = 18,         /* hdmoe_pw_bwd: pointwise layer, input + weight gradient in one launch */
  HDMOE_SEL_RELAYOUT_TILED = 19,   /* hdmoe_patch_relayout_tiled: order-1 patch <-> image relayout, tiled through LDS */
  HDMOE_SEL_COMBINE_FWD_VEC = 20,  /* hdmoe_combine_rows_fwd_vec: 16-byte combine forward (also the gather's backward) */
  HDMOE_SEL_COMBINE_BWD_VEC = 21,  /* hdmoe_combine_rows_bwd_vec: 16-byte combine backward */
  HDMOE_SEL_FILM_DGRAD = 22,       /* hdmoe_conv_bwd6_film: the bwd7 launch with the FiLM-backward epilogue in its dgrad program */
  HDMOE_SEL_ROW_WINDOW = 23,       /* a row-windowed launch (the hdmoe_*_rows / hdmoe_rag_*_own entry points of the ViT bank's edges) */
  HDMOE_SEL_FUSION_IN = 24,        /* hdmoe_fusion_in_fwd: fusion inputs + q / k / v projections of cross_attn in one launch */
  HDMOE_SEL_FUSION_IN_BWD = 25,    /* hdmoe_fusion_in_bwd: their input gradients, the gradient fan-in and dsw in one launch */
  HDMOE_SEL_FUSION_OUT = 26,       /* hdmoe_fusion_out_fwd: text out_proj + lerp + mp_cat + gate1 + mp_silu + gate2 + gate_mix in one launch */
  HDMOE_SEL_FUSION_OUT_BWD = 27,   /* hdmoe_fusion_out_bwd: their input gradients, the gradient fan-in and dalpha in one launch */
  HDMOE_SEL_ATTN_FWD_MFMA = 28,    /* hdmoe_attn_fwd: the bf16 D = 4 MFMA forward kernel */
  HDMOE_SEL_ATTN_BWD_MERGED = 29,  /* hdmoe_attn_bwd: the merged MFMA backward (Sq <= 1024) */
  HDMOE_SEL_ATTN_BWD_PAIR = 30,    /* hdmoe_attn_bwd: the MFMA dq + dk / dv pair (Sq > 1024) */
  HDMOE_SEL_ATTN_GENERIC = 31,     /* hdmoe_attn_fwd / hdmoe_attn_bwd: the one-row-per-thread kernels (one count per call) */
  HDMOE_SEL_FUSION_MID = 32,       /* hdmoe_fusion_mid_fwd: cross_attn.out_proj with its residual + cross_attn_text.q_proj in one launch */
  HDMOE_SEL_FUSION_MID_BWD = 33,   /* hdmoe_fusion_mid_bwd: their input gradients, the gradient fan-in of a and both weight gradients */
  HDMOE_SEL_COUNT = 34
};
int hdmoe_kernel_selections(long long* counts, int n, int reset);

/* Which kernel a layer gets: the library is the only place that decides, these queries ask it.  Nothing is launched or counted.
 * aligned16 stands for the pointer tests: != 0 = every tensor of the call 16-byte aligned, 0 = 4-byte aligned only.  has_seg / has_res:
 * the call passes a seg array / a residual.
 * hdmoe_conv_fwd_route: the walk hdmoe_conv_fwd itself makes for the same arguments (dtype HDMOE_F32S included).  route = HOST array of
 * 5 ints {HDMOE_ROUTE_CONV_*, then the template arguments of the instantiation, 0 in the slots the family does not use}:
 *   CONV7: CO, KMASK, W16    CONV6: MT, NT    CONV6S: NT    KGEMM: NT    GLIN: NJ    ROWLIN: outputs per tile    FWD / FWD2 / FWD3 / FWD5: NT (conv_fwd_kernel: NB), VEC, LEPI, NHR
 * HDMOE_ROUTE_CONV_NONE is an answer, not an error: nothing would run (an HDMOE_F32S layer outside conv6s's domain, which hdmoe_conv_fwd
 * refuses with HDMOE_EINVAL; an empty batch).
 * hdmoe_conv_generic_route: the generic tail of that walk alone (conv_fwd_plan), whether or not a specialised kernel would take the layer;
 * the same 5 ints, always one of FWD / FWD2 / FWD3 / FWD5.
 * hdmoe_conv_wgrad_route: route = HOST array of 34 ints {HDMOE_ROUTE_WGRAD_*, nclasses, then per kernel-size class in launch order
 * (passes, MAXT, OT, VEC)}; nclasses = 0 unless conv_wgrad2_kernel runs. */
enum {
  HDMOE_ROUTE_CONV_FWD = 0,   /* conv_fwd_kernel<T, NB, VEC> */
  HDMOE_ROUTE_CONV_FWD2 = 1,  /* conv_fwd2_kernel<T, NT, VEC> */
  HDMOE_ROUTE_CONV_FWD3 = 2,  /* conv_fwd3_kernel<T, NT> */
  HDMOE_ROUTE_CONV_FWD5 = 3,  /* conv_fwd5_kernel<T, NT, LEPI, NHR> */
  HDMOE_ROUTE_CONV_CONV7 = 4, /* conv7_kernel<CO, KMASK, W16, DBG> (csrc/conv7.hip) */
  HDMOE_ROUTE_CONV_CONV6 = 5, /* conv6_bf16_kernel<MT, NT> (csrc/conv6.hip) */
  HDMOE_ROUTE_CONV_CONV6S = 6,/* conv6_split_kernel<NT> (csrc/conv6s.hip) */
  HDMOE_ROUTE_CONV_KGEMM = 7, /* kgemm_kernel<NT> (csrc/kgemm.hip) */
  HDMOE_ROUTE_CONV_GLIN = 8,  /* glin_f32_kernel<NJ> (csrc/mlinear.hip) */
  HDMOE_ROUTE_CONV_NONE = 9,  /* no kernel */
  HDMOE_ROUTE_CONV_ROWLIN = 10, /* rowlin_f32_kernel, route[1] = outputs per tile (csrc/rowlin.hip) */
  HDMOE_ROUTE_WGRAD_V2 = 0,   /* conv_wgrad2_kernel<T, OT, MAXT, VEC>, one launch per class and pass */
  HDMOE_ROUTE_WGRAD_V1 = 1,   /* conv_wgrad_kernel<T> */
  HDMOE_ROUTE_WGRAD_SWG = 2,  /* swg_f32_kernel (csrc/lwgrad.hip) */
  HDMOE_ROUTE_WGRAD_TOWG = 3, /* towg_bf16_kernel */
  HDMOE_ROUTE_WGRAD_LWG = 4   /* lwg_f32_kernel / lwg_bf16_kernel */
};
int hdmoe_conv_fwd_route(int* route, int N, int H, int W, int Ho, int Wo, int Cin, int Cphys, int Ipad, int Cout, int Cstore, int stride, int ones,
                         int ngroups, int has_seg, int has_res, long wstride, const int* kh, const int* kw, const int* pt, const int* pl,
                         int dtype, int aligned16);
int hdmoe_conv_generic_route(int* route, int N, int H, int W, int Ho, int Wo, int Cin, int Cphys, int Ipad, int Cout, int Cstore, int stride,
                             int ones, int ngroups, const int* kh, const int* kw, int dtype, int aligned16);
int hdmoe_conv7_min_images(void);   /* least number of images of a layer that conv7 (and the fused backward on it) takes */
int hdmoe_conv_wgrad_route(int* route, int N, int H, int W, int Ho, int Wo, int Cin, int Cphys, int Cout, int stride, int ones, int ngroups,
                           int has_seg, const int* kh, const int* kw, const int* pt, const int* pl, int dtype, int aligned16);

/* Multi-tensor weight bank: one prep launch per forward and one gradient-finish launch per backward for ALL MP_Conv weights
 * of a model.  descs: device array of descriptors (layout = hdmoe_wbank_desc_bytes() bytes each, see csrc/wbank.hip);
 * rows: device int32 pairs (descriptor index, output-channel row), one workgroup per pair. */
int hdmoe_wbank_desc_bytes(void);
int hdmoe_wbank_prep(const void* descs, const int* rows, int nrows, int mutate, HS stream);
int hdmoe_wbank_bwd(const void* descs, const int* rows, int nrows, HS stream);

/* ---- K4/K7: pointwise, broadcast, relayout  (model_internals.py:33-127, model_components.py:232-253) ----- */
int hdmoe_axpby(void* out, const void* x, const void* y, float a, float b, long n, int dtype, HS stream);      /* a*x + b*y (y may be NULL) : mp_sum */
int hdmoe_sum_n(void* out, const void* const* srcs, const float* src_scale, int n, long nelem, int dtype, HS stream);   /* sum_k src_scale[k] * srcs[k], n <= 16 tensors (16-byte aligned), src_scale = host array or NULL (all 1): fan-out backward */
int hdmoe_affine(void* out, const void* x, float a, float c, long n, int dtype, HS stream);                     /* a*x + c */
int hdmoe_mul(void* out, const void* x, const void* y, long n, int dtype, HS stream);
/* One Heun stage of the EDM sampler with the sigma schedule on the device (reference Utils/EDM_sampler.py:90-107): t = float64 [N + 1] device
 * array, idx = device int32 stage counter.  sched_pick: *sigma = t[*idx + off];  heun_euler: x_next = x_hat + (t[i+1] - t[i]) (x_hat - den) / t[i];
 * heun_correct: out = x_hat + h (0.5 (x_hat - den) / t[i] + 0.5 (x_next - den2) / t[i+1]);  idx_advance: *idx += 1.  fp32 latents of n elements.
 * Known region (inpainting): x0, noise, mask = fp32 arrays of n elements each, either all NULL (exactly the update above) or all set, in which
 * case heun_euler / heun_correct end with the epilogue  x <- mask (x0 + s noise) + (1 - mask) x  at s = (float) t[i+1], in that form
 * (mask = 1 at s = 0 returns x0, mask = 0 returns x, bit-for-bit).  In-place calls (out == x_hat) are allowed.
 * known_blend: the same blend with a host scalar s, in place on x (x, x0, noise in dtype; mask fp32): the host-driven sampler loop.
 * dpm2m_step: one DPM-Solver++(2M) stage (one evaluation per stage; i = *idx, i0 = *i0 = the first stage run, a = t[i+1] / t[i]):
 * t[i+1] == 0: x_out = den;  i == i0: x_out = a x + (1 - a) den;  else, with r = log(t[i-1] / t[i]) / log(t[i] / t[i+1]),
 * x_out = a x + (1 - a) ((1 + 1/(2r)) den - 1/(2r) den_prev);  then the known-region epilogue as above (all NULL or all set), and
 * den_prev <- den in the same pass (den_prev is read before it is written, element by element).  x_out == x is allowed; den_prev must
 * not overlap x_out, x or den.  HDMOE_EINVAL for a NULL required pointer, n < 0, a partial known block or an overlapping den_prev.
 * Stochastic stages.  Stage i draws one standard normal per latent element: eps[j] is the value hdmoe_randn(out, seed = *seed,
 * *seed_dev = i, scale = 1, n) writes to out[j] (Philox block j / 4, key *seed + i * 0x9E3779B97F4A7C15), whatever the alignment, the vector
 * width or n % 4.  seed = device word, i = *idx: nothing random is a launch scalar, so a captured stage replays with fresh noise.
 * heun_churn (reference :90-97): tc = t[i], gamma = gamma_cap if s_min <= tc <= s_max else 0, *t_hat = tc + gamma tc (double),
 * *sigma = (float) *t_hat (it stands in for sched_pick(.., 0)), x_hat = x + c eps with c = (float)(sqrt(t_hat^2 - tc^2) s_noise).  gamma == 0:
 * x_hat = x bit-for-bit, nothing is drawn.  x_hat == x is allowed.  HDMOE_EINVAL for a NULL pointer, n < 0, a negative or non-finite
 * gamma_cap or s_noise, a NaN s_min or s_max.
 * heun_euler_hat / heun_correct_hat: heun_euler / heun_correct with t_hat = *t_hat (non-NULL) in place of t[i]; t[i+1] and the blend stay.
 * dpm2m_sde_step: DPM-Solver++(2M) SDE, midpoint form.  dpm2m_step with h = log(t[i] / t[i+1]), e = exp(-eta h), a = (t[i+1] / t[i]) e,
 * b = 1 - a (double, each rounded to float once): t[i+1] == 0: x_out = den;  i <= i0: x_out = a x + b den;  else
 * x_out = a x + b ((1 + 1/(2r)) den - 1/(2r) den_prev);  then, if eta > 0 and t[i+1] != 0, x_out += c eps with
 * c = (float)(t[i+1] sqrt(1 - e^2) s_noise);  then the known-region epilogue and den_prev <- den.  eta == 0 is dpm2m_step bit-for-bit.
 * The rules of dpm2m_step apply; also HDMOE_EINVAL for a NULL seed and a negative or non-finite eta or s_noise. */
int hdmoe_sched_pick(float* sigma, const double* t, const int* idx, int off, HS stream);
int hdmoe_idx_advance(int* idx, HS stream);
int hdmoe_heun_euler(float* xn, const float* xh, const float* den, const double* t, const int* idx, long n,
                     const float* x0, const float* noise, const float* mask, HS stream);
int hdmoe_heun_correct(float* out, const float* xh, const float* den, const float* xn, const float* den2, const double* t, const int* idx, long n,
                       const float* x0, const float* noise, const float* mask, HS stream);
int hdmoe_known_blend(void* x, const void* x0, const void* noise, const float* mask, float s, long n, int dtype, HS stream);
int hdmoe_dpm2m_step(float* x_out, const float* x, const float* den, float* den_prev, const double* t, const int* idx, const int* i0, long n,
                     const float* x0, const float* noise, const float* mask, HS stream);
int hdmoe_heun_churn(float* x_hat, const float* x, float* sigma, double* t_hat, const double* t, const int* idx, const unsigned long long* seed,
                     double gamma_cap, double s_min, double s_max, double s_noise, long n, HS stream);
int hdmoe_heun_euler_hat(float* xn, const float* xh, const float* den, const double* t, const int* idx, const double* t_hat, long n,
                         const float* x0, const float* noise, const float* mask, HS stream);
int hdmoe_heun_correct_hat(float* out, const float* xh, const float* den, const float* xn, const float* den2, const double* t, const int* idx,
                           const double* t_hat, long n, const float* x0, const float* noise, const float* mask, HS stream);
int hdmoe_dpm2m_sde_step(float* x_out, const float* x, const float* den, float* den_prev, const double* t, const int* idx, const int* i0, long n,
                         const float* x0, const float* noise, const float* mask, float eta, float s_noise, const unsigned long long* seed,
                         HS stream);
/* Tiled sampling (csrc/tiles.hip): a (B, C, H, W) latent larger than the model's (h, w) is evaluated on Ty x Tx overlapping model-sized
 * windows and the outputs are blended back.  All tensors fp32 NCHW.  oy[Ty] / ox[Tx]: int32 DEVICE arrays of the tile origins along y / x
 * (0 <= origin <= H - h / W - w; the kernels clamp an origin into that range, so no access leaves a tensor whatever the arrays hold).
 * Tile-batch row r = (b Ty + ky) Tx + kx is tile (ky, kx) of sample b.
 * tile_gather: tiles[0 .. rows) <- rows row0 .. row0 + rows - 1 of the tile batch, cropped out of x: tiles[r - row0][c][i][j] =
 * x[b][c][oy[ky] + i][ox[kx] + j], an exact copy.
 * tile_blend: ny[Ty][H] / nx[Tx][W]: fp32 DEVICE tables of the normalised 1-D window weights, zero where the tile does not cover the
 * position.  out[b][c][y][x] = sum over ky ascending, kx ascending within it, of fl(ny[ky][y] nx[kx][x]) tiles[(b Ty + ky) Tx + kx][c][y - oy[ky]][x - ox[kx]]:
 * one fp32 product for the weight, then fma accumulation in that order from -0 (so one covering tile of weight 1 returns its value bit for
 * bit).  Tiles that do not cover the position and terms of weight zero are skipped.  Every output element is written once, by one lane:
 * no atomics, no zero-fill, deterministic.
 * 16-byte accesses when W, w and every x origin are multiples of 4 and the pointers are aligned (four consecutive x then lie wholly inside
 * or outside any tile; the origins are read on the device, the kernel picks the arm), else element by element.
 * HDMOE_EINVAL, nothing launched: a NULL pointer, a size < 1, h > H or w > W, Ty or Tx outside [1, HDMOE_TILE_MAX_AXIS]; tile_gather also
 * row0 < 0, rows < 1, row0 + rows > B Ty Tx. */
#define HDMOE_TILE_MAX_AXIS 32
int hdmoe_tile_gather(float* tiles, const float* x, const int* oy, const int* ox, int B, int C, int H, int W, int h, int w, int Ty, int Tx,
                      long row0, long rows, HS stream);
int hdmoe_tile_blend(float* out, const float* tiles, const int* oy, const int* ox, const float* ny, const float* nx, int B, int C, int H, int W,
                     int h, int w, int Ty, int Tx, HS stream);
/* Measurement aid: `blocks` x 256 threads, 8 x `iters` dependent v_exp_f32 per thread (out: blocks * 256 floats).  bench.py times it to state the
 * transcendental issue rate the attention kernels (reference models/model_internals.py:374-404: one exp per score) are bounded by. */
int hdmoe_exp_rate(float* out, int blocks, int iters, HS stream);
int hdmoe_cast(void* out, const void* x, long n, int dt_in, int dt_out, HS stream);
/* Separable even-length FIR resampling, channel-last (resample(x, f, mode) for f other than [1, 1]; reference models/model_internals.py:95-127):
 * up == 0: stride-2 depthwise correlation with outer(k, k) and padding `pad` (F.conv2d there); up == 1: its transpose (F.conv_transpose2d).
 * taps: L <= 8 host floats.  Each direction is the other's backward. */
int hdmoe_fir_resample(void* y, const void* x, const float* taps, int L, int pad, float scale, int up, int N, int H, int W, int Ho, int Wo, int C,
                       int dtype, HS stream);
int hdmoe_mp_silu_fwd(void* out, const void* x, long n, int dtype, HS stream);
int hdmoe_mp_silu_bwd(void* dx, const void* dy, const void* x, long n, int dtype, HS stream);
/* fused decoder-block entry (model_components.py:232-253): the block input feeds mp_silu AND the skip / residual path */
int hdmoe_mp_silu_bwd_add(void* dx, const void* dy, const void* x, const void* gx, float sx, long n, int dtype, HS stream);   /* dx = sx * gx + dy * mp_silu'(x) */
int hdmoe_cat2_silu_fwd(void* out, void* out_h, const void* a, const void* b, float wa, float wb, int Ca, int Cb, long rows,
                        int dtype, HS stream);                                                                     /* out = mp_cat, out_h = mp_silu(out) */
int hdmoe_cat2_silu_bwd(void* da, void* db, const void* gcat, const void* gh, const void* xcat, float wa, float wb, int Ca,
                        int Cb, long rows, int dtype, HS stream);
int hdmoe_sigmoid_fwd(void* out, const void* x, float a, long n, int dtype, HS stream);                         /* sigmoid(a*x) */
int hdmoe_sigmoid_bwd(void* dx, const void* dy, const void* y, float a, long n, int dtype, HS stream);
int hdmoe_film_silu_fwd(void* out, const void* u, const float* e, int N, long HW, int C, int dtype, HS stream);  /* mp_silu(u * e[n][c]) */
int hdmoe_film_silu_bwd(void* du, float* de, const void* da, const void* u, const float* e, int N, long HW, int C,
                        int dtype, HS stream);                                                                   /* de accumulates */
int hdmoe_film_silu_drop_fwd(void* out, const void* u, const float* e, int N, long HW, int C, unsigned long long seed,
                             const unsigned long long* seed_dev, float p, int dtype, HS stream);                  /* + F.dropout fused (:245-246) */
int hdmoe_film_silu_drop_bwd(void* du, float* de, const void* da, const void* u, const float* e, int N, long HW, int C,
                             unsigned long long seed, const unsigned long long* seed_dev, float p, int dtype, HS stream);
/* The same with the keep decisions saved by the forward (bf16 only): mask [N][HW][C/8] bytes, bit j = element j of the 16-byte vector kept.
 * out / du are bit-identical to the drop_fwd / drop_bwd pair; the backward reads the byte instead of drawing the Philox words again. */
int hdmoe_film_silu_drop_fwd_mask(void* out, unsigned char* mask, const void* u, const float* e, int N, long HW, int C,
                                  unsigned long long seed, const unsigned long long* seed_dev, float p, int dtype, HS stream);
int hdmoe_film_silu_mask_bwd(void* du, float* de, const void* da, const void* u, const float* e, const unsigned char* mask, int N,
                             long HW, int C, float p, int dtype, HS stream);
int hdmoe_scale_rows_fwd(void* out, const void* x, const float* s, long rows, long L, int dtype, HS stream);    /* out[r][:] = s[r]*x[r][:] */
int hdmoe_scale_rows_bwd(void* dx, float* ds, const void* dy, const void* x, const float* s, long rows, long L,
                         int dtype, HS stream);                                                                  /* dx and/or ds (accumulates) */
int hdmoe_cat2_fwd(void* out, const void* a, const void* b, float wa, float wb, int Ca, int Cb, long rows, int dtype, HS stream); /* mp_cat */
int hdmoe_cat2_bwd(void* da, void* db, const void* dout, float wa, float wb, int Ca, int Cb, long rows, int dtype, HS stream);
int hdmoe_pool2(void* out, const void* x, int N, int Ho, int Wo, int C, float scale, int dtype, HS stream);      /* resample 'down' (scale .25) / bwd of 'up' (1) */
int hdmoe_upsample2(void* out, const void* x, int N, int Ho, int Wo, int C, float scale, int dtype, HS stream);  /* resample 'up' (1) / bwd of 'down' (.25) */
int hdmoe_seq_reduce(float* out, const void* x, int N, long S, int C, float scale, int dtype, HS stream);        /* out[n][c] += scale*sum_s x[n][s][c] */
int hdmoe_seq_bcast_add(void* out, const void* x, const float* t, int N, long S, int C, float scale, int dtype, HS stream);
int hdmoe_bias_add(void* out, const void* x, const float* bias, long rows, long L, int dtype, HS stream);
int hdmoe_colsum(float* out, const void* dy, long rows, long L, int dtype, HS stream);                          /* accumulates */
int hdmoe_lerp_param_fwd(void* out, const void* a, const void* b, const float* alpha, long n, int dtype, HS stream);   /* model_config2.py:291 */
int hdmoe_lerp_param_bwd(void* da, void* db, float* dalpha, const void* g, const void* a, const void* b,
                         const float* alpha, long n, int dtype, HS stream);
int hdmoe_gate_mix_fwd(void* out, float* gate, const void* logits, const void* U, const void* A, long rows, int C,
                       int dtype, HS stream);                                                                    /* model_config2.py:297-301 */
int hdmoe_gate_mix_bwd(void* dU, void* dA, void* dlogits, const void* dout, const float* dgate, const float* gate,
                       const void* U, const void* A, long rows, int C, int dtype, HS stream);
int hdmoe_softmax_rows_fwd(float* out, const float* x, long rows, int C, float scale, HS stream);               /* model_components.py:64 */
int hdmoe_softmax_rows_bwd(float* dx, const float* dy, const float* y, long rows, int C, float scale, HS stream);
int hdmoe_nchw_to_nhwc(void* out, const float* x, const float* s, int N, int C, long HW, int dtype, HS stream);  /* + per-sample scale (c_in) */
int hdmoe_nhwc_to_nchw(float* out, const void* F, const float* sf, const float* x, const float* sx, int N, int C,
                       long HW, int dtype, HS stream);                                                           /* sf*F + sx*x : D_x, model_config2.py:449 */
/* guided egress: F is the head output of the pair-stacked batch [conditional rows 0..N-1 ; unconditional rows N..2N-1] (NHWC);
 * out[n] = sx[n] x[n] + sf[n] ((1 - g) F[N + n] + g F[n]) -- the EDM egress and the classifier-free-guidance lerp in one pass */
int hdmoe_nhwc_to_nchw_guided(float* out, const void* F, const float* sf, const float* x, const float* sx, float g, int N,
                              int C, long HW, int dtype, HS stream);
/* the same with one scale per sample, g[0..N-1] in DEVICE memory: out[n] = sx[n] x[n] + sf[n] ((1 - g[n]) F[N + n] + g[n] F[n]).  A constant
 * vector gives the bits of the scalar entry point; the values are not checked (the caller validates them on the host). */
int hdmoe_nhwc_to_nchw_guided_rows(float* out, const void* F, const float* sf, const float* x, const float* sx, const float* g, int N,
                                   int C, long HW, int dtype, HS stream);
/* out[r][:] = (1 - g[r]) ref[r][:] + g[r] d[r][:], g[0..rows-1] in DEVICE memory, rows of `per` elements: the guidance blend of two
 * denoiser outputs with one scale per sample.  16-byte accesses when per is a multiple of the vector width (8 bf16 / 4 fp32) and the
 * pointers are aligned -- a vector never holds elements of two rows -- else element by element.  A constant vector gives the bits of
 * hdmoe_axpby(out, ref, d, 1 - g, g) where both take the same path (always, when per is a multiple of the vector width). */
int hdmoe_lerp_rows(void* out, const void* ref, const void* d, const float* g, long rows, long per, int dtype, HS stream);
/* Guidance combine: rescale and projected guidance (APG) in one launch, one workgroup per sample, all sums over the sample's `per` elements.
 * With D_c = d[n], D_u = ref[n], w = g_rows ? g_rows[n] : g (g_rows: DEVICE memory or NULL):
 *   M   = (D_c - D_u) + beta M_prev                       fp32; M_prev = momentum[n] (fp32, read and overwritten by M); beta == 0: the
 *                                                         buffer is neither read nor written and may be NULL, beta != 0 needs it
 *   S1 = sum M^2, S2 = sum M D_c, S3 = sum D_c^2, T1 = sum D_c, T2 = sum M          accumulated in fp64
 *   s   = sqrt(S1) > r ? r / sqrt(S1) : 1;   c = S3 == 0 ? 0 : S2 / S3;   b = (w - 1) s;   a = 1 - b (1 - eta) c               (fp64)
 *   rho = sqrt(var(D_c) / var(a D_c + b M)) from the five sums, 1 when a variance is <= 0;   f = phi rho + (1 - phi)            (fp64)
 *   out = fl(f a) D_c + fl(f b) M                         fp32, rounded once to the output dtype
 * eta = 1, r = inf, beta = 0, phi = 0 is (1 - w) D_u + w D_c.  Samples of at most HDMOE_GUIDE_COMBINE_RESIDENT elements stay in registers
 * across the reduction (every operand read once); larger ones re-read their operands after it.  16-byte accesses when per is a multiple
 * of the vector width and the pointers are aligned, else element by element.  dtype: of ref, d and out (fp32 / bf16). */
#define HDMOE_GUIDE_COMBINE_RESIDENT 16384
int hdmoe_guide_combine(void* out, const void* ref, const void* d, float g, const float* g_rows, float eta, float r, float beta, float phi,
                        float* momentum, long rows, long per, int dtype, HS stream);
/* The same on the pair-stacked head output F (2N, H, W, C) of the shared-routing pass: D_c = sx[n] x[n] + sf[n] F[n] and
 * D_u = sx[n] x[n] + sf[n] F[N + n] are formed in registers and never written; out and momentum are fp32 NCHW, per = C HW.  dtype: of F. */
int hdmoe_nhwc_to_nchw_guide_combine(float* out, const void* F, const float* sf, const float* x, const float* sx, float g, const float* g_rows,
                                     float eta, float r, float beta, float phi, float* momentum, int N, int C, long HW, int dtype, HS stream);
/* Composed guidance: K conditions D_1 .. D_K (1 <= K <= HDMOE_COMPOSE_MAX) with weights a[n][k] (fp32, DEVICE memory, (rows, K), any
 * sign) and optional masks m[n][k][p] (fp32 in [0, 1], DEVICE memory, (rows, K, HW) over the HW latent positions, broadcast over
 * channels: per = C HW, element e = c HW + p; NULL = no masks) become ONE conditional operand in registers, per element, in fp32, with
 * contraction off and left to right:
 *   c_k = a[n][k] m[n][k][p]                              (no masks: c_k = a[n][k], no multiplication)
 *   c_0 = (((1 - c_1) - c_2) - ...) - c_K
 *   D_c = (((c_0 D_u) + c_1 D_1) + c_2 D_2) + ... + c_K D_K          i.e. D_u + sum_k c_k (D_k - D_u)
 * D_c and D_u then enter the steps of hdmoe_guide_combine above unchanged (same kernel body): M = (D_c - D_u) + beta M_prev, the five
 * fp64 sums, s / c / b / a / rho / f, out = fl(f a) D_c + fl(f b) M.  K = 1, a = 1, no masks: c_0 = 0 and D_c = D_1 (finite D_u), the
 * output has the bits of hdmoe_guide_combine / hdmoe_nhwc_to_nchw_guide_combine with the same launch scalars.  w = 1, eta = 1, r = inf,
 * beta = 0, phi = 0: out = D_c exactly.  On the re-read arm D_c is formed a second time by the same fp32 operations, as M is.  The
 * values of a and m are not checked (the caller validates them on the host).  16-byte accesses under the conditions of the parent entry
 * point and, with masks, HW a multiple of the vector width and m aligned (a vector's mask values are then one load); else element by
 * element (hdmoe_guide_compose: element by element always re-reads, whatever the sample's size).  HDMOE_EINVAL, nothing launched: K out of range, a NULL, a NULL entry of d_ptrs, masks with HW < 1 or per % HW != 0, and
 * whatever the parent refuses.  HW is not read without masks.
 * d_ptrs: HOST array of K DEVICE pointers to (rows, per) tensors of `dtype` (fp32 / bf16), like ref and out. */
#define HDMOE_COMPOSE_MAX 8
int hdmoe_guide_compose(void* out, const void* ref, const void* const* d_ptrs, int K, const float* a, const float* m, long HW, float g,
                        const float* g_rows, float eta, float r, float beta, float phi, float* momentum, long rows, long per, int dtype,
                        HS stream);
/* The same as the egress of the shared-routing pass: F (NHWC, `dtype`) is the head output of the variant-stacked batch of (K + 1) N rows,
 * rows k N .. k N + N - 1 belong to condition k + 1 and the last N rows are unconditional (K = 1: the pair stacking above).
 * D_k = sx[n] x[n] + sf[n] F[k N + n] and D_u = sx[n] x[n] + sf[n] F[K N + n] are formed in registers as
 * hdmoe_nhwc_to_nchw_guide_combine forms its two operands, and never written; out and momentum are fp32 NCHW, m is (N, K, HW). */
int hdmoe_nhwc_to_nchw_compose(float* out, const void* F, const float* sf, const float* x, const float* sx, int K, const float* a, const float* m,
                               float g, const float* g_rows, float eta, float r, float beta, float phi, float* momentum, int N, int C, long HW,
                               int dtype, HS stream);
int hdmoe_patch_relayout(void* out, const void* in, int N, int H, int W, int C, int p, int hp, int wp, int order,
                         int to_img, int dtype, HS stream);                                                      /* PixelShuffle / patchify */
/* The same bytes for order 1 (PixelShuffle) by a tiled transpose through LDS, 16-byte accesses on both sides (csrc/relayout.hip).
 * Returns 1 and launches nothing outside its domain -- order 0, p or C not a multiple of the 16-byte vector width (8 bf16 / 4 fp32),
 * a token above 32 KiB, p > 64, unaligned pointers: the caller then runs hdmoe_patch_relayout. */
int hdmoe_patch_relayout_tiled(void* out, const void* in, int N, int H, int W, int C, int p, int hp, int wp, int order,
                               int to_img, int dtype, HS stream);
/* Row-windowed forms for the edges of the ViT expert bank (patch embedding in, un-patching out), where expert g owns the contiguous
 * rows [seg[g], seg[g+1]) of the routed batch.  rows: DEVICE pointer to two ints {begin, end} (in the bank: seg + g), read by the
 * kernel, never by the host: the launch always has the all-rows grid, so a captured graph follows the routing of each replay.  Rows
 * inside the window get exactly what the all-rows entry point writes for them; no other row is read or written; an empty window
 * does nothing.  (Weight gradients over a window: hdmoe_conv_wgrad / hdmoe_pw_bwd with seg = rows and one group.) */
int hdmoe_patch_relayout_rows(void* out, const void* in, const int* rows, int N, int H, int W, int C, int p, int hp, int wp, int order,
                              int to_img, int dtype, HS stream);
int hdmoe_patch_relayout_tiled_rows(void* out, const void* in, const int* rows, int N, int H, int W, int C, int p, int hp, int wp,
                                    int order, int to_img, int dtype, HS stream);                               /* 1: declined, as the all-rows form */
int hdmoe_bias_add_rows(void* out, const void* x, const float* bias, const int* rows, int N, long S, long L, int dtype, HS stream);   /* [N][S][L] */
int hdmoe_colsum_rows(float* out, const void* dy, const int* rows, int N, long S, long L, int dtype, HS stream);                      /* accumulates */
/* pointwise forward / dgrad y = alpha * x w^T of one group over the row window, w = the [Cout][Ipad] image of hdmoe_wprep_fwd; flat != 0:
 * the positions as one long row (full tiles), as ops.mp_conv presents a linear layer.  Same kernels as hdmoe_conv_fwd runs for the layer
 * (kgemm with the window in positions, conv_fwd5, the generic per-row kernels).  1: declined (not bf16), nothing launched. */
int hdmoe_pw_fwd_rows(const void* x, const void* w, void* y, float alpha, const int* rows, int N, int H, int W, int Cin, int Ipad,
                      int Cout, int flat, int dtype, HS stream);
int hdmoe_fourier(float* out, const float* x, const float* freqs, const float* phases, int B, int F, HS stream); /* model_internals.py:171-174 */
int hdmoe_edm_coeffs(float* coef, const float* sigma, int nsig, float sigma_data, int B, HS stream);             /* model_config2.py:431-438 */
int hdmoe_sigmoid_scaling(float* sv, float* su, float* pair, const float* c_noise, float tp, float soft, int B, HS stream); /* :244-249 */
int hdmoe_adaln_fwd(float* out, const float* x, const float* cond, long B, int F, HS stream);                   /* model_components.py:148-151 */
int hdmoe_adaln_bwd(float* dx, float* dcond, const float* g, const float* x, const float* cond, long B, int F, HS stream);
int hdmoe_take_col_pos_fwd(float* out, const float* w, long B, int E, int e, HS stream);                         /* w[:,e] where > 0 (model_config1.py:26,35) */
int hdmoe_take_col_pos_bwd(float* dw, const float* g, const float* w, long B, int E, int e, HS stream);          /* dw pre-zeroed */
/* Philox key = seed + (*seed_dev) * golden (seed_dev: optional device step counter, so captured graphs replay with fresh draws) */
int hdmoe_dropout(void* out, const void* x, unsigned long long seed, const unsigned long long* seed_dev, float p, long n, int dtype,
                  HS stream);                                                                                    /* F.dropout, model_components.py:245-246 */
int hdmoe_randn(float* out, unsigned long long seed, const unsigned long long* seed_dev, float scale, long n, HS stream); /* randn*zeta, :155-156 */
/* randn_ds: hdmoe_randn with the scale read from device memory (*scale, fp32): bit for bit what hdmoe_randn writes for scale = *scale,
 * and a captured launch follows a scale that changes between replays.  HDMOE_EINVAL for a NULL out / scale or n < 0. */
int hdmoe_randn_ds(float* out, unsigned long long seed, const unsigned long long* seed_dev, const float* scale, long n, HS stream);
int hdmoe_seed_advance(unsigned long long* seed_dev, HS stream);

/* ---- training inputs of one step, made on the device  (csrc/traingen.hip; reference Utils/utils.py:26-61, 228-330, training.py:125-135) ----
 * One call per step, two launches: a one-workgroup kernel (sigma, shuffle, both router masks, zeta) and a 16-byte-access noising kernel.
 * Every output goes to a caller-owned static buffer, nothing is read back by the host, so the buffers can feed captured graphs.
 *   sigma (B) , src (B, int32), unet_mask / vit_mask (B, E) fp32 0/1, zeta_out (1), x (B, chw) = x0 + sigma[b] eps
 * RNG contract.  Every draw is Philox4x32-10 under the key hdmoe_randn(seed = seed, *seed_dev = 4 step + r) uses, i.e.
 * seed + (4 step + r) * 0x9E3779B97F4A7C15 (mod 2^64); value s of a stream is lane s % 4 of Philox block s / 4:
 *   r = 0  eps: element j of eps (flat over (B, chw)) is element j of hdmoe_randn(.., scale = 1) under that key, whatever chw % 4 is;
 *   r = 1  z_s: element s of hdmoe_randn under that key (the log-normal draws);
 *   r = 2  u_s = u01(word s) (the log-uniform draws);      r = 3  k_i = u01(word i) (the shuffle keys).
 * Nothing reads torch's generator or the library's seed stream; (seed, step) alone fix the outputs.
 * Semantics.  n_ln = (int)(B (1 - extreme_prob)) in double.  Pre-shuffle value s is exp(p_mean + p_std z_s) for s < n_ln and
 * exp(ln sigma_min + u_s (ln sigma_max - ln sigma_min)) otherwise, clamped to [sigma_min, sigma_max].  src[i] = the rank of k_i among the B
 * keys (ties: the lower position first), a permutation of 0 .. B-1; sigma[i] = value src[i].  Masks, per router with its centers (E) and
 * bandwidth: pct = clamp(0.5 (1 + erf((ln sigma - p_mean) / (p_std sqrt 2))), 0, 1), dist_e = |pct - center_e|, mask = dist_e <= bw, and the
 * min_active nearest experts (ties: the lower index) are 1 in any case.  *zeta_out = zeta.
 * HDMOE_EINVAL: a NULL pointer, B < 1 or B > 4096, chw < 1, E < 1 or E > 8, min_active < 0 or > E, sigma_min <= 0 or sigma_max < sigma_min,
 * extreme_prob outside [0, 1].  x / x0 16-byte aligned with chw % 4 == 0 take the 16-byte path, anything else the scalar one. */
int hdmoe_train_inputs(float* x, float* sigma, float* unet_mask, float* vit_mask, float* zeta_out, int* src, const float* x0,
                       const float* unet_centers, const float* vit_centers, unsigned long long seed, unsigned long long step, long B, long chw,
                       int E, int min_active, double sigma_min, double sigma_max, double p_mean, double p_std, double extreme_prob,
                       double unet_bw, double vit_bw, float zeta, HS stream);
/* Text-conditioning dropout of one step, for classifier-free guidance: row i of out (B rows of `row` elements of elem_bytes = 4 or 2
 * bytes -- the kernel moves bytes, so fp32 / bf16 / fp16; a row is everything behind the batch dimension) is row i of text when
 * keep[i] == 1 and null_row (one row; NULL: zeros) otherwise; keep (B) fp32 holds 0 / 1.  One launch over the whole device: the copy
 * of the text into its static buffer with the substitution folded in.
 * RNG contract (continued).  The drop draw of sample i is d_i = u01(word i % 4 of Philox4x32-10 block (c0 = i / 4, c1 = 1)) under the
 * key of the r = 3 stream of that step, seed + (4 step + 3) * 0x9E3779B97F4A7C15; the shuffle keys k_i are the same key's blocks with
 * c1 = 0, so no existing draw changes and no counter 4 step + r is reused.  Sample i is dropped iff d_i < (float)p; u01 > 0, so p = 0
 * drops nothing, and p = 1 drops everything but a sample whose 24-bit word is 2^24 - 1 (its + 0.5f rounds u01 to 1.0f in fp32: one draw
 * in 2^24).  (seed, step) alone fix the result.
 * row * elem_bytes % 16 == 0 with out / text / null_row 16-byte aligned takes the 16-byte path, anything else moves elements.
 * HDMOE_EINVAL: NULL out / keep / text, B < 1, row < 1, elem_bytes not 2 or 4, p outside [0, 1] or NaN, out == text. */
int hdmoe_text_dropout(void* out, float* keep, const void* text, const void* null_row, unsigned long long seed, unsigned long long step,
                       long B, long row, int elem_bytes, double p, HS stream);

/* ---- the device-resident latent dataset  (csrc/traingen.hip, csrc/keyed_perm.h; reference Utils/training.py:226-239 the shuffled
 * drop_last loader, Utils/VAE_CLIP.py:58-66 the posterior draw) ----
 * The batch of step k is a pure function of (seed, world, rank, k): which items, their posterior draw, their horizontal flip, their text.
 * Keyed permutation.  perm(seed, epoch, N, x) for 0 <= x < N, 1 <= N < 2^31: k = max(2, bit_length(N - 1)) rounded up to even, h = k / 2,
 * m = 2^h - 1, K = ((seed ^ 0xA0761D6478BD642F) + epoch * 0x9E3779B97F4A7C15) mod 2^64.  Eight Feistel rounds on (L, R) = (x >> h, x & m):
 * for r = 0..7, (L, R) <- (R, L ^ (F_r(R) & m)) with F_r(R) = word 0 of the Philox4x32-10 block (c0 = R, c1 = r) under K; y = (L << h) | R;
 * while y >= N the eight rounds are applied to y again (cycle walking: the rounds are a bijection of [0, 2^k) and the walk started inside
 * [0, N), so it comes back).  Host and device run the same function (csrc/keyed_perm.h).
 * hdmoe_dataset_perm is the host side, no device needed: out[i] = perm(seed, epoch, N, first + i) for 0 <= i < count.
 * HDMOE_EINVAL: NULL out, N < 1, N >= 2^31, first < 0, count < 0, first + count > N. */
int hdmoe_dataset_perm(int* out, unsigned long long seed, unsigned long long epoch, long N, long first, long count);
/* The step's batch.  spe = N / (B world) steps per epoch (>= 1: an incomplete last batch is dropped), epoch = step / spe, pos = step % spe,
 *   item[i] = perm(data_seed, epoch, N, pos B world + rank B + i)
 * data_seed is the run's seed before the rank is mixed in, so the ranks of a step hold disjoint slices of one epoch permutation; `seed` is
 * the rank's own (what hdmoe_train_inputs takes).  RNG contract (continued): the data streams are Philox4x32-10 under
 * (seed ^ 0xE7037ED1A0B428DB) + (4 step + r) * 0x9E3779B97F4A7C15, so no draw of hdmoe_train_inputs / hdmoe_text_dropout changes or is reused:
 *   r = 0  eps_p: element j, flat over the OUTPUT (B, chw), is element j of hdmoe_randn under that key (the posterior noise);
 *   r = 1  flip[i] = u01(word i % 4 of block (i / 4, 0)) < (float)p_flip, stored as fp32 0 / 1.
 * Outputs, with w' = flip[i] ? W - 1 - w : w, rows of mean / std_dev (N, chw) in data_dtype (HDMOE_F32 or HDMOE_BF16, converted on load):
 *   x0[i,c,h,w] = scale (mean[item[i],c,h,w'] + std_dev[item[i],c,h,w'] eps_p[i,c,h,w])      (std_dev NULL: scale mean[..], nothing drawn)
 *   x[i,..] = x0[i,..] + sigma[i] eps[i,..]
 * and sigma, eps, both masks, zeta_out, src exactly as hdmoe_train_inputs defines them for (seed, step): bit for bit.
 * Two launches: the one-workgroup per-sample kernel, which also writes item and flip, and one pass that gathers, draws, mirrors, noises and
 * writes x0 and x together.  It moves 4 elements per thread (16-byte stores, a mirrored vector read at W - 4 - w with its lanes reversed)
 * when W % 4 == 0, x / x0 are 16-byte aligned and mean / std_dev aligned to 4 of their elements; chw % 4 == 0 is not enough -- at
 * (4, 8, 6) a vector would straddle image rows -- and anything else moves single elements.  Row offsets item * chw are 64-bit.
 * HDMOE_EINVAL: what hdmoe_train_inputs rejects, a NULL x0 / item / flip / mean, x == x0, N < 1 or >= 2^31, H or W < 1, chw no multiple
 * of H W, world < 1, rank outside [0, world), B world > N, p_flip outside [0, 1] or NaN, scale NaN.  HDMOE_EDTYPE: another data_dtype. */
int hdmoe_dataset_inputs(float* x, float* x0, float* sigma, float* unet_mask, float* vit_mask, float* zeta_out, int* src, int* item, float* flip,
                         const void* mean, const void* std_dev, int data_dtype, const float* unet_centers, const float* vit_centers,
                         unsigned long long seed, unsigned long long data_seed, unsigned long long step, long B, long chw, long N, int H, int W,
                         int world, int rank, double scale, double p_flip, int E, int min_active, double sigma_min, double sigma_max,
                         double p_mean, double p_std, double extreme_prob, double unet_bw, double vit_bw, float zeta, HS stream);
/* The batch's text: hdmoe_text_dropout with row i of out taken from row t of `table` (K rows), t = text_index[item[i]] when text_index
 * (N, int32) is given, else 0 when K == 1 (one fixed prompt) and item[i] when K == N.  The drop decision and keep are hdmoe_text_dropout's
 * (same draw, same key, the same kernel with a row indirection); p = 0 is a pure gather.  item holds values in [0, N) and text_index values
 * in [0, K): the kernel follows them unchecked, the caller range-checks text_index once.
 * HDMOE_EINVAL: NULL out / keep / table / item, out == table, B, K, N or row < 1, elem_bytes not 2 or 4, p outside [0, 1] or NaN, and K
 * neither 1 nor N without a text_index. */
int hdmoe_text_gather_dropout(void* out, float* keep, const void* table, const int* text_index, const int* item, const void* null_row,
                              unsigned long long seed, unsigned long long step, long B, long K, long N, long row, int elem_bytes, double p,
                              HS stream);

/* ---- held-out evaluation on the device  (csrc/evalstats.hip; no counterpart in the reference, which measures nothing but the training
 * loss of the current batch) ----
 * hdmoe_eval_inputs: one evaluation batch from the dataset's `mean` table ((N, chw) in data_dtype, HDMOE_F32 or HDMOE_BF16), one launch.
 * `levels` = K sigma values (device fp32).  For 0 <= i < B:
 *   item[i] = (first + i) % N,   k_i = (item[i] + round) % K,   sigma[i] = levels[k_i],   level[i] = k_i for i < count and -1 for the rows
 *   count <= i < B that pad the last batch (they carry a finite sigma and ordinary latents: the model sees nothing unusual);
 *   x0[i] = scale mean[item[i]] (the posterior mean: no draw, no flip -- the target is a function of the item alone);
 *   x[i] = x0[i] + sigma[i] eps_i, one fma per element as in hdmoe_train_inputs.
 * RNG contract (continued).  Element j of eps_i is element j of hdmoe_randn(seed = seed ^ 0x8EBC6AF09C88C6E3, *seed_dev = item[i] K + k_i,
 * scale = 1, n = chw), i.e. Philox4x32-10 under (seed ^ 0x8EBC6AF09C88C6E3) + (item[i] K + k_i) * 0x9E3779B97F4A7C15, lane j % 4 of block
 * j / 4 whatever chw % 4 is.  The key holds the item and the level and nothing else: the noise of an (item, level) pair does not depend on
 * B, the position in the batch, round, rank or step, and no draw of the training streams above changes or is reused.
 * It moves 4 elements per thread when chw % 4 == 0, x / x0 are 16-byte aligned and mean is aligned to 4 of its elements (there is no flip,
 * so a vector may straddle image rows); anything else moves single elements.  Row offsets item * chw are 64-bit.
 * HDMOE_EINVAL: a NULL pointer, x == x0, B, chw, N or K < 1, K > 64, B > 4096, N >= 2^31, count < 0 or > B, first < 0, round < 0, scale
 * NaN.  HDMOE_EDTYPE: another data_dtype.  Nothing is written on error. */
int hdmoe_eval_inputs(float* x, float* x0, float* sigma, int* level, int* item, const void* mean, int data_dtype, const float* levels,
                      unsigned long long seed, int round, long first, long count, long B, long chw, long N, int K, double scale, HS stream);
/* hdmoe_eval_accumulate: acc (K, F) doubles, F = 6 + 4 E, += the statistics of one batch.  Row k sums over the samples with level[i] == k:
 *   [ n, mse, mse^2, w mse, mse exp(-lv) + lv, lv, pU[0..E), (pU > 0)[0..E), pV[0..E), (pV > 0)[0..E) ]
 * mse = sum_j (denoised - x0)^2 / L of the sample ((B, L) fp32 each), w = (sigma^2 + sigma_data^2) / (sigma sigma_data)^2 the EDM weight,
 * lv = clamp(log_var, -10, 10) as hdmoe_edm_loss_fwd takes it (log_var (B) fp32; NULL: lv = 0), pU / pV the (B, E) fp32 gate
 * probabilities of the two routers.  A row with level < 0 or >= K contributes nothing and indexes nothing.
 * Two launches, no atomics, nothing zeroed: the caller zeroes acc between evaluations, outside any captured graph.  The first launch writes
 * one fp32 partial sum of squares per (sample, chunk of hdmoe_eval_chunk() = 4096 elements) into ws -- B * ceil(L / hdmoe_eval_chunk())
 * floats, caller-provided; the chunking does not depend on B -- the second is one workgroup that sums per level, in sample order, in
 * double.  The same inputs give the same bits, eager or replayed; a NaN reaches the sums of its own level only.
 * HDMOE_EINVAL: NULL acc / ws / denoised / x0 / sigma / level / pU / pV, B < 1 or > 4096, L < 1, E < 1 or > 8, K < 1 or > 64. */
int hdmoe_eval_chunk(void);
int hdmoe_eval_accumulate(double* acc, float* ws, const float* denoised, const float* x0, const float* sigma, const int* level,
                          const float* log_var, const float* pU, const float* pV, int B, long L, int E, int K, double sigma_data, HS stream);

/* ---- K6: norms  (model_internals.py:8-30; nn.GroupNorm / nn.LayerNorm in model_components.py) ------------ */
int hdmoe_pixelnorm_fwd(void* xn, void* h, const void* x, long rows, int C, int dtype, HS stream);               /* h = mp_silu(xn), optional */
int hdmoe_pixelnorm_bwd(void* dx, const void* dxn, const void* dh, const void* x, long rows, int C, float sx, int dtype, HS stream);   /* sx scales dxn */
int hdmoe_groupnorm_fwd(void* y, float* mean, float* rstd, const void* x, const float* gamma, const float* beta, int N,
                        long S, int C, int G, int act, float eps, int dtype, HS stream);                         /* act: 0 none, 1 relu, 2 mp_silu */
int hdmoe_groupnorm_bwd(void* dx, float* dgamma, float* dbeta, float* ws, const void* dy, const void* x,
                        const float* gamma, const float* beta, const float* mean, const float* rstd, int N, long S, int C,
                        int G, int act, int dtype, HS stream);                                                   /* ws: 2*N*G floats */
/* small batches: each sample's rows are split over `parts` (<= 64) workgroups.  fwd ws: 2*N*parts*G floats (partial mean / M2,
 * merged in a fixed order); bwd ws: 2*N*G floats that the CALLER ZEROES (row-range blocks add into them). */
int hdmoe_groupnorm_fwd_split(void* y, float* mean, float* rstd, float* ws, int parts, const void* x, const float* gamma,
                              const float* beta, int N, long S, int C, int G, int act, float eps, int dtype, HS stream);
int hdmoe_groupnorm_bwd_bcast(void* dx, float* dgamma, float* dbeta, float* ws, const float* g, float scale, const void* x,
                              const float* gamma, const float* beta, const float* mean, const float* rstd, int N, long S, int C, int G,
                              int act, int dtype, HS stream);   /* incoming gradient = g[n][c] * scale at every position (mean over S follows the norm) */
int hdmoe_groupnorm_bwd_split(void* dx, float* dgamma, float* dbeta, float* ws, int parts, const void* dy, const void* x,
                              const float* gamma, const float* beta, const float* mean, const float* rstd, int N, long S, int C,
                              int G, int act, int dtype, HS stream);
/* Router-trunk backward with bf16 gradient tensors (GroupNorm(1, C) + ReLU of Router.hard_route, reference models/model_components.py:100-112;
 * x = the conv output, fp32).  gn1t_bwd: dz bf16 [N][S][C] or (dz == null) g[n][c] * gscale at every position -> dx bf16; ws: 2 N floats;
 * dgamma / dbeta accumulate.  gn1t_act: out bf16 = relu(y * scale[n][c] + shift[n][c]) (scale == null: bf16(y)) -- the conv input as the bf16
 * weight-gradient program reads it. */
int hdmoe_gn1t_bwd(void* dx, float* dgamma, float* dbeta, float* ws, const void* dz, const float* g, float gscale, const float* x, const float* gamma,
                   const float* beta, const float* mean, const float* rstd, int N, long S, int C, HS stream);
int hdmoe_gn1t_act(void* out, const float* y, const float* scale, const float* shift, int N, long S, int C, HS stream);
/* The same backward in at most two launches per layer, with every sum in a fixed order that does not depend on the rest of the batch and no
 * float atomics.  gn1t_stats: from dz (bf16 [N][S][C]) the per-(sample, row range) sums into ws (gn1t_stats_floats floats).  gn1t_apply: dx (bf16)
 * from dz and ws, or (dz == null) from g[n][c] * gscale at every position and the forward's pcnt / qsum (hdmoe_gn1_finalize_relu_mean_pq);
 * in the same launch a = gn1t_act(xin, scale, shift) ([N][S][CI], bit-identical); dgamma / dbeta accumulate.  C, CI % 8 == 0, <= 2048. */
int hdmoe_gn1t_stats_floats(int N, long S, int C);
int hdmoe_gn1t_stats(float* ws, const void* dz, const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd, int N,
                     long S, int C, HS stream);
int hdmoe_gn1t_apply(void* dx, void* a, float* dgamma, float* dbeta, const float* ws, const void* dz, const float* g, float gscale, const float* pcnt,
                     const float* qsum, const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd, const float* xin,
                     const float* scale, const float* shift, int N, long S, int C, int CI, HS stream);
int hdmoe_layernorm_fwd(void* y, float* mean, float* rstd, const void* x, const float* gamma, const float* beta, long rows,
                        int C, float eps, int dtype, HS stream);
int hdmoe_layernorm_bwd(void* dx, float* dgamma, float* dbeta, const void* dy, const void* x, const float* gamma,
                        const float* mean, const float* rstd, long rows, int C, int dtype, HS stream);

/* ---- K5: attention core  (model_internals.py:374-404) --------------------------------------------------------
 * hdmoe_attn_bwd: delta [B][H][Sq] fp32 scratch; dbias [H][Sb][Sb] fp32 or null: its [:, :Sq, :Skv] corner accumulates (+=; the caller
 * zeroes a fresh buffer), the rest is not touched. */
int hdmoe_attn_fwd(void* out, float* lse, const void* q, const void* k, const void* v, const float* bias, int B, int Sq,
                   int Skv, int H, int D, int Sb, int dtype, HS stream);
int hdmoe_attn_bwd(void* dq, void* dk, void* dv, float* dbias, float* delta, const void* dout, const void* out,
                   const void* q, const void* k, const void* v, const float* lse, const float* bias, int B, int Sq,
                   int Skv, int H, int D, int Sb, int dtype, HS stream);

/* rel_pos_bias resize for S > S0 (model_internals.py:388-397: F.interpolate(..., mode='bicubic', align_corners=False)).
 * fwd: out [H][S][S] <- table [H][S0][S0];  bwd: dtable (caller zeroes) += transpose of the same linear map applied to dout. */
int hdmoe_bicubic_fwd(float* out, const float* table, int H, int S0, int S, HS stream);
int hdmoe_bicubic_bwd(float* dtable, const float* dout, int H, int S0, int S, HS stream);

/* ---- ViT expert BANK: ragged tokens (csrc/ragged.hip, csrc/attention.hip) ----------------------------------------
 * The reference evaluates its ViT experts one by one on the samples routed to each (model_config1.py:25-37,
 * model_components.py:435-706).  The bank keeps all routed rows in one padded tensor [R][Sp][C]: rows [seg[g], seg[g+1])
 * (device int32, from hdmoe_dispatch_plan) belong to expert g and hold lens[g] (host int array) real tokens followed by
 * zero padding.  srcs / dsts / gamma / ... are host arrays of per-expert device pointers. */
int hdmoe_rag_pack(void* dst, const void* const* srcs, const float* const* pos, const int* seg, const int* lens, int ngroups,
                   int R, int Sp, int C, int dtype, HS stream);
int hdmoe_rag_pack_bwd(void* const* dsrcs, float* const* dpos, const void* ddst, const int* seg, const int* lens, int ngroups,
                       int R, int Sp, int C, int dtype, HS stream);
int hdmoe_rag_unpack(void* const* dsts, const void* src, const int* seg, const int* lens, int ngroups, int R, int Sp, int C,
                     int dtype, HS stream);
int hdmoe_rag_unpack_bwd(void* dsrc, const void* const* ddsts, const int* seg, const int* lens, int ngroups, int R, int Sp,
                         int C, int dtype, HS stream);
/* own-row forms: expert g's compact tensor is written (pack_bwd, unpack) / read (unpack_bwd) in its rows [seg[g], seg[g+1]) only */
int hdmoe_rag_pack_bwd_own(void* const* dsrcs, float* const* dpos, const void* ddst, const int* seg, const int* lens, int ngroups,
                           int R, int Sp, int C, int dtype, HS stream);
int hdmoe_rag_unpack_own(void* const* dsts, const void* src, const int* seg, const int* lens, int ngroups, int R, int Sp, int C,
                         int dtype, HS stream);
int hdmoe_rag_unpack_bwd_own(void* dsrc, const void* const* ddsts, const int* seg, const int* lens, int ngroups, int R, int Sp,
                             int C, int dtype, HS stream);
/* rows of y [R][row_bytes] that lie in no expert's window := 0, the others stay untouched (the shared output of row-windowed passes) */
int hdmoe_rag_zero_unowned(void* y, const int* seg, int ngroups, int R, long row_bytes, HS stream);
int hdmoe_rag_select(void* y, const void* const* outs, const int* seg, int ngroups, int R, long row_bytes, HS stream);
int hdmoe_rag_select_bwd(void* const* douts, const void* dy, const int* seg, int ngroups, int R, long row_bytes, HS stream);
/* nn.GroupNorm(G, C) over each row's real tokens (+ act: 0 none, 1 relu, 2 mp_silu); mean / rstd [R][G] */
int hdmoe_gn_rag_fwd(void* y, float* mean, float* rstd, const void* x, const float* const* gamma, const float* const* beta,
                     const int* seg, const int* lens, int ngroups, int R, int Sp, int C, int G, int act, float eps, int dtype,
                     HS stream);
int hdmoe_gn_rag_bwd(void* dx, float* const* dgamma, float* const* dbeta, const void* dy, const void* x,
                     const float* const* gamma, const float* const* beta, const float* mean, const float* rstd, const int* seg,
                     const int* lens, int ngroups, int R, int Sp, int C, int G, int act, int dtype, HS stream);
/* nn.LayerNorm(C) per token with the row's expert's affine; mean / rstd [R * Sp] */
int hdmoe_ln_rag_fwd(void* y, float* mean, float* rstd, const void* x, const float* const* gamma, const float* const* beta,
                     const int* seg, int ngroups, int R, int Sp, int C, float eps, int dtype, HS stream);
int hdmoe_ln_rag_bwd(void* dx, float* const* dgamma, float* const* dbeta, const void* dy, const void* x,
                     const float* const* gamma, const float* mean, const float* rstd, const int* seg, int ngroups, int R, int Sp,
                     int C, int dtype, HS stream);
/* self-attention over each row's real tokens with the expert's rel_pos_bias table bias[g] [H][sb[g]][sb[g]]
 * (model_internals.py:374-404); lse / delta [R][H][Sp]; dbias[g] accumulate (+=), or dbias == NULL */
int hdmoe_attn_rag_fwd(void* out, float* lse, const void* q, const void* k, const void* v, const float* const* bias,
                       const int* seg, const int* lens, const int* sb, int ngroups, int R, int Sp, int H, int D, int dtype,
                       HS stream);
int hdmoe_attn_rag_bwd(void* dq, void* dk, void* dv, float* const* dbias, float* delta, const void* dout, const void* out,
                       const void* q, const void* k, const void* v, const float* lse, const float* const* bias, const int* seg,
                       const int* lens, const int* sb, int ngroups, int R, int Sp, int H, int D, int dtype, HS stream);
/* longest row (largest lens[g]) the two above accept at head dim D: backward == 0 hdmoe_attn_rag_fwd, else hdmoe_attn_rag_bwd, which
 * keeps more of a head in LDS and so takes shorter rows; 0: no kernel for this D.  Launches nothing. */
int hdmoe_attn_rag_max_len(int D, int backward);

/* ---- many small linear layers over ONE input in one launch (csrc/mlinear.hip): Unet_block.emb_layer of every block
 * (model_components.py:232-236) and MP_Attention.q_time / k_time / v_time of every ViT block (model_internals.py:360-372).
 * w[l] = prepared fp32 weight image of layer l, [ngroups][O[l]][Ipad]; lens = host array O[0..L); y / dy: host arrays of L device
 * pointers to [R][O[l]] fp32; G: host array of L * 8 device pointers to the [O[l]][I] fp32 gradient slabs (NULL = skip), += */
int hdmoe_mlinear_fwd(float* const* y, const float* x, const float* const* w, const int* seg, const int* lens, int L, int R, int I,
                      int Ipad, int ngroups, float c, HS stream);
int hdmoe_mlinear_dgrad(float* dx, const float* const* dy, const float* const* w, const int* seg, const int* lens, int L, int R,
                        int I, int Ipad, int ngroups, HS stream);
int hdmoe_mlinear_wgrad(float* const* G, const float* const* dy, const float* x, const int* seg, const int* lens, int L, int R, int I,
                        int ngroups, HS stream);

/* ---- K1/K2: router head + dispatch  (model_components.py:155-168, model_config1.py:11-39) ---------------------- */
int hdmoe_router_head_fwd(float* sparse, float* probs, float* xout, int* idx, const float* logits, const float* noise,
                          const float* mask, long B, int E, int k, HS stream);
int hdmoe_router_head_bwd(float* dlogits, const float* dsparse, const float* dprobs, const float* dxout,
                          const float* sparse, const float* probs, const int* idx, const float* mask, long B, int E, int k,
                          HS stream);
int hdmoe_dispatch_plan(int* perm, int* row_expert, float* row_w, int* inv, int* seg, const float* sparse, int B, int E,
                        int kcap, HS stream);
/* The head with a per-expert selection bias (auxiliary-loss-free load balancing): the top-k runs over xout[e] + sel_bias[e] (ties to the
 * lowest index, masked entries stay -inf); probs, xout and the k gate weights -- the softmax of the raw xout over the selected experts,
 * stabilised by their maximum -- do not see the bias, and the backward is hdmoe_router_head_bwd from the saved idx and sparse.  With a
 * zero bias every output is bit-identical to hdmoe_router_head_fwd.  load / target (E each; both or neither) are ACCUMULATED: load[e] += 1
 * per row that selected e among the experts its mask allows (a row with fewer allowed experts than k fills up with masked ones at weight 0:
 * not counted), target[e] += round(2^20 min(k, a_b) / a_b) per row b whose mask allows e, a_b = that row's allowed experts (E without a
 * mask; rows with a_b = 0 add nothing).  Integers: the sums do not depend on the order of the atomics. */
int hdmoe_router_head_bias_fwd(float* sparse, float* probs, float* xout, int* idx, const float* logits, const float* noise,
                               const float* mask, const float* sel_bias, long long* load, long long* target, long B, int E, int k,
                               HS stream);
/* One launch behind the optimizer step.  ok NULL or *ok != 0: bias[e] += rate * sign(target[e] - 2^20 load[e]) (compared in integers, a tie
 * gives 0), then the mean over e is subtracted, then the result is clamped to [-bias_max, bias_max]; *ok == 0 leaves bias bit for bit.
 * Always: last_load / last_target = the accumulators, then the accumulators are cleared. */
int hdmoe_balance_bias_update(float* bias, long long* load, long long* target, long long* last_load, long long* last_target,
                              const int* ok, float rate, float bias_max, int E, HS stream);
/* counts[e] += seg[e+1] - seg[e] as float: rows routed to expert e since the last optimizer step (read by hdmoe_mt_adamw's `use` flags;
 * cleared by the caller behind the update) */
int hdmoe_seg_counts(float* counts, const int* seg, int E, HS stream);
/* counts[e] += rows of `sparse` (B, E) with a weight > 0 in column e: the same bookkeeping on the path that evaluates every expert on
 * the whole batch (no dispatch plan); reference models/model_config1.py:26-29. */
int hdmoe_route_counts(float* counts, const float* sparse, int B, int E, HS stream);
int hdmoe_gather_rows(void* dst, const void* src, const int* perm, long R, long L, int dtype, HS stream);
/* dst[r] = src[perm[r] % Bsrc] (zeros where perm[r] < 0): gather for a plan built over stacked copies of Bsrc source rows -- the
 * guided evaluation's 2B-row plan over B-row stem features / time embeddings, which are stored once */
int hdmoe_gather_rows_paired(void* dst, const void* src, const int* perm, long R, long L, int Bsrc, int dtype, HS stream);
int hdmoe_combine_rows_fwd(void* out, const void* ys, const int* inv, const float* row_w, long B, int kcap, long L,
                           int dtype, HS stream);
int hdmoe_combine_rows_bwd(void* dys, float* dsparse, const void* dout, const void* ys, const int* perm,
                           const int* row_expert, const float* row_w, long R, int E, long L, int dtype, HS stream);
/* 16-byte forms (csrc/relayout.hip): one workgroup per (row, chunk), row decoded and inv / perm / row_w read once per workgroup.  out and
 * dys are bit-identical to the scalar forms; dsparse sums its per-chunk dot product in another tree.  Return 1 and launch nothing
 * when L is not a multiple of 8 (bf16) / 4 (fp32) or a pointer is not 16-byte aligned: the caller then runs the scalar form. */
int hdmoe_combine_rows_fwd_vec(void* out, const void* ys, const int* inv, const float* row_w, long B, int kcap, long L,
                               int dtype, HS stream);
int hdmoe_combine_rows_bwd_vec(void* dys, float* dsparse, const void* dout, const void* ys, const int* perm,
                               const int* row_expert, const float* row_w, long R, int E, long L, int dtype, HS stream);

/* ---- N2 (next to the path): EDM_LOSS fused  (Utils/utils.py:127-172) ---------------------------------------------- */
/* out[5] = loss, denoising, balance, z_loss, pure_loss; aux: 2E+3 floats kept for the backward; sse: B floats scratch */
int hdmoe_edm_loss_fwd(float* out, float* aux, float* sse, const float* denoised, const float* target, const float* log_var,
                       const float* pU, const float* pV, const float* rU, const float* rV, int B, long L, int E, float unet_bal,
                       float vit_bal, float z_bal, HS stream);
int hdmoe_edm_loss_bwd(float* dD, float* dlv, float* dpU, float* dpV, float* drU, float* drV, const float* gin, const float* aux,
                       const float* sse, const float* denoised, const float* target, const float* log_var, const float* rU,
                       const float* rV, int B, long L, int E, float unet_bal, float vit_bal, float z_bal, HS stream);

/* ---- the 33-channel first conv of Unet_expert (torch.cat([x, ones]), reference models/model_components.py:416) on the conv6 / wgrad6
 * kernels (csrc/ones6.hip): the ones channel becomes a per-expert border-aware bias map, its weight gradient a sum of dy over pixel
 * rectangles.  wf [g][tap][O][Ipad] / wd [g][tap][C + 1][Opad]: the weight images of the (C + 1)-channel layer; gbias, S: fp32
 * workspaces [ngroups][H][W][O]; G33: weight-gradient slabs [tap][O][C + 1] (+=); G32: zeroed workspace slabs [tap][O][C]; ws: as
 * hdmoe_conv_wgrad6.  Both return 1 without launching anything outside the domain (bf16, conv6 shapes, k in {3, 5} for the backward). */
int hdmoe_conv6_ones_fwd(const void* x, const void* wf, void* y, float* gbias, float alpha, const int* seg, int ngroups, long wstride,
                         int N, int H, int W, int C, int O, int Ipad, const int* kh, int dtype, HS stream);
int hdmoe_conv6_ones_bwd(const void* x, const void* dy, const void* wd, void* dx, float* const* G33, float* S, float* const* G32, const int* seg,
                         int ngroups, long wdstride, int N, int H, int W, int C, int O, int Opad, const int* kh, float alpha, void* ws, long ws_bytes,
                         int dtype, HS stream);

/* ---- K3+K4 fused: Unet_block main branch as one persistent launch (csrc/blk6.hip; reference models/model_components.py:240-253) ----
 * u = conv(x, w1); h = dropout_p(mp_silu(u * e[n][c])); y = alpha * conv(h, w2) + beta * res   (u, h, y written; the activation tile
 * stays in LDS between the two convs).  x [N][H][W][Cin], u / h / y / res [N][H][W][C] bf16, e fp32 [N][C]; w1 [g][tap][C][Cin],
 * w2 [g][tap][C][C] forward weight images; kh: per-expert square kernel size, "same" padding.  Returns 1 without launching outside
 * the kernel's domain (bf16, W in {16, 32}, H % (256 / W) == 0, k in {3, 5, 7}, Cin % 32 == 0, C in {32, 64}). */
int hdmoe_unet_block_fwd(const void* x, const void* w1, const void* w2, void* u, void* h, void* y, const void* res, const float* e,
                         unsigned long long seed, const unsigned long long* seed_dev, float p, float alpha, float beta, const int* seg,
                         int ngroups, long w1stride, long w2stride, int N, int H, int W, int Cin, int C, const int* kh, int dtype,
                         HS stream);
int hdmoe_blk6_debug_stamps(void* buf);   /* development: 8 x 64 u64 device buffer for workgroup 0's in-kernel time stamps, or NULL */

/* ---- N3: fused multi-tensor clip_grad_norm_ + AdamW  (Utils/training.py:55-65,195-197) ----------------------------------- */
/* descs: device array of {p, g, m, v, step, use addresses, numel, group} (hdmoe_opt_desc_bytes() bytes each); chunks: device int32 pairs
 * (descriptor index, 4096-element chunk index).  The clip coefficient min(1, max_norm/(sqrt(sumsq)+1e-6)) is read on the device.
 * step: the tensor's own AdamW step count (device float, advanced by hdmoe_mt_adamw); use: device float, > 0 when the tensor received a
 * gradient this step, or 0 = always -- a tensor of an expert that got no sample is skipped like a grad-None tensor in torch.optim.AdamW
 * (reference models/model_config1.py:26-29 leaves such an expert out of the graph; Utils/training.py:195-197). */
int hdmoe_opt_desc_bytes(void);
int hdmoe_mt_sumsq(float* sumsq, const void* descs, const int* chunks, int nchunks, float* ws, HS stream);   /* ws: nchunks floats; deterministic */
int hdmoe_mt_clip_scale(const void* descs, const int* chunks, int nchunks, const float* sumsq, float max_norm, HS stream);
int hdmoe_mt_adamw(const void* descs, const int* chunks, int nchunks, int ntensors, const float* sumsq, float max_norm, const float* group_lr,
                   const float* group_wd, int ngroups, float beta1, float beta2, float eps, HS stream);
/* hdmoe_mt_adamw behind a device verdict: *ok != 0 is hdmoe_mt_adamw bit for bit, *ok == 0 writes nothing (no weight decay, no moment
 * decay, no per-tensor step increment).  ok == NULL is hdmoe_mt_adamw. */
int hdmoe_mt_adamw_ok(const void* descs, const int* chunks, int nchunks, int ntensors, const float* sumsq, float max_norm, const float* group_lr,
                      const float* group_wd, int ngroups, float beta1, float beta2, float eps, const int* ok, HS stream);
/* One statistics pass over the same table: the descriptor's `group` is a statistics group 0..ngroups-1 (1 <= ngroups <= 64; a chunk whose
 * group lies outside counts towards the total only), `which` picks the array (d.g or d.p).
 *   stats  (ngroups + 1, 4) fp32: {sum, sum of squares, min, max} over the FINITE elements of the group; a non-finite element adds 0
 *   counts (ngroups + 1, 2) int64: {non-finite elements, elements}
 * The last row of both is the total over every chunk.  A group without elements: {0, 0, +inf, -inf}, {0, 0}.
 *   ok       (int32, may be NULL): 1 when the total non-finite count is 0 and the total sum of squares is finite (finite elements can
 *            still overflow the sum), else 0
 *   counters (int64 [4], may be NULL): {passes measured, passes with ok == 0, such passes in a row, step of the last such pass (-1 until
 *            there is one; the launch scalar `step`)}; an ok pass sets the in-a-row count to 0.  The caller initialises them once.
 *   ws       HDMOE_STATS_WS_PER_CHUNK * nchunks floats of scratch
 * Two launches, no atomics, fixed summation order: a chunk's partial takes thread t's elements t, t + 256, ... in order and then the block
 * tree of hdmoe_mt_sumsq; a row sums thread t's chunk partials t, t + 1024, ... in order and then the same block tree (1024 threads).  The
 * total sum of squares of a table without a non-finite element is therefore bit-identical to hdmoe_mt_sumsq's, and stats + 4 * ngroups + 1
 * can stand in for it as hdmoe_mt_adamw's `sumsq`.  HDMOE_EINVAL before anything is written: stats or counts NULL, ngroups outside 1..64,
 * which outside {0, 1}, nchunks < 0, or nchunks > 0 with descs, chunks or ws NULL.  nchunks == 0 writes the empty-group rows and ok = 1. */
#define HDMOE_STATS_GRAD 0
#define HDMOE_STATS_PARAM 1
#define HDMOE_STATS_WS_PER_CHUNK 6
int hdmoe_mt_stats(float* stats, long long* counts, int* ok, long long* counters, const void* descs, const int* chunks, int nchunks,
                   int ngroups, int which, long long step, float* ws, HS stream);

/* ---- N4: exponential moving average of the weights (EDM2 power-function profiles; no counterpart in the reference) ---------------- */
/* descs: device array of {p, e[4] addresses, numel} (hdmoe_ema_desc_bytes() bytes each), all fp32; chunks: device int32 pairs
 * (descriptor index, 4096-element chunk index), as for N3.  hdmoe_mt_ema advances *step_counter (device int64) to t and then writes, for
 * every element and every profile k < nprofiles (1..4), e_k += a_k * (p - e_k) with one fma.  HDMOE_EMA_POWER: gammas_or_betas = gamma_k
 * (device doubles), a_k = 1 - (1 - 1/t)^(gamma_k + 1) evaluated in fp64 on the device, a_k = 1 at t = 1 (e_k = p bit for bit).
 * HDMOE_EMA_CONSTANT: gammas_or_betas = beta_k, a_k = 1 - beta_k for every t.  No host value changes between steps, so one captured
 * launch serves every step; no atomics, bit-identical from run to run.  hdmoe_mt_swap exchanges p <-> e_profile in place (twice = identity).
 * nchunks == 0: nothing is launched, the counter stays. */
#define HDMOE_EMA_POWER 0
#define HDMOE_EMA_CONSTANT 1
int hdmoe_ema_desc_bytes(void);
int hdmoe_mt_ema(const void* descs, const int* chunks, int nchunks, int nprofiles, long long* step_counter, const double* gammas_or_betas,
                 int mode, HS stream);
/* hdmoe_mt_ema behind a device verdict (hdmoe_mt_stats' ok): *ok != 0 is hdmoe_mt_ema bit for bit, *ok == 0 writes nothing (no step
 * increment, no profile write).  ok == NULL is hdmoe_mt_ema. */
int hdmoe_mt_ema_ok(const void* descs, const int* chunks, int nchunks, int nprofiles, long long* step_counter, const double* gammas_or_betas,
                    int mode, const int* ok, HS stream);
int hdmoe_mt_swap(const void* descs, const int* chunks, int nchunks, int profile, HS stream);
/* Post-hoc reconstruction (EDM2 section 3.2): nsrc saved averages -> ndst new ones in one pass.  src_table / dst_table: device arrays of
 * nsrc (1..4096) / ndst (1..8) 64-bit device addresses of flat fp32 buffers of numel elements each; weights: device doubles [nsrc][ndst],
 * source-major.  dst_t[i] = (float) sum_s weights[s][t] * (double) src_s[i]: one fp64 fma chain per element and target in source order
 * 0..nsrc-1, rounded to fp32 once at the store.  No atomics and no reduction across threads: bit-identical from run to run, and a target's
 * result does not depend on which other targets share its launch.  Every source is read once for all targets and every target is
 * written once, (nsrc + ndst) * 4 * numel bytes.  16-byte accesses when every table entry is 16-byte aligned, 4-byte ones otherwise.
 * numel == 0: nothing is launched. */
int hdmoe_mt_combine(const void* src_table, const void* dst_table, int nsrc, int ndst, long numel, const double* weights, HS stream);

#undef HS
#ifdef __cplusplus
}
#endif
#endif /* HDMOE_H */
