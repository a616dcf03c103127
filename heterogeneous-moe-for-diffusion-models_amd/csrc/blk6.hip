// K3 + K4 fused: the main branch of a Unet_block as ONE persistent launch for all experts of a layer (reference
// models/model_components.py:240-253):
//     conv_res1 (k x k) -> * (1 + emb_layer(e) * gain) -> mp_silu -> F.dropout -> conv_res2 (k x k) -> mp_sum with the residual.
//
// Why: at this model's widths (32 / 64 channels on 32x32 / 16x16 latents) a k x k layer is 10-20 GFLOP and 67 MB -- below the bf16 ridge and
// a handful of work units per CU, so the three launches of a block (conv6, film_silu, conv6) are dominated by their fixed costs and by the
// HBM round trips of the intermediate tensor: written by the first conv, read and re-written by the FiLM pass, read by the second conv.
// Here a work unit is one 256-pixel output tile (8 x 32 or 16 x 16) of one routed row: the workgroup computes the first conv on the tile
// grown by (k - 1) / 2 rows on either side (halo recompute, columns are whole image rows), applies the middle op to the accumulators,
// leaves the activation in LDS as the second conv's input image and runs the second conv from there.  Per block and pixel the forward then
// moves x once in and u (the pre-activation, for the backward), h (the activation, for conv_res2's weight gradient) and y once out -- the
// three intermediate READS and one launch boundary per conv disappear, and a unit carries 2.25-2.5x the MFMA work of a conv6 unit behind
// one pipeline prologue.  LDS per workgroup (160 KB): two x-chunk buffers, the intermediate image (1-2 planes of 32 channels), two weight
// stages; the DMA pieces, swizzle and tap loop are conv6's (conv6_body.h).
//
// Domain: bf16, W in {16, 32}, H a multiple of 256 / W, square odd k in {3, 5, 7} with "same" padding, Ca % 32 == 0, Cm in {32, 64},
// Cb % 32 == 0.  Everything else returns 1 (the caller runs the layers one by one).
#include <type_traits>
#include "common.h"
#include "conv_args.h"
#include "conv6_common.h"
#include "hdmoe.h"
#include "blk6_body.h"

namespace {

template <int NW, int NTM, int NTB>
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void blk6_kernel(B6Args a) {
  blk6_body<NW, NTM, NTB>(a, blockIdx.x, gridDim.x);
}

struct B6Plan { B6Args a; int NW, NTM, NTB; unsigned G; size_t lds; };
void* g_b6_stamps = nullptr;
constexpr int B6_EB = 256;                    // bytes of LDS behind the weight buffers: the unit's FiLM vector (<= 64 floats)

int blk6_plan(const void* x, const void* wa, const void* wb, void* y, const void* res, const int* seg, int ngroups, long wa_stride,
              long wb_stride, int N, int H, int W, int Ca, int Cm, int Cb, const int* ks, B6Plan& plan) {
  if (!(W == 16 || W == 32) || Ca % 32 || Cb % 32 || !(Cm == 32 || Cm == 64) || ngroups < 1 || ngroups > HDMOE_MAX_GROUPS) return 1;
  int maxk = 0;
  for (int g = 0; g < ngroups; ++g) {
    if (ks[g] != 3 && ks[g] != 5 && ks[g] != 7) return 1;
    if (ks[g] > maxk) maxk = ks[g];
  }
  const long taps = (long)maxk * maxk;
  const long xbytes = (long)N * H * W * Ca * 2;
  const long wabytes = ((long)(ngroups - 1) * wa_stride + taps * Cm * Ca) * 2, wbbytes = ((long)(ngroups - 1) * wb_stride + taps * Cb * Cm) * 2;
  if (!conv_align_extent_ok({x, wa, wb, y, res}, {xbytes, wabytes, wbbytes, (long)N * H * W * (Cb > Cm ? Cb : Cm)})) return 1;
  B6Args& a = plan.a;
  a.x = x; a.wa = wa; a.wb = wb; a.y = y; a.res = res; a.seg = seg; a.wa_stride = wa_stride; a.wb_stride = wb_stride;
  a.N = N; a.H = H; a.W = W; a.Ca = Ca; a.Cm = Cm; a.Cb = Cb; a.ngroups = ngroups;
  a.xbytes = (int)xbytes; a.wabytes = (int)wabytes; a.wbbytes = (int)wbbytes;
  for (int g = 0; g < HDMOE_MAX_GROUPS; ++g) { a.ks[g] = g < ngroups ? ks[g] : ks[0]; }
  conv_sort_groups_desc(a.ks, a.order, ngroups);
  const int NTM = Cm / 32, NTB = Cb % 64 == 0 ? 2 : 1;
  const int nbmax = 32 * (NTM > NTB ? NTM : NTB);
  // Geometry candidates, best first: 4-wave workgroups, two per CU (<= 80 KB of LDS each, one x buffer, conv A over <= 12 blocks), on
  // the 256-pixel tile or -- 64-channel layers, whose intermediate image is twice as large -- on a 128-pixel tile; else one 8-wave
  // workgroup per CU with two x buffers.
  struct Cand { int nw, th; };
  const Cand cands[3] = {{4, 256 / W}, {8, 256 / W}, {4, 128 / W}};     // (128-pixel tiles measured slower than the 8-wave form: last resort)
  bool found = false;
  for (const Cand& cd : cands) {
    const int th = cd.th;
    if (th < 4 || H % th || (th * W) % 32) continue;
    if (cd.nw == 4 && (th * W == 128) && NTM != 2) continue;
    const int ppt = ((th + 2 * (maxk - 1)) * (W + maxk - 1) + 15) / 16;
    const int nblkA = (th + maxk - 1) * W / 32;
    if (ppt > 48 || ((th + maxk - 1) * W) % 32) continue;
    if (cd.nw == 4 && (nblkA > (NTM == 2 ? 8 : 12) || ppt > 36)) continue;
    const int xb = cd.nw * ((ppt + cd.nw - 1) / cd.nw) * 1024;
    const int hbp = (((th + maxk - 1) * (W + maxk - 1) * 64) + 1023) / 1024 * 1024;
    const int cap = cd.nw == 4 ? 80 * 1024 : 160 * 1024;
    const int fixed = (cd.nw == 4 ? 1 : 2) * xb + NTM * hbp + B6_EB;
    const int best = conv_pick_stage_T(ngroups, ks, nbmax / 16, fixed, nbmax * 64, cap);
    if (!best) continue;
    a.TH = th; a.tpi = H / th; a.xb_bytes = xb; a.hb_plane = hbp; a.T = best; a.wb_bytes = best * nbmax * 64; a.nxp = xb / 1024 / cd.nw;
    plan.NW = cd.nw;
    plan.lds = (size_t)fixed + 2 * (size_t)a.wb_bytes;
    found = true;
    break;
  }
  if (!found) return 1;
  a.m_tpi = conv_recip(a.tpi); a.m_T = conv_recip(a.T);
  const long units = (long)N * a.tpi;
  const long gcap = plan.NW == 4 ? 512 : 256;
  plan.G = (unsigned)(units < gcap ? units : gcap);
  plan.NTM = NTM; plan.NTB = NTB;
  a.stamps = (unsigned long long*)g_b6_stamps;
  a.dbg = 0;
  return 0;
}

int blk6_launch(const B6Plan& plan, hipStream_t stream) {
  static unsigned long long attr_set = 0;
  if (hdmoe_first_on_device(attr_set)) {
#define B6_ATTR(W, M, B, L) (void)hipFuncSetAttribute((const void*)blk6_kernel<W, M, B>, hipFuncAttributeMaxDynamicSharedMemorySize, L * 1024)
    B6_ATTR(8, 1, 1, 160); B6_ATTR(8, 1, 2, 160); B6_ATTR(8, 2, 1, 160); B6_ATTR(8, 2, 2, 160);
    B6_ATTR(4, 1, 1, 80); B6_ATTR(4, 1, 2, 80); B6_ATTR(4, 2, 1, 80); B6_ATTR(4, 2, 2, 80);
  }
  hdmoe_count_selection(HDMOE_SEL_BLK6);
  conv_pick<4, 8>(plan.NW, [&](auto Nw) { conv_pick<2, 1>(plan.NTM, [&](auto Ntm) { conv_pick<2, 1>(plan.NTB, [&](auto Ntb) {
    constexpr int NW = decltype(Nw)::value;
    hipLaunchKernelGGL((blk6_kernel<NW, decltype(Ntm)::value, decltype(Ntb)::value>), dim3(plan.G), dim3(64 * NW), plan.lds, stream, plan.a);
  }); }); });
  return hdmoe_launch_status();
}

}  // namespace

extern "C" {

// development hook (tools/blk6_bench.py --stamps): 8 x 64 u64 device buffer receiving workgroup 0's in-kernel time stamps
int hdmoe_blk6_debug_stamps(void* buf) { g_b6_stamps = buf; return HDMOE_OK; }

/* Forward of Unet_block's main branch for all experts of a layer (reference models/model_components.py:240-253):
 *   u = conv(x, w1)                         [N][H][W][C]   (written: the backward needs the pre-activation; NULL: not stored)
 *   h = dropout_p(mp_silu(u * e[n][c]))     [N][H][W][C]   (written: conv_res2's weight gradient reads it; NULL: not stored)
 *   y = alpha * conv(h, w2) + beta * res    [N][H][W][C]
 * x [N][H][W][Cin] bf16 is the block's (already mp_silu'd) input; w1 [g][tap][C][Cin], w2 [g][tap][C][C]: forward weight images of
 * hdmoe_wbank_prep / hdmoe_wprep_fwd (w?stride elements per expert); kh: per-expert square kernel size ("same" padding); e fp32 [N][C];
 * seed / seed_dev / p: the dropout of hdmoe_film_silu_drop_fwd (same Philox stream: bit-identical to the three separate launches).
 * Returns 1 without launching when the layer is outside the kernel's domain. */
int hdmoe_unet_block_fwd(const void* x, const void* w1, const void* w2, void* u, void* h, void* y, const void* res, const float* e,
                         unsigned long long seed, const unsigned long long* seed_dev, float p, float alpha, float beta, const int* seg,
                         int ngroups, long w1stride, long w2stride, int N, int H, int W, int Cin, int C, const int* kh, int dtype,
                         hipStream_t stream) {
  if (!x || !w1 || !w2 || !y || !e || N < 0 || p < 0.f || p >= 1.f) return HDMOE_EINVAL;       // (u, h may be NULL: inference, nothing saved for a backward)
  if (dtype != HDMOE_BF16) return 1;
  if (((uintptr_t)u | (uintptr_t)h) & 15) return 1;
  if (N == 0) return HDMOE_OK;
  B6Plan plan;
  if (blk6_plan(x, w1, w2, y, res, seg, ngroups, w1stride, w2stride, N, H, W, Cin, C, C, kh, plan)) return 1;
  B6Args& a = plan.a;
  a.alpha = alpha; a.beta = beta; a.alpha_mid = 1.f; a.mode = 0; a.e = e; a.u = u; a.hmid = h; a.de = nullptr;
  a.seed_dev = seed_dev; a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32); a.p = p;
  return blk6_launch(plan, stream);
}

}  // extern "C"
