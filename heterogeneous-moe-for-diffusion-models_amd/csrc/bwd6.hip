// Input gradient AND weight gradient of a k x k bf16 expert layer in ONE launch ("horizontal" fusion): the first G6 workgroups run the
// conv6 program on dy with the flipped weights (dgrad), the others the wgrad6 programs (3x3 class, then 5x5 class) on (x, dy).
// The two are independent, both read dy, and on this model's layer sizes each alone is dominated by its fixed costs (launch, pipeline
// prologue, tail of a persistent grid): back to back they cost ~30 + ~40 us per layer on the backward chain of the U-Net branch,
// side by side in one grid about the longer of the two.  A fork onto a second stream inside the graph would also overlap them, but a
// hipGraph with internal branches no longer runs concurrently with the other branch's graph (measured: the ViT backward graph then
// waits for the whole U-Net backward graph).
#include "common.h"
#include "conv_args.h"
#include "conv6_common.h"
#include "hdmoe.h"
#include "conv6_body.h"
#include "conv7_body.h"
#include "wgrad6_body.h"
#include "wgrad7_body.h"
#include "wgrad8_body.h"
#include "conv6s_body.h"

namespace {

template <int MT, int NT, int TWS, int OT>
__global__ __launch_bounds__(512) void bwd6_kernel(C6Args c, W6Args a3, W6Args a5, int G6, int ibs, int obs) {
  const int b = blockIdx.x;
  if (b < G6) { conv6_body<MT, NT>(c, b, G6); return; }
  int r = b - G6;
  const int bx = r % ibs; r /= ibs;
  const int by = r % obs;
  const int z = r / obs;
  if (z < a3.chunks) wgrad6_body<3, TWS, OT, false>(a3, bx, by, z);
  else wgrad6_body<5, TWS, OT, false>(a5, bx, by, z - a3.chunks);
}

template <int MT, int NT, int TWS, int OT>
void launch_bwd6(const C6Plan& cp, const W6DualPlan& wp, hipStream_t stream) {
  static unsigned long long attr = 0;
  if (hdmoe_first_on_device(attr)) { (void)hipFuncSetAttribute((const void*)bwd6_kernel<MT, NT, TWS, OT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
  const size_t lds = cp.lds > wp.lds ? cp.lds : wp.lds;
  const unsigned grid = cp.G + (unsigned)(wp.ibs * wp.obs * (wp.c[0].chunks + wp.c[1].chunks));
  hipLaunchKernelGGL((bwd6_kernel<MT, NT, TWS, OT>), dim3(grid), dim3(512), lds, stream, cp.a, wp.c[0], wp.c[1], (int)cp.G, wp.ibs, wp.obs);
}

// The same with the whole-image streaming kernel (conv7_body.h) as the dgrad program: 32 x 32 maps, enough images to fill the chip.
// EPI = 1: the dgrad program ends in the FiLM-backward epilogue (conv7_body.h) -- the layer's input is h = dropout(mp_silu(u * e)).
// DBG: the dgrad program is conv7_body's development instantiation (stamps, ablations).
template <int CO, int KMASK, int TWS, int OT, int EPI = 0, bool DBG = false>
__global__ __launch_bounds__(512) void bwd7_kernel(C7Args c, W6Args a3, W6Args a5, int G7, int ibs, int obs) {
  const int b = blockIdx.x;
  if (b < G7) { conv7_body<CO, KMASK, TWS == 4, EPI, DBG>(c, b, G7); return; }
  int r = b - G7;
  if (TWS == 5 && OT == 0) {                                 // 32 x 32 maps: the streaming weight-gradient programs (output chunks of 32)
    const int nbx3 = a3.Cin / (32 * a3.icw), nby3 = a3.Cout / (32 * a3.ocw), n3 = nbx3 * nby3 * a3.chunks;
    if (r < n3) {                                            // 3x3 class: wgrad8, icw x ocw channel chunks per workgroup
      const int bx = r % nbx3; r /= nbx3;
      const int by = r % nby3, z = r / nby3, pairs = a3.icw * a3.ocw;
      if (pairs == 0) wgrad7_body<3>(a3, bx, by, z);         // (never taken: icw >= 1; kept because removing it changes the kernel's register allocation)
      else if (pairs == 4) wgrad8_body3<4, 8>(a3, bx, by, z);
      else if (pairs == 2) wgrad8_body3<2, 8>(a3, bx, by, z);
      else wgrad8_body3<2, 16>(a3, bx, by, z);
      return;
    }
    r -= n3;
    const int bx = r % ibs; r /= ibs;
    wgrad7_body<5>(a5, bx, r % obs, r / obs);
  } else if (OT > 0) {                                       // 16 x 16 maps: the wgrad6 programs
    const int bx = r % ibs; r /= ibs;
    const int by = r % obs;
    const int z = r / obs;
    if (z < a3.chunks) wgrad6_body<3, TWS, OT == 0 ? 1 : OT, false>(a3, bx, by, z);
    else wgrad6_body<5, TWS, OT == 0 ? 1 : OT, false>(a5, bx, by, z - a3.chunks);
  }
}

template <int CO, int KMASK, int TWS, int OT, int EPI = 0, bool DBG = false>
void launch_bwd7(const C7Plan& cp, const W6DualPlan& wp, hipStream_t stream) {
  // a registered stamp buffer (development) takes the DBG kernel where one is instantiated: the shapes tools/conv7_check.py --stamps-bwd runs
  if constexpr (!DBG && EPI == 0 && (TWS == 5 || OT == 2)) {
    if (cp.a.stamps || cp.a.dbg) { launch_bwd7<CO, KMASK, TWS, OT, 0, true>(cp, wp, stream); return; }
  }
  static unsigned long long attr = 0;
  if (hdmoe_first_on_device(attr)) { (void)hipFuncSetAttribute((const void*)bwd7_kernel<CO, KMASK, TWS, OT, EPI, DBG>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
  const size_t clds = cp.lds + (EPI ? C7Lds<TWS == 4>::film_extra(CO) : 0);
  const size_t lds = clds > wp.lds ? clds : wp.lds;
  const int obs = OT == 0 ? wp.c[0].Cout / 32 : wp.obs;      // OT == 0: wgrad7 / wgrad8 (output chunks of 32)
  unsigned nw = (unsigned)(wp.ibs * obs * (wp.c[0].chunks + wp.c[1].chunks));
  if (OT == 0) nw = (unsigned)((wp.c[0].Cin / (32 * wp.c[0].icw)) * (wp.c[0].Cout / (32 * wp.c[0].ocw)) * wp.c[0].chunks + wp.ibs * obs * wp.c[1].chunks);
  hipLaunchKernelGGL((bwd7_kernel<CO, KMASK, TWS, OT, EPI, DBG>), dim3(cp.G + nw), dim3(512), lds, stream, cp.a, wp.c[0], wp.c[1], (int)cp.G, wp.ibs, obs);
}

// The same for a router-trunk layer (fp32 tensors on the bf16 pipe: conv6_split program + wgrad6<SPLIT> program).
template <int NT, int TWS, int OT>
__global__ __launch_bounds__(512) void bwd6s_kernel(C6SArgs c, W6Args a3, int G6, int ibs, int obs) {
  const int b = blockIdx.x;
  if (b < G6) { conv6s_body<NT>(c, b, G6); return; }
  int r = b - G6;
  const int bx = r % ibs; r /= ibs;
  wgrad6_body<3, TWS, OT, true>(a3, bx, r % obs, r / obs);
}
template <int NT, int TWS, int OT>
void launch_bwd6s(const C6SPlan& cp, const W6DualPlan& wp, hipStream_t stream) {
  static unsigned long long attr = 0;
  if (hdmoe_first_on_device(attr)) { (void)hipFuncSetAttribute((const void*)bwd6s_kernel<NT, TWS, OT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
  const size_t lds = cp.lds > wp.lds ? cp.lds : wp.lds;
  const unsigned grid = cp.G + (unsigned)(wp.ibs * wp.obs * wp.c[0].chunks);
  hipLaunchKernelGGL((bwd6s_kernel<NT, TWS, OT>), dim3(grid), dim3(512), lds, stream, cp.sa, wp.c[0], (int)cp.G, wp.ibs, wp.obs);
}

}  // namespace

extern "C" {

/* hdmoe_conv_bwd6 for fp32 tensors computed as split bf16 (3x3 layers of the router trunks): wd = [hi | lo] bf16 dgrad image with
 * `wd_plane` elements per plane. */
int hdmoe_conv_bwd6s(const void* x, const void* dy, const void* wd, void* dx, float* const* G, const int* seg, int ngroups, long wd_stride,
                     long wd_plane, int N, int H, int W, int Cin, int Cout, const int* kh, const int* kw, const int* pt, const int* pl,
                     float alpha, void* ws, long ws_bytes, const float* in_scale, const float* in_shift, int in_relu, int hi_only, hipStream_t stream) {
  if (!dx || !wd || ngroups < 1 || ngroups > HDMOE_MAX_GROUPS || Cout % 16) return 1;
  W6DualPlan wp;
  if (wgrad6_plan_split(x, dy, G, seg, ngroups, N, H, W, Cin, Cout, kh, kw, pt, pl, ws, ws_bytes, wp)) return 1;
  if ((in_scale == nullptr) != (in_shift == nullptr) || (in_scale && (ngroups != 1 || seg))) return HDMOE_EINVAL;
  wp.c[0].in_scale = in_scale; wp.c[0].in_shift = in_shift; wp.c[0].in_relu = in_relu;   // the weight gradient sees relu(x * scale + shift)
  wp.c[0].hi_only = hi_only ? 1 : 0;
  const ConvArgs c = conv_dgrad_args(dy, wd, dx, seg, ngroups, wd_stride, N, H, W, Cin, Cout, kh, kw, pt, pl, alpha);   // (3 x 3, pad 1: wgrad6_plan_split)
  C6SPlan cp;
  if (conv6s_plan(c, wd_plane, nullptr, cp)) return 1;
  cp.sa.nprod = hi_only ? 1 : 3;
  hdmoe_count_selection(HDMOE_SEL_BWD6S);
  conv_pick<2, 1>(cp.NT, [&](auto Nt) { conv_pick<5, 4>(wp.TWS, [&](auto Tws) { conv_pick<2, 1>(wp.OT, [&](auto Ot) {
    launch_bwd6s<decltype(Nt)::value, decltype(Tws)::value, decltype(Ot)::value>(cp, wp, stream);
  }); }); });
  return hdmoe_launch_status();
}

/* dx = alpha * dgrad(dy, wd)  and  partial slabs of dW into ws (deferred reduction, as hdmoe_conv_wgrad6(..., defer = 1)) for one grouped
 * k x k bf16 layer with 3x3 and 5x5 experts (stride 1, "same" padding pt = (k - 1) / 2).  wd: flipped dgrad weight image
 * [g][tap][Cin][Cout] (hdmoe_wprep_fwd / the weight bank).  Returns 1 without launching when the layer is outside the domain. */
int hdmoe_conv_bwd6(const void* x, const void* dy, const void* wd, void* dx, float* const* G, const int* seg, int ngroups, long wd_stride,
                    int N, int H, int W, int Cin, int Cout, const int* kh, const int* kw, const int* pt, const int* pl, float alpha,
                    void* ws, long ws_bytes, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || !dx || !wd || ngroups < 1 || ngroups > HDMOE_MAX_GROUPS || Cout % 16) return 1;
  W6DualPlan wp;
  if (wgrad6_plan_dual(x, dy, G, seg, ngroups, N, H, W, Cin, Cout, kh, kw, pt, pl, ws, ws_bytes, dtype, wp)) return 1;
  const ConvArgs c = conv_dgrad_args(dy, wd, dx, seg, ngroups, wd_stride, N, H, W, Cin, Cout, kh, kw, pt, pl, alpha);
  {
    C7Plan cp7;                                            // 32 x 32 maps: the streaming kernel as the dgrad program (wgrad6 handles 3x3 / 5x5 only)
    if (!conv7_plan(c, dtype, cp7) && cp7.kmask == 3 && (cp7.w16 != 0) == (wp.TWS == 4)) {
      if (wp.TWS == 5) {
        hdmoe_count_selection(HDMOE_SEL_BWD7_32);
        if (wp.c[0].chunks) {
          hdmoe_count_selection(HDMOE_SEL_BWD7_32_WGRAD8);
          hdmoe_count_selection(wp.c[0].icw == 2 ? (wp.c[0].ocw == 2 ? HDMOE_SEL_WGRAD8_C22 : HDMOE_SEL_WGRAD8_C21)
                                                 : (wp.c[0].ocw == 2 ? HDMOE_SEL_WGRAD8_C12 : HDMOE_SEL_WGRAD8_C11));
        }
        if (wp.c[1].chunks) hdmoe_count_selection(HDMOE_SEL_BWD7_32_WGRAD7);
      } else {
        hdmoe_count_selection(wp.OT == 2 ? HDMOE_SEL_BWD7_16_OT2 : HDMOE_SEL_BWD7_16_OT1);
      }
      conv_pick<2, 1>(cp7.CO, [&](auto Co) {           // 32 x 32 maps: wgrad7 / wgrad8 (OT = 0); 16 x 16: the wgrad6 programs
        if (wp.TWS == 5) launch_bwd7<decltype(Co)::value, 3, 5, 0>(cp7, wp, stream);
        else conv_pick<2, 1>(wp.OT, [&](auto Ot) { launch_bwd7<decltype(Co)::value, 3, 4, decltype(Ot)::value>(cp7, wp, stream); });
      });
      return hdmoe_launch_status();
    }
  }
  C6Plan cp;
  if (conv6_plan(c, dtype, cp)) return 1;
  hdmoe_count_selection(HDMOE_SEL_BWD6);
  conv_pick<2, 1>(cp.MT, [&](auto M) { conv_pick<2, 1>(cp.NT, [&](auto Nt) { conv_pick<5, 4>(wp.TWS, [&](auto Tws) { conv_pick<2, 1>(wp.OT, [&](auto Ot) {
    launch_bwd6<decltype(M)::value, decltype(Nt)::value, decltype(Tws)::value, decltype(Ot)::value>(cp, wp, stream);
  }); }); }); });
  return hdmoe_launch_status();
}

/* hdmoe_conv_bwd6 for a layer whose input is h = dropout_p(mp_silu(u * e[n][c])) (conv_res2 of Unet_block) and feeds nothing else: the dgrad
 * program applies the FiLM backward in its epilogue, so dx receives du = d(loss)/du and film_de [N][Cin] fp32 the per-sample gradient of e
 * (written, not accumulated), as hdmoe_film_silu_drop_bwd would compute them from the dx of hdmoe_conv_bwd6 (du bit-identical).
 * film_mask: the keep bytes of hdmoe_film_silu_drop_fwd_mask, or NULL with film_p == 0 (no dropout).  Returns 1 without launching when the
 * layer is outside the epilogue's domain (the caller then takes hdmoe_conv_bwd6 and the standalone FiLM backward). */
int hdmoe_conv_bwd6_film(const void* x, const void* dy, const void* wd, void* dx, float* const* G, const int* seg, int ngroups, long wd_stride,
                         int N, int H, int W, int Cin, int Cout, const int* kh, const int* kw, const int* pt, const int* pl, float alpha,
                         void* ws, long ws_bytes, const void* film_u, const float* film_e, const unsigned char* film_mask, float* film_de,
                         float film_p, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || !dx || !wd || ngroups < 1 || ngroups > HDMOE_MAX_GROUPS || Cout % 16) return 1;
  if (!film_u || !film_e || !film_de || ((uintptr_t)film_u & 15) || ((uintptr_t)film_e & 15)) return 1;
  if (film_p < 0.f || film_p >= 1.f || (film_p > 0.f) != (film_mask != nullptr)) return HDMOE_EINVAL;
  W6DualPlan wp;
  if (wgrad6_plan_dual(x, dy, G, seg, ngroups, N, H, W, Cin, Cout, kh, kw, pt, pl, ws, ws_bytes, dtype, wp)) return 1;
  const ConvArgs c = conv_dgrad_args(dy, wd, dx, seg, ngroups, wd_stride, N, H, W, Cin, Cout, kh, kw, pt, pl, alpha);
  C7Plan cp7;
  if (conv7_plan(c, dtype, cp7) || cp7.kmask != 3 || (cp7.w16 != 0) != (wp.TWS == 4)) return 1;
  // the instantiations with the epilogue: 32 x 32 maps with either output-block width, 16 x 16 maps with 64-channel blocks on both sides
  // (the bwd7 kernels of the bench's blocks); any number of output blocks
  const bool big = wp.TWS == 5, small = wp.TWS == 4 && cp7.CO == 2 && wp.OT == 2;
  if (!big && !small) return 1;
  cp7.a.film_u = film_u; cp7.a.film_e = film_e; cp7.a.film_mask = film_mask; cp7.a.film_de = film_de;
  cp7.a.film_inv = film_p > 0.f ? 1.f / (1.f - film_p) : 1.f;
  hdmoe_count_selection(HDMOE_SEL_FILM_DGRAD);
  if (big) {
    hdmoe_count_selection(HDMOE_SEL_BWD7_32);
    if (wp.c[0].chunks) {
      hdmoe_count_selection(HDMOE_SEL_BWD7_32_WGRAD8);
      hdmoe_count_selection(wp.c[0].icw == 2 ? (wp.c[0].ocw == 2 ? HDMOE_SEL_WGRAD8_C22 : HDMOE_SEL_WGRAD8_C21)
                                             : (wp.c[0].ocw == 2 ? HDMOE_SEL_WGRAD8_C12 : HDMOE_SEL_WGRAD8_C11));
    }
    if (wp.c[1].chunks) hdmoe_count_selection(HDMOE_SEL_BWD7_32_WGRAD7);
    if (cp7.CO == 2) launch_bwd7<2, 3, 5, 0, 1>(cp7, wp, stream); else launch_bwd7<1, 3, 5, 0, 1>(cp7, wp, stream);
  } else {
    hdmoe_count_selection(HDMOE_SEL_BWD7_16_OT2);
    launch_bwd7<2, 3, 4, 2, 1>(cp7, wp, stream);
  }
  return hdmoe_launch_status();
}

}  // extern "C"
