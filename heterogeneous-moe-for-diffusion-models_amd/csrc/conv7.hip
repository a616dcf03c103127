// K3 (third generation): whole-image streaming convolution for the k x k expert layers on 32 x 32 feature maps -- forward and dgrad of
// MP_Conv (reference models/model_internals.py:253-275), all experts of a layer in one launch (models/model_config1.py:25-37).
// Design notes: conv7_body.h.  Domain: bf16, stride 1, H = W = 32 or H = W = 16, square k in {3, 5, 7} with "same" padding (k - 1) / 2,
// Cin % 32 == 0 (<= 256), Cout % 32 == 0 (<= 256), at least C7_MIN_IMAGES images (a unit is a whole image: fewer images than CUs leave CUs idle,
// conv6's 256-pixel units fill the chip better then).  Everything else stays on conv6 / conv.hip.
#include "conv_args.h"
#include "hdmoe.h"
#include "conv7_body.h"

namespace {

template <int CO, int KMASK, bool W16, bool DBG>
__global__ __launch_bounds__(512) void conv7_kernel(C7Args a) { conv7_body<CO, KMASK, W16, 0, DBG>(a, blockIdx.x, gridDim.x); }

}  // namespace

constexpr int C7_MIN_IMAGES = 192;
extern "C" int hdmoe_conv7_min_images(void) { return C7_MIN_IMAGES; }

// 0 = planned, 1 = outside the domain
int conv7_plan(const ConvArgs& c, int dtype, C7Plan& plan) {
  if (dtype != HDMOE_BF16 || c.stride != 1 || c.ones || c.Cphys != c.Cin || c.Ipad != c.Cin || c.Cin % 32 || c.Cin > 256 || c.Cstore != c.Cout) return 1;
  if (c.Cout % 32 || c.Cout > 256) return 1;                 // (more than 64 output channels: blocks of 64 / 32 walked over the same image)
  const bool w16 = c.H == 16;
  if (!((c.H == 32 && c.W == 32) || (c.H == 16 && c.W == 16)) || c.Ho != c.H || c.Wo != c.W || c.N < C7_MIN_IMAGES) return 1;
  int kmask = 0;
  long maxtaps = 0;
  for (int g = 0; g < c.ngroups; ++g) {
    const int k = c.kh[g];
    if (c.kw[g] != k || (k != 3 && k != 5 && k != 7) || c.pt[g] != (k - 1) / 2 || c.pl[g] != (k - 1) / 2) return 1;
    kmask |= k == 3 ? 1 : (k == 5 ? 2 : 4);
    if ((long)k * k > maxtaps) maxtaps = (long)k * k;
  }
  const long xbytes = (long)c.N * c.H * c.W * c.Cin * 2;
  const long wbytes = ((long)(c.ngroups - 1) * c.wstride + maxtaps * c.Cout * c.Cin) * 2;
  if (!conv_align_extent_ok({c.x, c.w, c.y, c.res}, {xbytes, wbytes, (long)c.N * c.H * c.W * c.Cout})) return 1;
  // the kernel builds its DMA offsets from these byte strides in 32-bit registers: the largest offset of either operand stays below 2^31,
  // and a group's base is a multiple of 8 (its low bits carry the kernel size)
  const long gstride = c.wstride * 2, tapstride = (long)c.Cout * c.Cin * 2, imgstride = (long)c.H * c.W * c.Cin * 2;
  if ((gstride & 7) || (c.ngroups - 1) * gstride + maxtaps * tapstride >= (1l << 31) || c.N * imgstride >= (1l << 31)) return 1;
  C7Args& a = plan.a;
  a.x = c.x; a.w = c.w; a.y = c.y; a.res = c.res; a.seg = c.seg;
  a.N = c.N; a.Cin = c.Cin; a.Cout = c.Cout; a.ngroups = c.ngroups; a.alpha = c.alpha; a.beta = c.beta;
  a.xbytes = (int)xbytes; a.wbytes = (int)wbytes;
  a.dbg = 0;
  a.film_u = nullptr; a.film_e = nullptr; a.film_mask = nullptr; a.film_de = nullptr; a.film_inv = 1.f;   // (hdmoe_conv_bwd6_film sets them)
  a.stamps = (unsigned long long*)hdmoe_debug_stamp_buffer();
  conv_sort_groups_desc(c.kh, a.order, c.ngroups);          // heaviest images first
  for (int i = 0; i < HDMOE_MAX_GROUPS; ++i) a.gk[i] = (int)(a.order[i] * gstride) | c.kh[a.order[i]];
  const long gcap = 256;
  const long units = w16 ? (c.N + 1) / 2 + c.ngroups : c.N;    // (16 x 16: pairs of images of one expert; an upper bound for any routing)
  plan.G = (unsigned)(units < gcap ? units : gcap);
  plan.CO = c.Cout % 64 == 0 ? 2 : 1;
  a.tapstride = (int)tapstride; a.blkstride = 32 * plan.CO * c.Cin * 2;
  a.imgstride = (int)imgstride; a.rowstride = c.W * c.Cin * 2;
  plan.w16 = w16 ? 1 : 0;
  plan.lds = w16 ? C7Lds<true>::BYTES : C7Lds<false>::BYTES;
  plan.kmask = (kmask & 4) ? 7 : 3;                          // instantiated kernel-size sets: {3, 5} and {3, 5, 7}
  return 0;
}

template <int CO, int KMASK, bool W16, bool DBG>
static void conv7_launch_t(const C7Plan& p, hipStream_t stream) {
  static unsigned long long attr = 0;
  if (hdmoe_first_on_device(attr)) { (void)hipFuncSetAttribute((const void*)conv7_kernel<CO, KMASK, W16, DBG>, hipFuncAttributeMaxDynamicSharedMemorySize, C7Lds<W16>::BYTES); }
  hipLaunchKernelGGL((conv7_kernel<CO, KMASK, W16, DBG>), dim3(p.G), dim3(512), C7Lds<W16>::BYTES, stream, p.a);
}

void conv7_launch(const C7Plan& p, hipStream_t stream) {
  conv_pick<2, 1>(p.CO, [&](auto Co) { conv_pick<7, 3>(p.kmask, [&](auto Km) { conv_pick<1, 0>(p.w16 != 0, [&](auto W16) {
    // the development kernel (stamps, ablations) only while a stamp buffer is registered or an ablation is set; {3, 5} layers only
    if constexpr (decltype(Km)::value == 3) {
      if (p.a.stamps || p.a.dbg) { conv7_launch_t<decltype(Co)::value, 3, decltype(W16)::value != 0, true>(p, stream); return; }
    }
    conv7_launch_t<decltype(Co)::value, decltype(Km)::value, decltype(W16)::value != 0, false>(p, stream);
  }); }); });
}

int conv7_try_launch(const ConvArgs& c, int dtype, hipStream_t stream, int* tmpl) {
  C7Plan plan;
  if (conv7_plan(c, dtype, plan)) return 1;
  if (tmpl) { tmpl[0] = plan.CO; tmpl[1] = plan.kmask; tmpl[2] = plan.w16; return 0; }
  hdmoe_count_selection(plan.w16 ? HDMOE_SEL_CONV7_16 : HDMOE_SEL_CONV7_32);
  conv7_launch(plan, stream);
  return hdmoe_launch_status();
}
