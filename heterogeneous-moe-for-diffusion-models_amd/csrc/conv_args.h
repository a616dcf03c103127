// Argument block shared by the conv forward / dgrad kernels (conv.hip: v5 and the odd-shape kernels; conv6.hip: the
// persistent LDS-DMA pipelined kernel).
#pragma once
#include <initializer_list>
#include <type_traits>
#include "common.h"

struct ConvArgs {
  const void* x;      // [N][H][W][Cphys]
  const void* w;      // [g][tap][Cout][Ipad]
  void* y;            // [N][Ho][Wo][Cstore]
  const void* res;    // optional [N][Ho][Wo][Cstore]:  y = alpha*acc + beta*res
  const int* seg;     // [ngroups+1] row offsets or null
  long wstride;
  int N, H, W, Ho, Wo, Cin, Cphys, Ipad, Cout, Cstore, stride, ones, ngroups;
  int n0;             // first row of this launch (row-per-blockIdx.y kernels: 65535 rows per launch)
  int kh[HDMOE_MAX_GROUPS], kw[HDMOE_MAX_GROUPS], pt[HDMOE_MAX_GROUPS], pl[HDMOE_MAX_GROUPS];
  float alpha, beta;
  const int* win = nullptr;   // conv_fwd5 on a flattened pointwise layer (N = H = 1): DEVICE {begin, end}, only the positions
  int winL = 0;               //   [begin * winL, end * winL) of the one long row are computed (hdmoe_pw_fwd_rows); null: all
};

// ---- plan helpers shared by conv6_plan, conv6s_plan, conv7_plan and blk6_plan
// every pointer 16-byte aligned (null: absent) and every extent (bytes of a DMA operand, elements of an output) below 2^31
static inline bool conv_align_extent_ok(std::initializer_list<const void*> ptrs, std::initializer_list<long> extents) {
  for (const void* p : ptrs) if ((uintptr_t)p & 15) return false;
  for (long e : extents) if (e >= (1l << 31)) return false;
  return true;
}
// Template dispatch: f(std::integral_constant<int, A>) for the first listed A == v, else for the last one -- a plan's run-time integer
// becomes a template argument; nest one call per parameter.
template <int A, int... Rest, typename F> static inline void conv_pick(int v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, A>{});
  else if (v == A) f(std::integral_constant<int, A>{});
  else conv_pick<Rest...>(v, f);
}
// The same for the element type: f(float{}) for HDMOE_F32, else f(bf16{}) (the caller has checked the dtype code)
template <typename F> static inline void conv_pick_dtype(int dtype, F&& f) {
  if (dtype == HDMOE_F32) f(float{}); else f(bf16{});
}
// order[] = the groups by descending kernel size (longest units first; stable)
static inline void conv_sort_groups_desc(const int* ks, int* order, int ngroups) {
  for (int g = 0; g < HDMOE_MAX_GROUPS; ++g) order[g] = g;
  for (int i = 1; i < ngroups; ++i)
    for (int k = i; k > 0 && ks[order[k]] > ks[order[k - 1]]; --k) { const int t = order[k]; order[k] = order[k - 1]; order[k - 1] = t; }
}
// 2^32 / d + 1: x / d = (x * magic) >> 32 with a fix-up (c6_udiv); d == 1 would need 2^32 + 1 and takes the largest magic instead
static inline unsigned conv_recip(int d) { return d == 1 ? 0xFFFFFFFFu : (unsigned)((1ull << 32) / (unsigned)d + 1); }
// Largest weight stage (taps per stage, 9 .. 2) that fits: at most 40 DMA pieces per stage, fixed_lds_bytes + two stage buffers within cap;
// among those the fewest stages (barriers) over the groups, ties to the smaller stage (more even split of the taps).  0: none fits.
static inline int conv_pick_stage_T(int ngroups, const int* ks, int pieces_per_tap, long fixed_lds_bytes, int bytes_per_tap, long cap) {
  int best = 0, best_stages = 1 << 30;
  for (int t = 9; t >= 2; --t) {
    if (t * pieces_per_tap > 40 || fixed_lds_bytes + 2l * t * bytes_per_tap > cap) continue;
    int stages = 0;
    for (int g = 0; g < ngroups; ++g) stages += (ks[g] * ks[g] + t - 1) / t;
    if (stages <= best_stages) { best_stages = stages; best = t; }
  }
  return best;
}
// dst[0 .. HDMOE_MAX_GROUPS) = the per-group host array src[0 .. ngroups) (null: zeros); groups past ngroups repeat group 0
template <typename T> static inline void conv_fill_groups(T* dst, const T* src, int ngroups) {
  for (int g = 0; g < HDMOE_MAX_GROUPS; ++g) dst[g] = src ? src[g < ngroups ? g : 0] : T{};
}
// The argument block of one forward launch (n0 = 0); kh / kw / pt / pl are host arrays of ngroups entries.
static inline ConvArgs conv_fwd_args(const void* x, const void* w, void* y, const void* res, float alpha, float beta, const int* seg, int ngroups,
                                     long wstride, int N, int H, int W, int Ho, int Wo, int Cin, int Cphys, int Ipad, int Cout, int Cstore,
                                     int stride, int ones, const int* kh, const int* kw, const int* pt, const int* pl) {
  ConvArgs c;
  c.x = x; c.w = w; c.y = y; c.res = res; c.seg = seg; c.wstride = wstride;
  c.N = N; c.H = H; c.W = W; c.Ho = Ho; c.Wo = Wo; c.Cin = Cin; c.Cphys = Cphys; c.Ipad = Ipad; c.Cout = Cout; c.Cstore = Cstore;
  c.stride = stride; c.ones = ones; c.ngroups = ngroups; c.n0 = 0; c.alpha = alpha; c.beta = beta;
  conv_fill_groups(c.kh, kh, ngroups); conv_fill_groups(c.kw, kw, ngroups); conv_fill_groups(c.pt, pt, ngroups); conv_fill_groups(c.pl, pl, ngroups);
  return c;
}
// The input gradient of a stride-1 k x k layer as a forward conv over dy with the flipped weight image wd [g][tap][Cin][Cout]: the
// channel counts swap and the pads flip (k - 1 - p).  Cin / Cout are the layer's.
static inline ConvArgs conv_dgrad_args(const void* dy, const void* wd, void* dx, const int* seg, int ngroups, long wd_stride, int N, int H, int W,
                                       int Cin, int Cout, const int* kh, const int* kw, const int* pt, const int* pl, float alpha) {
  int fpt[HDMOE_MAX_GROUPS], fpl[HDMOE_MAX_GROUPS];
  for (int g = 0; g < ngroups; ++g) { fpt[g] = kh[g] - 1 - pt[g]; fpl[g] = kw[g] - 1 - pl[g]; }
  return conv_fwd_args(dy, wd, dx, nullptr, alpha, 0.f, seg, ngroups, wd_stride, N, H, W, H, W, Cout, Cout, Cout, Cin, Cin, 1, 0, kh, kw, fpt, fpl);
}

// Launch plan of the generic forward kernels (conv.hip): what hdmoe_conv_fwd launches when none of the specialised kernels below takes
// the layer.  conv_fwd_plan is pure (no HIP calls); HDMOE_EINVAL when the layer has more channel blocks than conv_fwd5 can address.
struct CvPlan {
  int kernel;                                  // HDMOE_ROUTE_CONV_FWD / _FWD2 / _FWD3 / _FWD5
  int NT;                                      // 32-channel tiles per workgroup (conv_fwd_kernel: its NB = 1, 2 or 4)
  int vec, lepi, NHR;                          // 16-byte input loads; fwd5: LDS-transposed epilogue, halo chunks per thread (7 or 9)
  int TH, TW, tiles_x, halo_cap, tg, ntiles;   // tile geometry; tg = kernel rows per weight stage (fwd5: its tg_flags word)
  dim3 grid;                                   // (grid.y = N: the row-per-blockIdx.y kernels run 65535 rows per launch)
  size_t lds;
};
int conv_fwd_plan(const ConvArgs& a, int dtype, CvPlan& p);

// Fused pro-/epilogue of the conv6 kernels (all optional):
//   in_scale/in_shift [N][Cin] fp32 + in_relu: the staged input is relu(x * scale[n][c] + shift[n][c]) -- GroupNorm(1,C) + ReLU of the
//   producing layer folded into this layer's staging pass (Router.hard_route, reference model_components.py:100-112);
//   stats [N][2] fp32 (caller zeroes): per-sample sum and sum of squares of the fp32 outputs, accumulated for the NEXT GroupNorm.
//   film_e != null (bf16 conv6 only): second output film_h = dropout_p(mp_silu(y * film_e[n][c])) (FiLM of Unet_block, conv6_common.h).
struct ConvFuse {
  const float* in_scale;
  const float* in_shift;
  float* stats;
  int in_relu;
  const float* film_e = nullptr; void* film_h = nullptr; const unsigned long long* film_seed_dev = nullptr;
  unsigned long long film_seed = 0; float film_p = 0.f;
};

// Returns HDMOE_OK after launching, a negative status on a launch error, or 1 when the shape is outside conv6's domain
// (the caller then takes the general kernels).  tmpl != null, here and in the forward *_try_launch helpers below: decide only -- same
// return value, nothing launched or counted, tmpl[] = the template arguments of the kernel that would run (include/hdmoe.h,
// hdmoe_conv_fwd_route).
int conv6_try_launch(const ConvArgs& a, const ConvFuse* fuse, int dtype, hipStream_t stream, int* tmpl = nullptr);

void* hdmoe_debug_stamp_buffer();     // development: the buffer registered with hdmoe_conv6_debug_stamps (conv6.hip), or null
void hdmoe_count_selection(int which);   // host-side kernel-selection counter HDMOE_SEL_* += 1 (conv.hip, hdmoe_kernel_selections)
// Whole-image streaming kernel for 32 x 32 maps (conv7.hip).  Same return convention.
int conv7_try_launch(const ConvArgs& a, int dtype, hipStream_t stream, int* tmpl = nullptr);

// Split-bf16 variant for fp32 tensors (conv6s.hip): w = bf16 [hi | lo][g][tap][Cout][Cin], `wplane_elems` elements per plane.
int conv6_split_try_launch(const ConvArgs& a, long wplane_elems, const ConvFuse* fuse, hipStream_t stream, int* tmpl = nullptr);

// Pointwise (linear / 1x1, stride 1) weight gradient (lwgrad.hip): G[g] [Cout][Cin] fp32 slabs (+=).  Same return convention.
// (lwgrad.hip's three: dry_run = decide only -- same return value, nothing launched)
int lwg_try_launch(const void* x, const void* dy, float* const* G, const int* seg, int ngroups, int N, long HW, int Cin, int Cout,
                   int dtype, hipStream_t stream, bool dry_run = false);

// Pointwise forward / dgrad with Cin >= 512 and Cout <= 64 (kgemm.hip).  Same return convention.
int kgemm_try_launch(const ConvArgs& a, int dtype, hipStream_t stream, const int* rows = nullptr, long HW = 0, int* tmpl = nullptr);

// k x k fp32 weight gradient for tiny input channel counts (taps * Cin <= 64: the stem), one expert (lwgrad.hip).  Same return convention.
int swg_try_launch(const void* x, const void* dy, float* G, int N, int H, int W, int Cin, int Cout, int k, int pt, int pl, int dtype,
                   hipStream_t stream, bool dry_run = false);

// k x k (k = 1 or 3) bf16 weight gradient for tiny output channel counts (Cout <= 4: output head, gate), one expert (lwgrad.hip).  Same return convention.
int towg_try_launch(const void* x, const void* dy, float* G, int N, int H, int W, int Cin, int Cout, int k, int pt, int pl, int dtype,
                    hipStream_t stream, bool dry_run = false);

// Grouped fp32 linear on one-position rows with a long input, 256 <= Cin <= 1024 (the experts' text projection; mlinear.hip).  Same return convention.
int glin_try_launch(const ConvArgs& a, int dtype, hipStream_t stream, int* tmpl = nullptr);

// fp32 pointwise forward / dgrad on at most 2048 positions, Cin >= 32 (the conditioning layers and the router heads; rowlin.hip).  Same return convention.
int rowlin_try_launch(const ConvArgs& a, int dtype, hipStream_t stream, int* tmpl = nullptr);
