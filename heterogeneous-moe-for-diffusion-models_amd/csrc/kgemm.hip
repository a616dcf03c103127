// Pointwise forward / dgrad with a LONG contraction and few outputs: y[m][o] = alpha * sum_k x[m][k] * w[o][k] + beta * res[m][o],
// K = Cin >= 512 (HDMOE_KGEMM_MINK), Cout <= 64, one expert.  These are the ViT experts' patch embedding (K = C * p^2 up to 8192 input features per
// token, reference models/model_components.py:670-679) and the input gradient of unpatch_proj (:700-706).  The general 1x1 path
// (conv.hip: conv_fwd5) tiles positions and walks K inside one workgroup: with 2048 tokens that is 8 workgroups on a 256-CU chip
// (285 us for a 33 MB read).  Here both operands are K-contiguous in memory, so MFMA fragments are plain 16-byte global loads (no
// LDS): a workgroup owns 32 rows, its eight waves split K in 64-element chunks (a lane reads 64 contiguous bytes of its row per
// chunk = four k-steps; the k <-> MFMA-slot assignment is arbitrary as long as both operands use the same one), and the partial
// sums meet in LDS in wave order (pw_stream.h pws_put / pws_sum: deterministic forward).
// DUAL (hdmoe_kgemm2_fwd): two 32-output layers over the SAME x in one launch -- tile 0 is layer 1 (w, y, alpha), tile 1 is layer 2 (w2,
// y2, alpha2); x is read once.  Each output's products, chunk split and meeting order are those of its own NT = 1 launch: bit-equal.
#include "common.h"
#include "conv_args.h"
#include "pw_stream.h"
#include "hdmoe.h"

namespace {

struct KArgs {
  const bf16* x; const bf16* w; bf16* y; const bf16* res; long M; int K, O; float alpha, beta;
  const int* rows; long HW;     // rows = DEVICE {begin, end}: only the positions [begin * HW, end * HW) (null: all M)
  const bf16* w2; bf16* y2; float alpha2;   // DUAL only
};

template <int NT, bool DUAL = false>
__global__ __launch_bounds__(512) void kgemm_kernel(KArgs a) {
  extern __shared__ __attribute__((aligned(16))) float red[];   // [8 waves][NT][16 regs][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  long mb = 0, me = a.M;
  if (a.rows) {                                                // tiles are counted from the window's first position: all of them are full
    const long N = a.M / a.HW;
    long b = a.rows[0], e = a.rows[1];
    b = b < 0 ? 0 : (b > N ? N : b);
    e = e < b ? b : (e > N ? N : e);
    mb = b * a.HW; me = e * a.HW;
  }
  const long m0 = mb + (long)blockIdx.x * 32;
  if (m0 >= me) return;
  const long mr = m0 + r < me ? m0 + r : me - 1;               // rows past the end read the last row, are never stored
  const bf16* xrow = a.x + mr * a.K + 32 * h;
  const bf16* wrow = a.w + (long)r * a.K + 32 * h;
  const bf16* wrow2 = DUAL ? a.w2 + (long)r * a.K + 32 * h : nullptr;
  static_assert(!DUAL || NT == 2, "two layers = two tiles");
  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x16)(0.f);
  const int nchunks = a.K >> 6;
  uint4 fx[2][4], fw[2][NT][4];
  auto load = [&](int buf, int c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) fx[buf][j] = *reinterpret_cast<const uint4*>(xrow + 64 * c + 8 * j);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) fw[buf][t][j] = *reinterpret_cast<const uint4*>((DUAL ? (t ? wrow2 : wrow) : wrow + (long)32 * t * a.K) + 64 * c + 8 * j);
  };
  auto mma = [&](int buf) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fw[buf][t][j]), __builtin_bit_cast(bf16x8, fx[buf][j]), acc[t], 0, 0, 0);
  };
  int c = wave;
  if (c < nchunks) load(0, c);
  for (; c < nchunks; c += 16) {
    if (c + 8 < nchunks) load(1, c + 8);
    mma(0);
    if (c + 8 < nchunks) {
      if (c + 16 < nchunks) load(0, c + 16);
      mma(1);
    }
  }
  pws_put<NT>(red, wave, lane, acc);
  __syncthreads();
  for (int e = tid; e < NT * 1024; e += 512) {
    const int l = e & 63, reg = (e >> 6) & 15, t = e >> 10;
    float v = pws_sum<8, NT>(red, e);
    const long m = m0 + (l & 31);
    const int o = (DUAL ? 0 : 32 * t) + acc_row(reg, l);
    if (m < me) {
      if constexpr (DUAL) {
        v *= t ? a.alpha2 : a.alpha;
        (t ? a.y2 : a.y)[m * 32 + o] = (bf16)v;
      } else {
        v *= a.alpha;
        if (a.res) v += a.beta * (float)a.res[m * a.O + o];
        a.y[m * a.O + o] = (bf16)v;
      }
    }
  }
}

}  // namespace

// Returns HDMOE_OK after launching, a negative status on a launch error, or 1 when the layer is outside this file's domain.
// rows != null: the row window of hdmoe_pw_fwd_rows (HW positions per row), on the all-rows grid.
int kgemm_try_launch(const ConvArgs& a, int dtype, hipStream_t stream, const int* rows, long HW, int* tmpl) {
  if (dtype != HDMOE_BF16 || a.ngroups != 1 || a.seg || a.stride != 1 || a.ones || a.kh[0] != 1 || a.kw[0] != 1 || a.pt[0] || a.pl[0]) return 1;
  constexpr int mink = 512;   // (768: the text projections of the fusion cross-attention, 37 + 31 -> ~2 x 12 us on the serial stage; same-box step -0.1 ms)
  if (a.Cin != a.Cphys || a.Ipad != a.Cin || a.Cin % 64 || a.Cin < mink || a.Cout != a.Cstore || a.Cout % 32 || a.Cout > 64) return 1;
  if (a.Ho != a.H || a.Wo != a.W || (((uintptr_t)a.x | (uintptr_t)a.w) & 15)) return 1;
  KArgs k;
  k.x = (const bf16*)a.x; k.w = (const bf16*)a.w; k.y = (bf16*)a.y; k.res = (const bf16*)a.res;
  k.M = (long)a.N * a.H * a.W; k.K = a.Cin; k.O = a.Cout; k.alpha = a.alpha; k.beta = a.beta;
  k.rows = rows; k.HW = HW; k.w2 = nullptr; k.y2 = nullptr; k.alpha2 = 0.f;
  if (rows && (HW < 1 || k.M % HW)) return 1;
  const long blocks = (k.M + 31) / 32;
  if (blocks > 0x7fffffffl) return 1;
  const int NT = a.Cout / 32;
  if (tmpl) { tmpl[0] = NT; return 0; }
  const size_t lds = (size_t)8 * NT * 4096;
  conv_pick<1, 2>(NT, [&](auto Nt) { hipLaunchKernelGGL(kgemm_kernel<decltype(Nt)::value>, dim3((unsigned)blocks), dim3(512), lds, stream, k); });
  return hdmoe_launch_status();
}

// Two pointwise layers with 32 outputs each over the same x [M][K] in one launch (the k / v projections of a cross-attention over a long
// context feature): y1 = alpha1 x w1^T, y2 = alpha2 x w2^T, w1 / w2 the prepared forward images [32][K].  Same domain as the single layer
// (K % 64 == 0, K >= 512, 16-byte aligned x and images); 1 outside it, nothing launched.
extern "C" int hdmoe_kgemm2_fwd(const void* x, const void* w1, const void* w2, void* y1, void* y2, long M, int K, float alpha1, float alpha2,
                                int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || K % 64 || K < 512) return 1;
  if (!x || !w1 || !w2 || !y1 || !y2 || M < 0) return HDMOE_EINVAL;
  if ((((uintptr_t)x | (uintptr_t)w1 | (uintptr_t)w2) & 15) || (((uintptr_t)y1 | (uintptr_t)y2) & 1)) return 1;
  const long blocks = (M + 31) / 32;
  if (blocks > 0x7fffffffl) return 1;
  if (M == 0) return HDMOE_OK;
  KArgs k;
  k.x = (const bf16*)x; k.w = (const bf16*)w1; k.y = (bf16*)y1; k.res = nullptr; k.M = M; k.K = K; k.O = 32; k.alpha = alpha1; k.beta = 0.f;
  k.rows = nullptr; k.HW = 0; k.w2 = (const bf16*)w2; k.y2 = (bf16*)y2; k.alpha2 = alpha2;
  hipLaunchKernelGGL((kgemm_kernel<2, true>), dim3((unsigned)blocks), dim3(512), (size_t)8 * 2 * 4096, stream, k);
  return hdmoe_launch_status();
}
