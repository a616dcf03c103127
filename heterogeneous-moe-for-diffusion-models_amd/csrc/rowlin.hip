// Row GEMM for fp32 POINTWISE layers on FEW positions: y[p][o] = alpha * sum_i x[p][i] * w[g(p)][o][i] (+ beta * res[p][o]) for
// P = N * H * W <= 2048 positions (the time embedding, scaling_net, the router heads' time_linear / linear, and their input gradients as the
// same product on the flipped weight image).  The generic kernels of conv.hip give such a layer one 256-position tile per 64 output
// channels: 1 - 16 workgroups on a 256-CU chip (9 - 36 us, 50 us for the 1024 -> 2 layer on one workgroup), most of it staging through LDS
// between barriers.  Here ONE WAVE owns a (32 outputs x 32 positions) tile and is a workgroup of its own, so the 256 x 512 layer runs on
// 128 CUs; both operands are K-contiguous, so a lane reads 32 consecutive bytes of its row per 16 inputs straight from memory, a
// 64-input trip ahead of the MFMAs that consume it.  No LDS, no barrier, no atomics.
// THE SUM IS THE GENERIC KERNELS' SUM, bit for bit: one accumulator per output, K walked in 16-input chunks in increasing order, each
// chunk as mma32's eight v_mfma_f32_32x32x2_f32 (MFMA j contracts the inputs {j, 8 + j} of the chunk; A = weights, B = activations
// as in conv_fwd5), then alpha * acc (+ beta * res).  These layers feed the bf16 experts (time embedding, FiLM scales): a different
// fp32 order moves values across bf16 rounding boundaries and the step's outputs by 1e-2 of their maxima (DESIGN Round 14).  Splitting
// K over waves -- which is what would bring the longest layers to the launch floor -- is therefore not done.
// A row's result depends on that row and its group's weights alone; a tile that straddles a segment boundary makes one pass per group.
#include "common.h"
#include "conv_args.h"
#include "hdmoe.h"

namespace {

struct RlinArgs {
  const float* x; const float* w; float* y; const float* res; const int* seg;
  long wstride;
  int P, HW, I, Ipad, O, ngroups, vec;
  float alpha, beta;
};

typedef f32x4 rl_trip[8];                                    // a lane's share of a 64-input trip: 4 chunks x (inputs 8h .. 8h + 7)

DEVI void rl_load(const RlinArgs& a, const float* xr, const float* wr, int kk, int h, rl_trip& xv, rl_trip& wv) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {                                // clamped addresses; rl_mac masks (as in lwgrad.hip: no `cond ? load : 0`)
    const int k = kk + 16 * (q >> 1) + 8 * h + 4 * (q & 1);
    const int kc = k < a.I ? k : 0;
    xv[q] = *reinterpret_cast<const f32x4*>(xr + kc);
    wv[q] = *reinterpret_cast<const f32x4*>(wr + kc);
  }
}
DEVI void rl_mac(const RlinArgs& a, int kk, int h, const rl_trip& xv, const rl_trip& wv, f32x16& acc) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (kk + 16 * (q >> 1) >= a.I) break;                      // (uniform: a chunk of zeros adds nothing)
    const bool ok = kk + 16 * (q >> 1) + 8 * h + 4 * (q & 1) < a.I;
    const f32x4 x = ok ? xv[q] : (f32x4)(0.f), w = ok ? wv[q] : (f32x4)(0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[j], x[j], acc, 0, 0, 0);
  }
}

__global__ __launch_bounds__(64) void rowlin_f32_kernel(RlinArgs a) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int p0 = blockIdx.x * 32, o0 = blockIdx.y * 32;
  const int pend = min(p0 + 32, a.P);
  for (int g = 0; g < a.ngroups; ++g) {
    const int lo = max(p0, a.seg ? a.seg[g] * a.HW : 0), hi = min(pend, a.seg ? a.seg[g + 1] * a.HW : a.P);
    if (lo >= hi) continue;
    // positions outside the pass and outputs past O read a valid row instead: their products land in accumulator columns / rows nobody stores
    const int p = p0 + r, o = o0 + r;
    const bool pin = p >= lo && p < hi;
    const float* xr = a.x + (long)(pin ? p : lo) * a.I;
    const float* wr = a.w + (long)g * a.wstride + (long)(o < a.O ? o : o0) * a.Ipad;
    f32x16 acc = (f32x16)(0.f);
    rl_trip xa, wa, xb, wb;
    rl_load(a, xr, wr, 0, h, xa, wa);
    for (int kk = 0; kk < a.I; kk += 128) {
      const bool second = kk + 64 < a.I;
      if (second) rl_load(a, xr, wr, kk + 64, h, xb, wb);
      rl_mac(a, kk, h, xa, wa, acc);
      if (second) {
        if (kk + 128 < a.I) rl_load(a, xr, wr, kk + 128, h, xa, wa);
        rl_mac(a, kk + 64, h, xb, wb, acc);
      }
    }
    // accumulator element reg of this lane: output o0 + (reg & 3) + 8 * (reg >> 2) + 4 * h, position p0 + r -- four consecutive outputs per quad
    if (pin) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int oc = o0 + 8 * i + 4 * h;
        if (oc >= a.O) continue;
        const long off = (long)p * a.O + oc;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = a.alpha * acc[4 * i + j];
        if (a.vec) {                                          // O % 4 == 0: the four outputs exist and the address is 16-byte aligned
          if (a.res) {
            const f32x4 rv = *reinterpret_cast<const f32x4*>(a.res + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += a.beta * rv[j];
          }
          *reinterpret_cast<f32x4*>(a.y + off) = (f32x4){v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (oc + j < a.O) {
              if (a.res) v[j] += a.beta * a.res[off + j];
              a.y[off + j] = v[j];
            }
        }
      }
    }
  }
}

}  // namespace

// fp32 pointwise layer on at most 2048 positions: see rowlin_f32_kernel.  Same return convention as the other *_try_launch helpers
// (1 = outside the domain); tmpl[0] = the tile's outputs.
int rowlin_try_launch(const ConvArgs& c, int dtype, hipStream_t stream, int* tmpl) {
  if (dtype != HDMOE_F32 || c.stride != 1 || c.ones || c.win || c.Cin != c.Cphys || c.Cout != c.Cstore || c.Ho != c.H || c.Wo != c.W) return 1;
  const long P = (long)c.N * c.H * c.W;
  if (P < 1 || P > 2048 || c.Cin < 32 || c.Cin % 4 || c.Ipad % 4 || c.Ipad < c.Cin || c.wstride % 4 || c.Cout < 1) return 1;
  for (int g = 0; g < c.ngroups; ++g) if (c.kh[g] != 1 || c.kw[g] != 1 || c.pt[g] || c.pl[g]) return 1;
  if (((uintptr_t)c.x | (uintptr_t)c.w | (uintptr_t)c.y | (uintptr_t)c.res) & 15) return 1;
  if (tmpl) { tmpl[0] = 32; return 0; }
  RlinArgs a;
  a.x = (const float*)c.x; a.w = (const float*)c.w; a.y = (float*)c.y; a.res = (const float*)c.res; a.seg = c.seg; a.wstride = c.wstride;
  a.P = (int)P; a.HW = c.H * c.W; a.I = c.Cin; a.Ipad = c.Ipad; a.O = c.Cout; a.ngroups = c.ngroups; a.vec = c.Cout % 4 == 0;
  a.alpha = c.alpha; a.beta = c.beta;
  hipLaunchKernelGGL(rowlin_f32_kernel, dim3((unsigned)((P + 31) / 32), (unsigned)((c.Cout + 31) / 32)), dim3(64), 0, stream, a);
  return hdmoe_launch_status();
}
