// Backward of the POINTWISE weight-bank layers (linear / 1x1 conv, stride 1, bf16) in ONE launch:
//   dx[p][i]    = alpha * sum_o dy[p][o] * w_g[o][i]          (tensor dtype; w from the flipped image wd [g][I][O], as conv.hip's dgrad reads it)
//   G[g][o][i] += sum_p dy[p][o] * x[p][i]                    (fp32, the bank's [tap = 1][O][I] slabs, as lwgrad.hip)
// Until round 6 a layer paid two launches for this (the general conv kernel on wd, then lwg_bf16_kernel), each reading all of dy.  The
// weights are at most 128 x 64, so the layer is pure streaming: its floor is one read of dy, one of x and one write of dx.
//
// A wave streams 64-position slices through pw_stream.h's PwsSlice: 16-byte loads -> wave-private LDS sub-tiles [64 positions][64 B].
// The staged dy slice feeds BOTH products:
//   dW: ds_read_b64_tr_b16 of dy and x (8 consecutive positions of one channel per lane), 32x32x16 MFMAs contracting over positions;
//   dx: plain 16-byte reads of dy (8 consecutive channels o of one position per lane) as the B operand, the group's wd tile -- held in
//       registers for the life of the workgroup -- as the A operand: D[i][p] = sum_o wd[i][o] dy[p][o].  In this orientation a lane owns
//       4 consecutive channels i of one position, so the result goes back into the (now free) x sub-tiles with 8-byte writes and
//       leaves for HBM with the same coalesced 16-byte row pattern the loads use.
// Persistent grid: one or two workgroups per CU, each a contiguous range of slices inside ONE expert group (so the wd tile never
// changes; pws_slot), one flush of the dW tiles per workgroup: the four waves meet pairwise through LDS (pws_put's layout), then float
// atomics with a staggered start.
// Domain: bf16; Cin % 32 == 0, Cout % 32 == 0, both <= 128, (Cin / 32) * (Cout / 32) <= 8 (the dW accumulators of a larger layer no
// longer fit the register file next to the staging registers: 128 x 128, 128 x 96 and 96 x 96 stay on the two-launch path).
#include "common.h"
#include "conv_args.h"
#include "pw_stream.h"
#include "hdmoe.h"

namespace {

struct PbwArgs {
  const bf16* x; const bf16* dy; const bf16* wd; bf16* dx; float* G[HDMOE_MAX_GROUPS]; const int* seg;
  int ngroups, N, I, O, upw;
  long HW, wdstride;
  float alpha;
};

template <int OT, int IT>
__global__ __launch_bounds__(256) void pw_bwd_kernel(PbwArgs a) {
  // per wave: dy sub-tiles [OT][64 positions][64 B], x sub-tiles [IT][64][64 B] (the latter double as the dx staging tile);
  // the whole buffer is reused for the cross-wave reduction at the end
  constexpr int WB = (OT + IT) * 4096, T = OT * IT;
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int g; long p0, p1, u0, u1;
  if (!pws_slot(a.seg, a.ngroups, a.N, a.HW, a.upw, blockIdx.x, g, p0, p1, u0, u1)) return;
  bf16* DX = a.dx;
  unsigned char* mine = lds + wave * WB;
  const int r = lane & 31, h = lane >> 5;
  // the group's weights as MFMA A operands: rows = input channels i, k = 8 consecutive output channels o  (wd [I][O])
  bf16x8 wfr[IT][OT][2];
  {
    const bf16* WD = a.wd + (long)g * a.wdstride;
#pragma unroll
    for (int u = 0; u < IT; ++u)
#pragma unroll
      for (int t = 0; t < OT; ++t)
#pragma unroll
        for (int k2 = 0; k2 < 2; ++k2) wfr[u][t][k2] = *reinterpret_cast<const bf16x8*>(WD + (long)(32 * u + r) * a.O + 32 * t + 16 * k2 + 8 * h);
  }
  PwsSlice<OT, IT> s;                                          // (whole rows of dy and x: no column offsets)
  auto load = [&](long u) { s.load(a.dy, nullptr, a.x, a.O, a.I, 0, 0, p0 + (u << 6), p0, p1, lane); };
  f32x16 acc[OT][IT];
#pragma unroll
  for (int t = 0; t < OT; ++t)
#pragma unroll
    for (int u = 0; u < IT; ++u) acc[t][u] = (f32x16)(0.f);
  const long iters = (u1 - u0 + 3) >> 2;
  if (u0 + wave < u1) load(u0 + wave);
  for (long it = 0; it < iters; ++it) {
    const long u = u0 + wave + 4 * it;
    const bool valid = u < u1;
    pws_fence();
    if (valid) s.store(mine, lane);
    pws_fence();
    if (u + 4 < u1) load(u + 4);
    if (valid) {
      // dW += dy^T x over the slice's 64 positions
      s.mma(mine, lane, acc);
      pws_fence();                                                // x has been consumed: its sub-tiles take dx
      // dx^T[i][p] = sum_o wd[i][o] dy[p][o], 32 positions at a time
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        f32x16 ax[IT];
#pragma unroll
        for (int v = 0; v < IT; ++v) ax[v] = (f32x16)(0.f);
#pragma unroll
        for (int t = 0; t < OT; ++t)
#pragma unroll
          for (int k2 = 0; k2 < 2; ++k2) {
            const bf16x8 d = *reinterpret_cast<const bf16x8*>(mine + t * 4096 + (32 * hh + r) * 64 + (2 * k2 + h) * 16);
#pragma unroll
            for (int v = 0; v < IT; ++v) ax[v] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfr[v][t][k2], d, ax[v], 0, 0, 0);
          }
        // accumulator register 4 q + j of lane (r, h): channel i = 8 q + 4 h + j, position 32 hh + r
#pragma unroll
        for (int v = 0; v < IT; ++v)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            bf16x4 o4;
#pragma unroll
            for (int j = 0; j < 4; ++j) o4[j] = (bf16)(a.alpha * ax[v][4 * q + j]);
            *reinterpret_cast<bf16x4*>(mine + (OT + v) * 4096 + (32 * hh + r) * 64 + (8 * q + 4 * h) * 2) = o4;
          }
      }
      pws_fence();
      const long pb = p0 + (u << 6);
#pragma unroll
      for (int k = 0; k < 4 * IT; ++k) {
        const int e = lane + 64 * k, q = e / (4 * IT), pc = e % (4 * IT);
        const uint4 v = *reinterpret_cast<const uint4*>(mine + OT * 4096 + (pc >> 2) * 4096 + q * 64 + (pc & 3) * 16);
        if (pb + q < p1) *reinterpret_cast<uint4*>(DX + (pb + q) * a.I + pc * 8) = v;
      }
    }
  }
  // ---- one flush per workgroup: waves 2, 3 hand their tiles to waves 0, 1 through LDS, those two meet in the atomic pass
  float* red = reinterpret_cast<float*>(lds);                  // [2][T][16 regs][64 lanes]: lane-major, conflict-free both ways
  auto put = [&](int slot) {
#pragma unroll
    for (int t = 0; t < OT; ++t) pws_put<IT>(red, slot * OT + t, lane, acc[t]);
  };
  __syncthreads();                                             // every wave is done with its sub-tiles
  if (wave >= 2) put(wave - 2);
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int t = 0; t < OT; ++t)
#pragma unroll
      for (int v = 0; v < IT; ++v)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) acc[t][v][reg] += red[((wave * T + t * IT + v) * 16 + reg) * 64 + lane];
  }
  __syncthreads();
  if (wave < 2) put(wave);
  __syncthreads();
  // every workgroup of the group adds into the same [O][I] slab: start each one at a different element so that they do not all queue
  // on the same addresses at the same time
  float* G = a.G[g];
  const int rot = (int)((blockIdx.x * 17u) % (unsigned)(T * 4)) * 256;
  for (int e0 = tid; e0 < T * 1024; e0 += 256) {
    const int e = (e0 + rot) % (T * 1024);
    const int l = e & 63, reg = (e >> 6) & 15, tu = e >> 10;
    const float v = red[(tu * 16 + reg) * 64 + l] + red[((T + tu) * 16 + reg) * 64 + l];
    const int o = 32 * (tu / IT) + acc_row(reg, l), i = 32 * (tu % IT) + (l & 31);
    atomicAdd(&G[(long)o * a.I + i], v);
  }
}

template <int OT, int IT>
int pbw_launch(const PbwArgs& a, unsigned slots, size_t lds, hipStream_t stream) {
  static unsigned long long attr = 0;
  if (hdmoe_first_on_device(attr)) { (void)hipFuncSetAttribute((const void*)pw_bwd_kernel<OT, IT>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }
  hipLaunchKernelGGL((pw_bwd_kernel<OT, IT>), dim3(slots), dim3(256), lds, stream, a);
  return hdmoe_launch_status();
}

}  // namespace

extern "C" int hdmoe_pw_bwd(const void* x, const void* dy, const void* wd, void* dx, float* const* G, const int* seg, int ngroups,
                            long wd_stride, int N, long HW, int Cin, int Cout, float alpha, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || Cin < 32 || Cout < 32 || Cin % 32 || Cout % 32 || Cin > 128 || Cout > 128) return 1;
  const int OT = Cout / 32, IT = Cin / 32;
  if (OT * IT > 8) return 1;
  if (!x || !dy || !wd || !dx || !G || ngroups < 1 || ngroups > HDMOE_MAX_GROUPS || N < 0 || HW < 0) return HDMOE_EINVAL;
  if ((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)wd | (uintptr_t)dx) & 15) || wd_stride % 8 || wd_stride < (long)Cin * Cout) return 1;
  const long total = (long)N * HW;
  if (total == 0) return HDMOE_OK;
  if (total >= (1l << 40)) return 1;
  PbwArgs a;
  a.x = (const bf16*)x; a.dy = (const bf16*)dy; a.wd = (const bf16*)wd; a.dx = (bf16*)dx; a.seg = seg;
  a.ngroups = ngroups; a.N = N; a.HW = HW; a.I = Cin; a.O = Cout; a.wdstride = wd_stride; a.alpha = alpha;
  for (int g = 0; g < HDMOE_MAX_GROUPS; ++g) {
    a.G[g] = G[g < ngroups ? g : 0];
    if (!a.G[g]) return HDMOE_EINVAL;
  }
  const size_t stage = (size_t)4 * (OT + IT) * 4096, red = (size_t)2 * OT * IT * 4096;
  const size_t lds = stage > red ? stage : red;
  // persistent grid: two workgroups per CU where two fit the register file (OT + IT <= 3: occupancy 2 waves per SIMD), else one;
  // a whole number of slices per wave
  const long target = OT + IT <= 3 ? 512 : 256;
  const long units = (total + 63) / 64 + ngroups;                       // 64-position slices (upper bound over the experts' ragged ends)
  long upw = (units + target - 1) / target;
  upw = (upw + 3) / 4 * 4;
  if (upw > (1l << 24)) return 1;
  a.upw = (int)upw;
  const long slots = units / upw + ngroups + 1;
  if (slots >= (1l << 31)) return 1;
  hdmoe_count_selection(HDMOE_SEL_PW_BWD);
  int rc = 1;                                                             // (OT * IT <= 8 was checked above)
  conv_pick<1, 2, 3, 4>(OT, [&](auto Ot) { conv_pick<1, 2, 3, 4>(IT, [&](auto It) {
    constexpr int O = decltype(Ot)::value, I = decltype(It)::value;
    if constexpr (O * I <= 8) rc = pbw_launch<O, I>(a, (unsigned)slots, lds, stream);
  }); });
  return rc;
}
