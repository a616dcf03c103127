// Weight gradient of the POINTWISE layers (linear / 1x1 conv, stride 1): dW[g][o][i] += sum over the positions p of expert g's rows of
// dy[p][o] * x[p][i]  (autograd of MP_Conv with kernel () or (1,1), reference models/model_internals.py:253-275).
//
// A third of the step's launches are such layers (ViT linears, q/k/v/out projections, time / text embeddings of every block, 1x1 skips),
// and the tiled k x k kernel (conv.hip: conv_wgrad2) spent 20-40 us on each of them whatever their size: the contraction runs over
// positions and there is no halo to share, so the work is a tall-skinny GEMM that should cost its HBM read.  Here a wave streams
// 64-position slices of x and dy on its own:
//   bf16: 16-byte loads -> wave-private LDS rows -> both MFMA operands by transposing reads (ds_read_b64_tr_b16), 32x32x16 MFMAs;
//   fp32: no LDS at all -- for v_mfma_f32_32x32x2_f32 a lane supplies ONE element A[row = lane & 31][k = lane >> 5], which for
//         position-major tensors is exactly a coalesced 128-byte row load per half-wave (exact fp32 products; these layers are tiny).
// The four waves of a workgroup split the workgroup's slice range, add their accumulators through LDS and flush one [32*OT][32*IT]
// tile with float atomics (the slab is shared with the other position partitions, as in conv_wgrad2).  The slot decode, the bf16 slice
// pipeline, the hand-over of the accumulators, the flush and the launch plan are pw_stream.h's, shared with pbwd.hip, kgemm.hip and
// fusion.hip.
// Domain: Cin % 32 == 0, Cout % 32 == 0, no constant-one input channel; everything else stays with conv.hip.
#include "common.h"
#include "conv_args.h"
#include "pw_stream.h"
#include "hdmoe.h"

namespace {

struct LwgArgs {
  const void* x; const void* dy; float* G[HDMOE_MAX_GROUPS]; const int* seg;
  const void* dy2; float* G2;   // DUAL only (below)
  int ngroups, N, I, O, upw;
  long HW;
};

// the four waves' tiles meet in LDS (red: [4 waves][OT * IT] tiles, pw_stream.h) and go into the slab with float atomics (it is shared with the
// other position partitions).  DUAL: output tile t = 1 is the second layer's: rows o0 .. of its own slab G2
template <int OT, int IT, bool DUAL = false>
DEVI void lwg_flush(f32x16 (&acc)[OT][IT], float* red, float* G, int o0, int i0, int I, int tid, float* G2 = nullptr) {
#pragma unroll
  for (int t = 0; t < OT; ++t) pws_put<IT>(red, (tid >> 6) * OT + t, tid & 63, acc[t]);
  __syncthreads();
  const int rot = (int)((blockIdx.z * 131u + blockIdx.x * 17u) % (unsigned)(OT * IT * 4)) * 256;
  pws_flush<4, OT * IT>(red, tid, 256, rot, [&](int tu, int reg, int l) -> float* {
    const int o = o0 + (DUAL ? 0 : 32 * (tu / IT)) + acc_row(reg, l), i = i0 + 32 * (tu % IT) + (l & 31);
    return &((DUAL && tu / IT) ? G2 : G)[(long)o * I + i];
  });
}

// A wave streams its slices through PwsSlice (pw_stream.h): the next slice's loads are in flight while this one's MFMAs run.
// DUAL (hdmoe_lwgrad2): two layers with 32 outputs each over the SAME x -- the dy sub-tile t = 0 is read from dy, t = 1 from dy2 (both
// [P][32]) and the tiles flush into G / G2; x is read once.  Slices, waves and the order in which a workgroup sums are those of each
// layer's own OT = 1 launch.
template <int OT, int IT, bool DUAL = false>
__global__ __launch_bounds__(256) void lwg_bf16_kernel(LwgArgs a) {
  // per wave: dy sub-tiles [OT][64 positions][64 B], x sub-tiles [IT][64][64 B]; reused for the cross-wave reduction at the end
  constexpr int WB = (OT + IT) * 4096;
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * 32 * IT, o0 = blockIdx.y * 32 * OT;
  int g; long p0, p1, u0, u1;
  if (!pws_slot(a.seg, a.ngroups, a.N, a.HW, a.upw, blockIdx.z, g, p0, p1, u0, u1)) return;
  unsigned char* mine = lds + wave * WB;
  PwsSlice<OT, IT> s;
  auto load = [&](long u) {
    s.template load<DUAL>((const bf16*)a.dy, (const bf16*)a.dy2, (const bf16*)a.x, a.O, a.I, o0, i0, p0 + (u << 6), p0, p1, lane);
  };
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
    if (valid) s.mma(mine, lane, acc);
  }
  __syncthreads();                                            // every wave is done with its sub-tiles: the flush re-uses the whole buffer
  lwg_flush<OT, IT, DUAL>(acc, reinterpret_cast<float*>(lds), a.G[g], o0, i0, a.I, tid, a.G2);
}

template <int OT, int IT>
__global__ __launch_bounds__(256) void lwg_f32_kernel(LwgArgs a) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * 32 * IT, o0 = blockIdx.y * 32 * OT;
  int g; long p0, p1, u0, u1;
  if (!pws_slot(a.seg, a.ngroups, a.N, a.HW, a.upw, blockIdx.z, g, p0, p1, u0, u1)) return;
  const float* X = (const float*)a.x;
  const float* DY = (const float*)a.dy;
  const int r = lane & 31, h = lane >> 5;
  f32x16 acc[OT][IT];
#pragma unroll
  for (int t = 0; t < OT; ++t)
#pragma unroll
    for (int u = 0; u < IT; ++u) acc[t][u] = (f32x16)(0.f);
  // this wave's positions: the workgroup's range in 8-position steps, round-robin over the four waves
  const long pa = p0 + (u0 << 6), pe = (p0 + (u1 << 6)) < p1 ? (p0 + (u1 << 6)) : p1;
  for (long pb = pa + 8 * wave; pb < pe; pb += 32) {
    float dv[4][OT], xv[4][IT];
    bool okm[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {                              // loads from clamped addresses first, masks afterwards (a `cond ? load : 0`
      const long p = pb + 2 * s + h;                           //  form serialises the loads behind one another)
      okm[s] = p < pe;
      const long pc = okm[s] ? p : pa;
#pragma unroll
      for (int t = 0; t < OT; ++t) dv[s][t] = DY[pc * a.O + o0 + 32 * t + r];
#pragma unroll
      for (int v = 0; v < IT; ++v) xv[s][v] = X[pc * a.I + i0 + 32 * v + r];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int t = 0; t < OT; ++t) dv[s][t] = okm[s] ? dv[s][t] : 0.f;
#pragma unroll
      for (int v = 0; v < IT; ++v) xv[s][v] = okm[s] ? xv[s][v] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < OT; ++t)
#pragma unroll
        for (int v = 0; v < IT; ++v) acc[t][v] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[s][t], xv[s][v], acc[t][v], 0, 0, 0);
  }
  lwg_flush<OT, IT>(acc, reinterpret_cast<float*>(lds), a.G[g], o0, i0, a.I, tid);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k x k layers with a TINY input channel count (the stem: 4 latent channels -> 32, 3x3; reference model_config2.py:66-68 input_proj):
// taps * Cin <= 64 columns.  The tiled kernel pads Cin to 32 per tap (8x the work, 300 us); here the contraction over pixels runs on
// v_mfma_f32_32x32x2_f32 with A = dy[pixel][o] (a coalesced row load) and B = the im2col row of x built on the fly
// (column n = tap * Cin + i -> x[pixel + tap offset][i], zero outside the image): 2 MFMAs per 2 pixels per wave, HBM-bound on dy.
// A wave's trip is one memory latency (24 loads, then 16 MFMAs) and nothing in it overlaps the next trip's loads.  With four waves on a
// CU -- one workgroup per CU, so that the atomic flush of the 1152 words stays at 256 workgroups -- each SIMD holds ONE wave.  NW = 16
// waves per workgroup put four waves on every SIMD with the same number of workgroups and atomics; they meet in LDS ([NW][NBLK]
// accumulator tiles, 128 KB for the stem) before the one flush.  Stem launch in the replayed step: 68.8 -> 53 us (DESIGN Round 14);
// what holds the rest is not found yet (the MFMAs are 7 us, the 38 MB of HBM 8 us).
struct SwgArgs { const float* x; const float* dy; float* G; int N, H, W, Cin, Cout, k, pt, pl; long ppb; };

template <int NBLK, int NW>
__global__ __launch_bounds__(64 * NW) void swg_f32_kernel(SwgArgs a) {
  extern __shared__ __attribute__((aligned(16))) float red[];   // [NW waves][NBLK][16][64]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int o0 = blockIdx.y * 32;
  const long total = (long)a.N * a.H * a.W;
  const long p0 = (long)blockIdx.x * a.ppb, p1 = p0 + a.ppb < total ? p0 + a.ppb : total;
  const int ncols = a.k * a.k * a.Cin;
  int ky[NBLK], kx[NBLK], ci[NBLK]; bool colok[NBLK];
#pragma unroll
  for (int b = 0; b < NBLK; ++b) {
    const int n = 32 * b + r;
    colok[b] = n < ncols;
    const int tap = colok[b] ? n / a.Cin : 0;
    ci[b] = colok[b] ? n - tap * a.Cin : 0;
    ky[b] = tap / a.k - a.pt; kx[b] = tap % a.k - a.pl;
  }
  f32x16 acc[NBLK];
#pragma unroll
  for (int b = 0; b < NBLK; ++b) acc[b] = (f32x16)(0.f);
  // 8 k-steps (16 pixels of this wave) per trip: all their loads are issued before the first MFMA (one step at a time the loop ran at
  // one memory latency per step)
  for (long base = p0; base < p1; base += 16 * NW) {
    float dv[8], xv[8][NBLK];
    bool okm[8], inm[8][NBLK];
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      const long p = base + 2 * NW * st + 2 * wave + h;
      const bool ok = p < p1;
      const unsigned pc = (unsigned)(ok ? p : p0);               // 32-bit index arithmetic (64-bit div / mod cost ~500 instructions per step)
      const unsigned t = pc / (unsigned)a.W;
      const int xw = (int)(pc - t * (unsigned)a.W);
      const unsigned img = t / (unsigned)a.H;
      const int yh = (int)(t - img * (unsigned)a.H);
      // unconditional loads from clamped (always valid) addresses, masks applied after ALL loads of the trip are in flight: a
      // `cond ? load : 0` form made the compiler wait for every load before issuing the next (24 serial memory latencies per trip)
      dv[st] = a.dy[(long)pc * a.Cout + o0 + r];
      okm[st] = ok;
#pragma unroll
      for (int b = 0; b < NBLK; ++b) {
        const int yy = yh + ky[b], xx = xw + kx[b];
        const bool in = ok && colok[b] && (unsigned)yy < (unsigned)a.H && (unsigned)xx < (unsigned)a.W;
        inm[st][b] = in;
        xv[st][b] = a.x[in ? (((long)img * a.H + yy) * a.W + xx) * a.Cin + ci[b] : 0];
      }
    }
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      dv[st] = okm[st] ? dv[st] : 0.f;
#pragma unroll
      for (int b = 0; b < NBLK; ++b) xv[st][b] = inm[st][b] ? xv[st][b] : 0.f;
    }
#pragma unroll
    for (int st = 0; st < 8; ++st)
#pragma unroll
      for (int b = 0; b < NBLK; ++b) acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(dv[st], xv[st][b], acc[b], 0, 0, 0);
  }
  pws_put<NBLK>(red, wave, lane, acc);
  __syncthreads();
  const int rot = (int)((blockIdx.x * 37u) % (unsigned)(NBLK * 4)) * 256;
  pws_flush<NW, NBLK>(red, tid, 64 * NW, rot, [&](int b, int reg, int l) -> float* {
    const int o = o0 + acc_row(reg, l), n = 32 * b + (l & 31);
    if (n >= ncols) return nullptr;
    const int tap = n / a.Cin, i = n - tap * a.Cin;
    return &a.G[((long)tap * a.Cout + o) * a.Cin + i];
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// k x k (k = 1 or 3) bf16 layers with a TINY output channel count (Cout <= 4: the output head 32 -> IN_in_channels 3x3 and the 2-way
// gate 32 -> 2 1x1, reference model_config2.py output_proj / gate2).  The tiled kernel pads Cout to 32 rows per tap and took ~80 us
// per layer on the serial tail of the step for 0.6 GFLOP; here it is plain vector arithmetic: thread = (channel pair of x, one of 16
// pixel slices of an 8-row band), 9 x 4 x 2 fp32 accumulators, x straight from HBM (4 bytes per pixel-thread, 64 B per pixel over the
// 16 lanes of a channel chunk), dy with its halo converted to fp32 [pixel][4] in LDS (one 16-byte broadcast read per tap).  The
// slices meet by two cross-lane steps + LDS, one atomic flush of the <= 1152 words per workgroup.
struct TowgArgs { const bf16* x; const bf16* dy; float* G; int N, H, W, Cin, Cout, pad, TH, tiles_y, ntiles, wshift; };

template <int K>
__global__ __launch_bounds__(256) void towg_bf16_kernel(TowgArgs a) {
  constexpr int T = K * K;
  typedef __attribute__((ext_vector_type(2))) float f2;
  extern __shared__ __attribute__((aligned(16))) float tsm[];  // dy halo tile [(TH + K - 1)][(W + K - 1)][4], later the 4 waves' sums
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cp = tid & 15, sl = tid >> 4;
  const int c0 = blockIdx.y * 32 + 2 * cp;
  const int HWp = a.W + K - 1, HHp = a.TH + K - 1;
  f2 acc[T][4];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[t][o] = (f2)(0.f);
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int n = tile / a.tiles_y, y0 = (tile - n * a.tiles_y) * a.TH;
    __syncthreads();                                          // the previous tile's readers are done
    for (int e = tid; e < HHp * HWp; e += 256) {
      const int hy = e / HWp, hx = e - hy * HWp;
      const int iy = y0 + hy - a.pad, ix = hx - a.pad;
      f32x4 v = (f32x4)(0.f);
      if ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
        const bf16* d = a.dy + (((long)n * a.H + iy) * a.W + ix) * a.Cout;
        for (int o = 0; o < a.Cout; ++o) v[o] = (float)d[o];
      }
      *reinterpret_cast<f32x4*>(tsm + 4 * e) = v;
    }
    __syncthreads();
    const int rows = a.H - y0 < a.TH ? a.H - y0 : a.TH, npx = rows * a.W;
    const bf16* xb = a.x + ((long)n * a.H + y0) * a.W * a.Cin + c0;
#pragma unroll 2
    for (int p = sl; p < npx; p += 16) {
      const int y = a.wshift >= 0 ? p >> a.wshift : p / a.W, xx = p - y * a.W;
      const unsigned xw = *reinterpret_cast<const unsigned*>(xb + (long)p * a.Cin);
      const f2 xf = {__builtin_bit_cast(float, xw << 16), __builtin_bit_cast(float, xw & 0xFFFF0000u)};
      // dW[tap][o][i] = sum_p' x[p'][i] dy[p' - tap + pad][o]: halo coordinates (y + 2 pad - ty, x + 2 pad - tx)
      const float* dbase = tsm + 4 * ((y + K - 1) * HWp + xx + K - 1);
#pragma unroll
      for (int ty = 0; ty < K; ++ty)
#pragma unroll
        for (int tx = 0; tx < K; ++tx) {
          const f32x4 d = *reinterpret_cast<const f32x4*>(dbase - 4 * (ty * HWp + tx));
#pragma unroll
          for (int o = 0; o < 4; ++o) acc[ty * K + tx][o] += xf * d[o];
        }
    }
  }
  // the 4 pixel slices of a wave (lanes with equal cp), then the 4 waves
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float v = acc[t][o][j];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        acc[t][o][j] = v;
      }
  __syncthreads();
  if (lane < 16) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int j = 0; j < 2; ++j) tsm[((wave * T + t) * 4 + o) * 32 + 2 * lane + j] = acc[t][o][j];
  }
  __syncthreads();
  for (int e = tid; e < T * 4 * 32; e += 256) {
    const int i = e & 31, o = (e >> 5) & 3, t = e >> 7;
    if (o < a.Cout) {
      const float v = tsm[e] + tsm[T * 128 + e] + tsm[2 * T * 128 + e] + tsm[3 * T * 128 + e];
      atomicAdd(&a.G[((long)t * a.Cout + o) * a.Cin + blockIdx.y * 32 + i], v);
    }
  }
}

}  // namespace

// k x k bf16 weight gradient for Cout <= 4 (k = 1 or 3, one expert, stride 1, "same" geometry): G [tap][Cout][Cin] += .  Same return convention.
int towg_try_launch(const void* x, const void* dy, float* G, int N, int H, int W, int Cin, int Cout, int k, int pt, int pl, int dtype,
                    hipStream_t stream, bool dry_run) {
  if (dtype != HDMOE_BF16 || Cout < 1 || Cout > 4 || Cin % 32 || (k != 1 && k != 3) || pt != (k - 1) / 2 || pl != (k - 1) / 2) return 1;
  if (!x || !dy || !G || ((uintptr_t)x & 3)) return 1;
  TowgArgs a;
  a.x = (const bf16*)x; a.dy = (const bf16*)dy; a.G = G; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.pad = (k - 1) / 2;
  if (k == 1) {                                              // pointwise: no halo, the image shape is irrelevant (ops flattens such tensors
    const long total = (long)N * H * W;                       // to ONE row of N * H * W pixels): re-tile as rows of 256 pixels
    if (total % 256 == 0 && total / 256 < (1l << 30)) { a.N = 1; a.H = (int)(total / 256); a.W = 256; N = 1; H = a.H; W = 256; }
  }
  a.TH = H < 8 ? H : 8;
  if (k == 1 && H >= 4 && (long)N * ((H + 7) / 8) < 256) a.TH = 4;   // (enough tiles for every CU)
  while (a.TH > 1 && (size_t)(a.TH + k - 1) * (W + k - 1) * 16 > 48 * 1024) a.TH >>= 1;
  if ((size_t)(a.TH + k - 1) * (W + k - 1) * 16 > 48 * 1024) return 1;
  a.tiles_y = (H + a.TH - 1) / a.TH;
  const long ntiles = (long)N * a.tiles_y;
  if (ntiles >= (1l << 30)) return 1;
  a.ntiles = (int)ntiles;
  a.wshift = -1;
  for (int sft = 0; sft < 9; ++sft) if ((1 << sft) == W) a.wshift = sft;
  const int cb = Cin / 32;
  long nb = 256 / cb; if (nb < 1) nb = 1;                    // ~one workgroup per CU: every workgroup ends with a flush of the same words
  if (nb > ntiles) nb = ntiles;
  const size_t halo = (size_t)(a.TH + k - 1) * (W + k - 1) * 16, red = (size_t)4 * k * k * 128 * 4;
  const size_t lds = halo > red ? halo : red;
  const dim3 grid((unsigned)nb, (unsigned)cb);
  if (dry_run) return HDMOE_OK;
  if (k == 3) hipLaunchKernelGGL(towg_bf16_kernel<3>, grid, dim3(256), lds, stream, a);
  else hipLaunchKernelGGL(towg_bf16_kernel<1>, grid, dim3(256), lds, stream, a);
  return hdmoe_launch_status();
}

// k x k fp32 layer with taps * Cin <= 64 (one expert, stride 1, "same" geometry): G [tap][Cout][Cin] += .  Same return convention.
int swg_try_launch(const void* x, const void* dy, float* G, int N, int H, int W, int Cin, int Cout, int k, int pt, int pl, int dtype,
                   hipStream_t stream, bool dry_run) {
  if (dtype != HDMOE_F32 || Cout % 32 || k * k * Cin > 64 || !x || !dy || !G || (long)N * H * W >= (1l << 31)) return 1;
  if (dry_run) return HDMOE_OK;
  SwgArgs a;
  a.x = (const float*)x; a.dy = (const float*)dy; a.G = G; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.k = k; a.pt = pt; a.pl = pl;
  const long total = (long)N * H * W;
  long blocks = 256 / (Cout / 32); if (blocks < 1) blocks = 1;       // one workgroup per CU: more only adds atomic flushes of the same 1152 words
  // 16 waves per workgroup when every workgroup has at least one trip for each of them; four waves below that (small maps)
  const int NW = (total + blocks - 1) / blocks >= 16 * 16 ? 16 : 4;
  long ppb = (total + blocks - 1) / blocks; ppb = (ppb + 16 * NW - 1) / (16 * NW) * (16 * NW);
  a.ppb = ppb;
  const dim3 grid((unsigned)((total + ppb - 1) / ppb), Cout / 32);
  const int NBLK = (k * k * Cin + 31) / 32;
  if (NW == 16) {
    static unsigned long long attr_set = 0;
    if (hdmoe_first_on_device(attr_set)) {
      (void)hipFuncSetAttribute((const void*)swg_f32_kernel<1, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * 1 * 4096);
      (void)hipFuncSetAttribute((const void*)swg_f32_kernel<2, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * 2 * 4096);
    }
    if (NBLK == 1) hipLaunchKernelGGL((swg_f32_kernel<1, 16>), grid, dim3(1024), 16 * 1 * 4096, stream, a);
    else hipLaunchKernelGGL((swg_f32_kernel<2, 16>), grid, dim3(1024), 16 * 2 * 4096, stream, a);
  } else {
    if (NBLK == 1) hipLaunchKernelGGL((swg_f32_kernel<1, 4>), grid, dim3(256), 4 * 1 * 4096, stream, a);
    else hipLaunchKernelGGL((swg_f32_kernel<2, 4>), grid, dim3(256), 4 * 2 * 4096, stream, a);
  }
  return hdmoe_launch_status();
}

// Returns HDMOE_OK after launching, a negative status on a launch error, or 1 when the layer is outside this file's domain.
int lwg_try_launch(const void* x, const void* dy, float* const* G, const int* seg, int ngroups, int N, long HW, int Cin, int Cout,
                   int dtype, hipStream_t stream, bool dry_run) {
  if (Cin % 32 || Cout % 32 || (dtype != HDMOE_BF16 && dtype != HDMOE_F32)) return 1;
  if (((uintptr_t)x | (uintptr_t)dy) & 15) return 1;
  LwgArgs a;
  a.x = x; a.dy = dy; a.seg = seg; a.ngroups = ngroups; a.N = N; a.HW = HW; a.I = Cin; a.O = Cout; a.dy2 = nullptr; a.G2 = nullptr;
  for (int g = 0; g < HDMOE_MAX_GROUPS; ++g) a.G[g] = G[g < ngroups ? g : 0];
  const int OT = Cout % 64 == 0 ? 2 : 1, IT = Cin % 64 == 0 ? 2 : 1;
  PwsPlan p;
  if (!pws_plan(p, (long)N * HW, ngroups, Cin / (32 * IT), Cout / (32 * OT), OT, IT, dtype == HDMOE_BF16)) return 1;
  a.upw = p.upw;
  if (dry_run) return HDMOE_OK;
  conv_pick<2, 1>(OT, [&](auto Ot) { conv_pick<2, 1>(IT, [&](auto It) {
    constexpr int O = decltype(Ot)::value, I = decltype(It)::value;
    if (dtype == HDMOE_BF16) hipLaunchKernelGGL((lwg_bf16_kernel<O, I>), p.grid, dim3(256), p.lds, stream, a);
    else hipLaunchKernelGGL((lwg_f32_kernel<O, I>), p.grid, dim3(256), p.lds, stream, a);
  }); });
  return hdmoe_launch_status();
}

// Weight gradients of two pointwise bf16 layers with 32 outputs each over the same x [P][Cin] in one launch: G1 ([32][Cin] fp32) +=
// dy1^T x, G2 += dy2^T x.  The grid is the one a single such layer gets (lwg_try_launch), so every workgroup forms for each slab the
// partial sum it would form there.  Domain: bf16, Cin % 64 == 0, 16-byte aligned tensors; 1 outside it, nothing launched.
extern "C" int hdmoe_lwgrad2(const void* x, const void* dy1, const void* dy2, float* G1, float* G2, long P, int Cin, int dtype,
                             hipStream_t stream) {
  if (dtype != HDMOE_BF16 || Cin % 64 || Cin < 64) return 1;
  if (!x || !dy1 || !dy2 || !G1 || !G2 || P < 0) return HDMOE_EINVAL;
  if ((((uintptr_t)x | (uintptr_t)dy1 | (uintptr_t)dy2) & 15) || (((uintptr_t)G1 | (uintptr_t)G2) & 3) || P >= (1l << 40)) return 1;
  if (P == 0) return HDMOE_OK;
  LwgArgs a;
  a.x = x; a.dy = dy1; a.dy2 = dy2; a.seg = nullptr; a.ngroups = 1; a.N = 1; a.HW = P; a.I = Cin; a.O = 32; a.G2 = G2;
  for (int g = 0; g < HDMOE_MAX_GROUPS; ++g) a.G[g] = G1;
  PwsPlan p;                                                             // the grid of ONE such layer (OT = 1, IT = 2), both layers' tiles in LDS
  if (!pws_plan(p, P, 1, Cin / 64, 1, 2, 2, true)) return 1;
  a.upw = p.upw;
  hipLaunchKernelGGL((lwg_bf16_kernel<2, 2, true>), p.grid, dim3(256), p.lds, stream, a);
  return hdmoe_launch_status();
}
