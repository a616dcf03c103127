// Fusion stage (models/_assembly.py _fusion_tail): its token-local chains in ONE launch per chain and direction.  Three chains: the one in
// front of the first attention call (hdmoe_fusion_in_*, below), the one behind the second (hdmoe_fusion_out_*, further down) and the one
// between the two (hdmoe_fusion_mid_*, last).
// The in chain:
//   forward   t = fv - fu;  d = sw[n] * t;  query = fu + d;  ctx = fv - d;  q = Wq query;  k = Wk ctx;  v = Wv ctx
//             (sw absent -- model_config2: query = fu, ctx = fv, only the three projections)
//   backward  dquery = Wq^T dq (+ gquery);  dctx = Wk^T dk + Wv^T dv (+ gctx);  dd = dquery - dctx;  dsw[n] += <dd, t>;  dt = sw[n] * dd;
//             dfu = dquery - dt;  dfv = dctx + dt
// Unfused this is axpby, scale_rows, axpby, axpby and three pointwise convs (seven launches), and in the backward three pw_bwd launches, six
// elementwise ones and four ATen adds, every one a round trip of a (rows, 32) bf16 tensor through HBM on a stream with nothing beside it.
// Every intermediate that the unfused chain stores is rounded to bf16 at the same point here (t, d, query, ctx, each projection's output,
// each sum of two gradients); between those points the arithmetic is fp32, the formulas are those of elementwise.hip.  The one difference
// is the fp32 summation order inside a 32-term dot product.
//
// Weight gradients: the plain backward entry points form none (hdmoe_conv_wgrad's lwg_bf16_kernel can, one launch per layer, from
// query / ctx and dq / dk / dv); the _wg ones contract them from the rows the wave already holds ("weight gradients inside the backward
// kernels", below) -- what the model's step runs.
//
// Layout.  A wave owns 32 rows (tokens) at a time.  Lane (r = lane & 31, h = lane >> 5) holds of row r the channels 8h .. 8h + 7 and
// 16 + 8h .. 16 + 8h + 7: two 16-byte global accesses, and exactly the B operand of mfma_f32_32x32x16_bf16 for the two k-steps of a
// 32-deep product (common.h mma32: B[8h + j][r]).  The 32 x 32 weight tile is the A operand, rows = output channels, held in registers
// for the life of the wave, read from the weight bank's prepared images (forward [O][32], flipped [I][32]) with the same two accesses.
// The accumulator of D[o][row] gives lane (r, h) the channels 8q + 4h + j (q, j < 4) of row r: after rounding to bf16 the lane pair
// (r, 0) / (r, 1) swaps two 8-byte halves (one cross-lane exchange of four dwords, no LDS tile) and each lane again holds the row layout
// above -- ready for its 16-byte store and for the elementwise arithmetic against tensors loaded in that layout.
// Streaming kernels: the floor is bytes / HBM rate (forward reads 2 and writes 5 tensors, backward reads 6 and writes 2 with sw).
#include "common.h"
#include "conv_args.h"
#include "pw_stream.h"
#include "hdmoe.h"

namespace {

struct Row32 { bf16x8 f[2]; };                                // channels 8h .. 8h + 7 and 16 + 8h .. 16 + 8h + 7 of one row

DEVI Row32 ld_row(const bf16* p, long row, int h) {
  Row32 x;
  x.f[0] = *reinterpret_cast<const bf16x8*>(p + row * 32 + 8 * h);
  x.f[1] = *reinterpret_cast<const bf16x8*>(p + row * 32 + 16 + 8 * h);
  return x;
}
DEVI void st_row(bf16* p, long row, int h, const Row32& x) {
  *reinterpret_cast<bf16x8*>(p + row * 32 + 8 * h) = x.f[0];
  *reinterpret_cast<bf16x8*>(p + row * 32 + 16 + 8 * h) = x.f[1];
}
// D[o][row] = sum_i w[o][i] x[row][i] over the 32 channels of x for the wave's 32 rows; w: lane (r, h) holds row o = r of the weight tile
DEVI f32x16 mm32(const Row32& w, const Row32& x, f32x16 acc = (f32x16)(0.f)) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.f[0], x.f[0], acc, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(w.f[1], x.f[1], acc, 0, 0, 0);
}
// bf16(alpha * acc) in the row layout.  Every lane of the wave must call it (cross-lane exchange).
DEVI Row32 pack(const f32x16& acc, float alpha, int h) {
  // register 4 q + j: channel 8 q + 4 h + j of this lane's row (common.h acc_row)
  uint2 u[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    bf16x4 b;
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = (bf16)(alpha * acc[4 * q + j]);
    u[q] = __builtin_bit_cast(uint2, b);
  }
  // h = 0 keeps channel blocks q = 0, 2 and needs its partner's; h = 1 keeps q = 1, 3
  const uint2 s0 = h ? u[0] : u[1], s1 = h ? u[2] : u[3];
  uint2 r0, r1;
  r0.x = __shfl_xor(s0.x, 32, 64); r0.y = __shfl_xor(s0.y, 32, 64);
  r1.x = __shfl_xor(s1.x, 32, 64); r1.y = __shfl_xor(s1.y, 32, 64);
  const uint4 o0 = h ? make_uint4(r0.x, r0.y, u[1].x, u[1].y) : make_uint4(u[0].x, u[0].y, r0.x, r0.y);
  const uint4 o1 = h ? make_uint4(r1.x, r1.y, u[3].x, u[3].y) : make_uint4(u[2].x, u[2].y, r1.x, r1.y);
  Row32 y;
  y.f[0] = __builtin_bit_cast(bf16x8, o0);
  y.f[1] = __builtin_bit_cast(bf16x8, o1);
  return y;
}
// y[row][o] = bf16(alpha * sum_i w[o][i] x[row][i])
DEVI Row32 proj(const Row32& w, const Row32& x, float alpha, int h) { return pack(mm32(w, x), alpha, h); }
// the accumulator in the row layout, still fp32 (for an epilogue that reads a tensor loaded in that layout): f[8 k + j] <-> Row32 f[k][j]
DEVI void to_rows(const f32x16& acc, int h, float* f) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float r0 = __shfl_xor(h ? acc[j] : acc[4 + j], 32, 64), r1 = __shfl_xor(h ? acc[8 + j] : acc[12 + j], 32, 64);
    f[j] = h ? r0 : acc[j];          f[4 + j] = h ? acc[4 + j] : r0;
    f[8 + j] = h ? r1 : acc[8 + j];  f[12 + j] = h ? acc[12 + j] : r1;
  }
}
// bf16(a + s * b) elementwise, s = +1 / -1 (hdmoe_axpby with unit weights: one fp32 rounding whatever the arm, then the store's)
DEVI Row32 addsub(const Row32& a, const Row32& b, float s) {
  Row32 y;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) y.f[k][j] = (bf16)((float)a.f[k][j] + s * (float)b.f[k][j]);
  return y;
}
// bf16(s * a) elementwise (scale_rows_fwd_kernel)
DEVI Row32 scaled(const Row32& a, float s) {
  Row32 y;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) y.f[k][j] = (bf16)((float)a.f[k][j] * s);
  return y;
}

// ---- weight gradients inside the backward kernels (hdmoe_fusion_in_bwd_wg / hdmoe_fusion_out_bwd_wg) ------------------------------------
// dW[o][i] = sum over rows of dy[row][o] x[row][i] contracts over what the row layout puts ACROSS lanes, so both operands take the
// LDS-transpose route of pw_stream.h: the wave writes its 32 bf16 rows to a wave-private LDS tile ([32 rows][64 B], 16-byte stores) and
// fetches the MFMA fragments back with the transposing read (pws_tr8: 8 consecutive rows of channel lane & 31), two 32x32x16 steps per
// 32 x 32 weight tile and row tile; a hand-over of the tile is a pws_fence.  The 16-byte chunk c of row r sits at chunk c ^ ((r >> 1) & 3):
// unswizzled, the row-per-lane stores of eight consecutive lanes would share two 16-byte bank slots; the transposing read takes an address
// per lane, so it follows the swizzle and still covers whole 64-byte rows (conflict-free either way).  The fp32 accumulators stay in
// registers over the wave's tiles.
constexpr int WG_TILE = 2048;                                 // bytes of one operand tile
constexpr int WG_WGS = 512;                                   // default persistent grid of the _wg kernels: two workgroups per CU

struct WgFrag { bf16x8 k[2]; };                               // both k-steps (rows 0 .. 15, 16 .. 31) of one operand
DEVI int wg_off(int row, int c16) { return row * 64 + ((c16 ^ ((row >> 1) & 3)) << 4); }
DEVI void wg_put(unsigned char* tile, int r, int h, const Row32& x) {
  *reinterpret_cast<bf16x8*>(tile + wg_off(r, h)) = x.f[0];
  *reinterpret_cast<bf16x8*>(tile + wg_off(r, 2 + h)) = x.f[1];
}
DEVI WgFrag wg_get(const unsigned char* tile, int lane) {
  const int c8 = pws_tr_col(lane) >> 3;                       // 8-byte chunk: channels 4 c8 .. 4 c8 + 3
  WgFrag f;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    const int row = 16 * ks + pws_tr_row(lane);
    f.k[ks] = pws_tr8(tile + wg_off(row, c8 >> 1) + 8 * (c8 & 1), tile + wg_off(row + 4, c8 >> 1) + 8 * (c8 & 1));
  }
  return f;
}
// acc[o][i] += sum over the tile's rows of dy[row][o] x[row][i]  (o = acc_row(reg, lane), i = lane & 31)
DEVI void wg_mma(f32x16& acc, const WgFrag& dy, const WgFrag& x) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dy.k[0], x.k[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dy.k[1], x.k[1], acc, 0, 0, 0);
}
// a row past the end (a copy of the last row) as the dy operand: zero, so that it adds exactly nothing to a slab
DEVI Row32 wg_keep(const Row32& x, bool ok) {
  Row32 y = x;
  if (!ok) { y.f[0] = (bf16x8)(0); y.f[1] = (bf16x8)(0); }
  return y;
}
// End of the kernel: the four waves' accumulators of one weight tile meet in LDS in wave order (red: [4][16 regs][64 lanes] floats) and
// the workgroup adds rows o < O of the tile into G (row stride ld) once, with float atomics.  Every workgroup adds to the same words:
// each starts at another quarter (pw_stream.h pws_flush).  All threads of the workgroup must call it.
DEVI void wg_flush(const f32x16& acc, float* red, float* G, int O, int ld, int tid, unsigned rot) {
  __syncthreads();                                            // red is free: the operand tiles, or the previous tile's sums, are done with
  pws_put<1>(red, tid >> 6, tid & 63, &acc);
  __syncthreads();
  pws_flush<4, 1>(red, tid, 256, 256 * (int)(rot & 3), [&](int, int reg, int l) -> float* {
    const int o = acc_row(reg, l);
    return o < O ? &G[o * ld + (l & 31)] : nullptr;
  });
}

struct FinArgs {
  const bf16 *fu, *fv; const float* sw; const bf16 *wq, *wk, *wv;
  bf16 *query, *ctx, *q, *k, *v;
  long rows, S, tiles;
  float aq, ak, av;
};

__global__ __launch_bounds__(256) void fusion_in_fwd_kernel(FinArgs a) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  if (wave >= a.tiles) return;
  const Row32 wq = ld_row(a.wq, r, h), wk = ld_row(a.wk, r, h), wv = ld_row(a.wv, r, h);
  // rows past the end read the last row (in bounds) and are not stored
  auto rowof = [&](long t) { const long row = t * 32 + r; return row < a.rows ? row : a.rows - 1; };
  Row32 fu = ld_row(a.fu, rowof(wave), h), fv = ld_row(a.fv, rowof(wave), h);
  for (long t = wave; t < a.tiles; t += nw) {
    const long row = t * 32 + r, rr = rowof(t);
    Row32 nfu = fu, nfv = fv;
    if (t + nw < a.tiles) { nfu = ld_row(a.fu, rowof(t + nw), h); nfv = ld_row(a.fv, rowof(t + nw), h); }
    Row32 qy = fu, cx = fv;
    if (a.sw) {
      const Row32 d = scaled(addsub(fv, fu, -1.f), a.sw[rr / a.S]);
      qy = addsub(fu, d, 1.f);
      cx = addsub(fv, d, -1.f);
    }
    const Row32 q = proj(wq, qy, a.aq, h), k = proj(wk, cx, a.ak, h), v = proj(wv, cx, a.av, h);
    if (row < a.rows) {
      if (a.sw) { st_row(a.query, row, h, qy); st_row(a.ctx, row, h, cx); }
      st_row(a.q, row, h, q); st_row(a.k, row, h, k); st_row(a.v, row, h, v);
    }
    fu = nfu; fv = nfv;
  }
}

struct FinBwdArgs {
  const bf16 *dq, *dk, *dv, *gquery, *gctx, *fu, *fv; const float* sw; const bf16 *wdq, *wdk, *wdv;
  bf16 *dfu, *dfv; float* dsw;
  float *Gq, *Gk, *Gv;                                          // WG only
  long rows, S, tiles;
  float aq, ak, av;
};

// WG: also the three weight gradients (above), Gq += dq^T query, Gk += dk^T ctx, Gv += dv^T ctx, query / ctx as the forward forms them
template <bool WG>
__global__ __launch_bounds__(256, WG ? 2 : 1) void fusion_in_bwd_kernel(FinBwdArgs a) {
  __shared__ float sm_v[4];
  __shared__ long sm_n[4];
  extern __shared__ __attribute__((aligned(1024))) unsigned char wg_lds[];   // WG: [4 waves][dq, dk, dv, query, ctx] tiles, then the flush's sums
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, w = threadIdx.x >> 6;
  f32x16 gacc[WG ? 3 : 1];
#pragma unroll
  for (int i = 0; i < (WG ? 3 : 1); ++i) gacc[i] = (f32x16)(0.f);
  const long wave = (long)blockIdx.x * 4 + w, nw = (long)gridDim.x * 4;
  const Row32 wq = ld_row(a.wdq, r, h), wk = ld_row(a.wdk, r, h), wv = ld_row(a.wdv, r, h);
  auto rowof = [&](long t) { const long row = t * 32 + r; return row < a.rows ? row : a.rows - 1; };
  Row32 dq = ld_row(a.dq, rowof(wave), h), dk = ld_row(a.dk, rowof(wave), h), dv = ld_row(a.dv, rowof(wave), h);
  Row32 pfu = {}, pfv = {};                                    // (WG) fu and fv travel with them: at two waves per SIMD little else hides a load
  if constexpr (WG) { pfu = ld_row(a.fu, rowof(wave), h); pfv = ld_row(a.fv, rowof(wave), h); }
  // the four waves of a workgroup take four consecutive tiles per trip and make the same number of trips (they meet at the dsw flush);
  // a wave whose tile lies past the end sits the trip out
  for (long t = wave; t - w < a.tiles; t += nw) {
    long flush_n = -1;
    float flush_v = 0.f;
    if (t < a.tiles) {
      const long row = t * 32 + r, rr = rowof(t);
      const bool ok = row < a.rows;
      Row32 ndq = dq, ndk = dk, ndv = dv;
      Row32 nfu = pfu, nfv = pfv;
      if (t + nw < a.tiles) {
        const long nr = rowof(t + nw);
        ndq = ld_row(a.dq, nr, h); ndk = ld_row(a.dk, nr, h); ndv = ld_row(a.dv, nr, h);
        if constexpr (WG) { nfu = ld_row(a.fu, nr, h); nfv = ld_row(a.fv, nr, h); }
      }
      Row32 qy = {}, cx = {};                                  // (WG) fu and fv
      if constexpr (WG) {
        // the weight gradients first: their operands are the prefetched dq, dk, dv and the forward's query and ctx, none is needed below
        qy = pfu; cx = pfv;
        Row32 xq = qy, xc = cx;
        if (a.sw) {
          const Row32 d = scaled(addsub(cx, qy, -1.f), a.sw[rr / a.S]);
          xq = addsub(qy, d, 1.f);
          xc = addsub(cx, d, -1.f);
        }
        unsigned char* mine = wg_lds + w * 5 * WG_TILE;
        pws_fence();                                            // (the previous tile's reads)
        wg_put(mine, r, h, wg_keep(dq, ok)); wg_put(mine + WG_TILE, r, h, wg_keep(dk, ok)); wg_put(mine + 2 * WG_TILE, r, h, wg_keep(dv, ok));
        wg_put(mine + 3 * WG_TILE, r, h, xq); wg_put(mine + 4 * WG_TILE, r, h, xc);
        pws_fence();
        const WgFrag fq = wg_get(mine + 3 * WG_TILE, lane), fc = wg_get(mine + 4 * WG_TILE, lane);
        wg_mma(gacc[0], wg_get(mine, lane), fq);
        wg_mma(gacc[1], wg_get(mine + WG_TILE, lane), fc);
        wg_mma(gacc[2], wg_get(mine + 2 * WG_TILE, lane), fc);
      }
      // the gradient fan-in of query (q_proj and the residual of out_proj) and of ctx (k_proj and v_proj), summed as autograd sums them:
      // two bf16 tensors at a time
      Row32 dquery = proj(wq, dq, a.aq, h);
      if (a.gquery) dquery = addsub(dquery, ld_row(a.gquery, rr, h), 1.f);
      Row32 dctx = addsub(proj(wk, dk, a.ak, h), proj(wv, dv, a.av, h), 1.f);
      if (a.gctx) dctx = addsub(dctx, ld_row(a.gctx, rr, h), 1.f);
      Row32 dfu = dquery, dfv = dctx;
      if (a.sw) {
        const long n = rr / a.S;
        const Row32 fu = WG ? qy : ld_row(a.fu, rr, h), fv = WG ? cx : ld_row(a.fv, rr, h);
        const Row32 tt = addsub(fv, fu, -1.f);                 // t = fv - fu, as the forward rounded it
        const Row32 dd = addsub(dquery, dctx, -1.f);
        float part = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
          for (int j = 0; j < 8; ++j) part += (float)dd.f[k][j] * (float)tt.f[k][j];
        if (!ok) part = 0.f;
        const Row32 dt = scaled(dd, a.sw[n]);
        dfu = addsub(dquery, dt, -1.f);
        dfv = addsub(dctx, dt, 1.f);
        // dsw[n] += <dd, t> over the sample's rows, fp32.  A tile inside one sample hands its sum to the workgroup's flush below;
        // a tile that a sample boundary crosses adds per row
        const long last = t * 32 + 31 < a.rows ? t * 32 + 31 : a.rows - 1;
        if ((t * 32) / a.S == last / a.S) {
          flush_v = wave_sum(part);
          flush_n = (t * 32) / a.S;
        } else {
          part += __shfl_xor(part, 32, 64);
          if (h == 0 && ok) atomicAdd(&a.dsw[n], part);
        }
      }
      if (ok) { st_row(a.dfu, row, h, dfu); st_row(a.dfv, row, h, dfv); }
      dq = ndq; dk = ndk; dv = ndv; pfu = nfu; pfv = nfv;
    }
    if (a.sw) {
      // one atomic per workgroup, trip and sample (scale_rows_bwd_kernel: one per workgroup): the waves' sums of the same sample are
      // added in wave order first
      if (lane == 0) { sm_v[w] = flush_v; sm_n[w] = flush_n; }
      __syncthreads();
      if (threadIdx.x == 0) {
        long cn = -1;
        float cv = 0.f;
        for (int i = 0; i < 4; ++i) {
          if (sm_n[i] < 0) continue;
          if (sm_n[i] != cn) {
            if (cn >= 0) atomicAdd(&a.dsw[cn], cv);
            cn = sm_n[i]; cv = sm_v[i];
          } else cv += sm_v[i];
        }
        if (cn >= 0) atomicAdd(&a.dsw[cn], cv);
      }
      __syncthreads();
    }
  }
  if constexpr (WG) {
    float* red = reinterpret_cast<float*>(wg_lds);
    wg_flush(gacc[0], red, a.Gq, 32, 32, threadIdx.x, blockIdx.x);
    wg_flush(gacc[1], red, a.Gk, 32, 32, threadIdx.x, blockIdx.x + 1);
    wg_flush(gacc[2], red, a.Gv, 32, 32, threadIdx.x, blockIdx.x + 2);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The chain behind the text attention, down to the gate (models/_assembly.py _fusion_tail):
//   at = ao Wo o2 + bo a (out_proj of cross_attn_text with its residual);  a2 = a + alpha_txt (at - a);  cat = [wa U | wb a2];
//   g1 = a1 W1 cat;  s = mp_silu(g1);  l = a2g W2 s (2 logits);  g = softmax(l);  mixed = k (U + g0 U + g1 a2)
// unfused: conv with residual epilogue, lerp_param, cat2, conv, mp_silu, conv, gate_mix (seven launches).  The forward also writes what
// the backward reads and cannot cheaply recompute, a2 and g1, and -- only when asked, for a caller that runs weight-only gradient launches
// -- cat and s as the `x` of gate1's and gate2's weight gradient (the _wg backward recomputes both from U, a2, g1).  at is recomputed in
// the backward from o2 (two MFMAs) instead of being stored.
struct FoutArgs {
  const bf16 *o2, *a, *U; const float* alpha_txt; const bf16 *wo, *w1, *w2;
  bf16 *mixed, *a2, *g1, *cat, *s; float* gate;
  long rows, tiles;
  float ao, bo, wa, wb, a1, a2g;
};
#define GATE_K 0.70710678118654752f                            /* 0.5 / sqrt(0.5), gate_mix_fwd_kernel */

// at = bf16(ao * acc + bo * a) in the row layout (the conv kernels' epilogue: v = alpha * acc; v += beta * res)
DEVI Row32 out_res(const f32x16& acc, const Row32& a, float ao, float bo, int h) {
#pragma clang fp contract(off)
  float f[16];
  to_rows(acc, h, f);
  Row32 y;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // spelled out so that no compiler chooses which product is folded: the epilogue's residual term is added inside a branch there,
      // so alpha * acc is rounded on its own and beta * res is the fused product
      const float v = ao * f[8 * k + j];
      y.f[k][j] = (bf16)__builtin_fmaf(bo, (float)a.f[k][j], v);
    }
  return y;
}

__global__ __launch_bounds__(256) void fusion_out_fwd_kernel(FoutArgs a) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  if (wave >= a.tiles) return;
  const Row32 wo = ld_row(a.wo, r, h);
  // gate1 [32][64]: the U half and the a2 half of a row as two tiles; gate2 [2][32]: rows 2 .. 31 of its tile are zero
  Row32 w1u, w1a, w2;
  w1u.f[0] = *reinterpret_cast<const bf16x8*>(a.w1 + r * 64 + 8 * h);       w1u.f[1] = *reinterpret_cast<const bf16x8*>(a.w1 + r * 64 + 16 + 8 * h);
  w1a.f[0] = *reinterpret_cast<const bf16x8*>(a.w1 + r * 64 + 32 + 8 * h);  w1a.f[1] = *reinterpret_cast<const bf16x8*>(a.w1 + r * 64 + 48 + 8 * h);
  w2 = ld_row(a.w2, r < 2 ? r : 0, h);
  if (r >= 2) { w2.f[0] = (bf16x8)(0); w2.f[1] = (bf16x8)(0); }
  const float al = *a.alpha_txt;
  for (long t = wave; t < a.tiles; t += nw) {
    const long row = t * 32 + r, rr = row < a.rows ? row : a.rows - 1;
    const Row32 o2 = ld_row(a.o2, rr, h), av = ld_row(a.a, rr, h), U = ld_row(a.U, rr, h);
    const Row32 at = out_res(mm32(wo, o2), av, a.ao, a.bo, h);
    Row32 a2, cu, ca;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = (float)av.f[k][j];
        a2.f[k][j] = (bf16)(x + al * ((float)at.f[k][j] - x));                 // lerp_param_fwd_kernel
        cu.f[k][j] = (bf16)((float)U.f[k][j] * a.wa);                           // cat2_fwd_kernel
        ca.f[k][j] = (bf16)((float)a2.f[k][j] * a.wb);
      }
    const Row32 g1 = pack(mm32(w1a, ca, mm32(w1u, cu)), a.a1, h);
    Row32 s;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) s.f[k][j] = (bf16)mp_silu_f((float)g1.f[k][j]);
    const f32x16 lacc = mm32(w2, s);                           // logits 0, 1 of row r: registers 0, 1 of lane (r, 0)
    const float l0 = __shfl((float)(bf16)(a.a2g * lacc[0]), r, 64), l1 = __shfl((float)(bf16)(a.a2g * lacc[1]), r, 64);
    const float m = fmaxf(l0, l1);
    const float e0 = __expf(l0 - m), e1 = __expf(l1 - m);
    const float g0 = e0 / (e0 + e1), gg1 = e1 / (e0 + e1);
    Row32 mixed;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float u = (float)U.f[k][j], x = (float)a2.f[k][j];
        mixed.f[k][j] = (bf16)(GATE_K * (u + g0 * u + gg1 * x));                // gate_mix_fwd_kernel
      }
    if (row < a.rows) {
      st_row(a.mixed, row, h, mixed);
      if (a.a2) {                                              // (NULL together: a forward that no backward follows)
        st_row(a.a2, row, h, a2); st_row(a.g1, row, h, g1);
      }
      if (a.cat) {                                             // (NULL together: the backward recomputes them, hdmoe_fusion_out_bwd_wg)
        st_row(a.s, row, h, s);
        *reinterpret_cast<bf16x8*>(a.cat + row * 64 + 8 * h) = cu.f[0];       *reinterpret_cast<bf16x8*>(a.cat + row * 64 + 16 + 8 * h) = cu.f[1];
        *reinterpret_cast<bf16x8*>(a.cat + row * 64 + 32 + 8 * h) = ca.f[0];  *reinterpret_cast<bf16x8*>(a.cat + row * 64 + 48 + 8 * h) = ca.f[1];
      }
      if (h == 0) *reinterpret_cast<float2*>(a.gate + 2 * row) = make_float2(g0, gg1);
    }
  }
}

// Backward of that chain, input gradients and elementwise backward only:
//   gate_mix backward -> dU', dA', dl;  ds = a2g W2^T dl;  dg1 = ds mp_silu'(g1);  dcat = a1 W1^T dg1;  dU = dU' + wa dcat[:32];
//   da2 = dA' + wb dcat[32:];  dat = alpha_txt da2;  dalpha += <da2, at - a>;  do2 = ao Wo^T dat;  da = (1 - alpha_txt) da2 + bo dat
// and dat, dg1, dl written as the `dy` of the three weight gradients.  Every sum of two gradients that autograd forms between the
// unfused ops is formed here, rounded to bf16 as there.
struct FoutBwdArgs {
  const bf16 *dmixed; const float *dgate, *gate; const bf16 *U, *a2, *g1, *o2, *a; const float* alpha_txt;
  const bf16 *wo, *wdo, *wd1, *wd2;
  bf16 *do2, *da, *dU, *dat, *dg1, *dl; float* dalpha;
  float *Go, *G1, *G2;                                          // WG only (dat, dg1, dl are then not written)
  long rows, tiles;
  float ao, bo, wa, wb, a1, a2g;
};

// WG: also the three weight gradients, Go += dat^T o2, G1 += dg1^T [cu | ca], G2 += dl^T s, with cat = [cu | ca] and s recomputed from U,
// a2 and g1 as the forward forms them; gate2's two output channels are rows 0, 1 of a tile whose other rows stay zero (its forward's trick)
template <bool WG>
__global__ __launch_bounds__(256, WG ? 2 : 1) void fusion_out_bwd_kernel(FoutBwdArgs a) {
  __shared__ float sm[16];
  extern __shared__ __attribute__((aligned(1024))) unsigned char wg_lds[];   // WG: [4 waves][dat, o2, dg1, cu, ca, dl, s] tiles, then the flush's sums
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  unsigned char* mine = wg_lds + (threadIdx.x >> 6) * 7 * WG_TILE;
  f32x16 gacc[WG ? 4 : 1];                                      // out_proj, gate1's U half, gate1's a2 half, gate2
#pragma unroll
  for (int i = 0; i < (WG ? 4 : 1); ++i) gacc[i] = (f32x16)(0.f);
  if constexpr (WG) wg_put(mine + 5 * WG_TILE, r, h, wg_keep(Row32{}, false));   // the dl tile: only channels 0, 1 are ever written again
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  const Row32 wo = ld_row(a.wo, r, h), wdo = ld_row(a.wdo, r, h);
  const Row32 wd1u = ld_row(a.wd1, r, h), wd1a = ld_row(a.wd1, 32 + r, h);      // flipped gate1 image [64][32]: input channels 0 .. 31 / 32 .. 63
  const bf16x8 wd2 = *reinterpret_cast<const bf16x8*>(a.wd2 + r * 16 + 8 * h);  // flipped gate2 image [32][16]: columns 2 .. 15 are zero
  const float al = *a.alpha_txt;
  float dal = 0.f;
  for (long t = wave; t < a.tiles; t += nw) {
    const long row = t * 32 + r, rr = row < a.rows ? row : a.rows - 1;
    const bool ok = row < a.rows;
    const Row32 dm = ld_row(a.dmixed, rr, h), U = ld_row(a.U, rr, h), a2 = ld_row(a.a2, rr, h);
    const float g0 = a.gate[2 * rr], gg1 = a.gate[2 * rr + 1];
    // (WG) every operand of the weight gradients goes to its LDS tile where it is formed, so that none stays in registers for it
    if constexpr (WG) {
      Row32 cu, ca;
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          cu.f[k][j] = (bf16)((float)U.f[k][j] * a.wa);                                                         // cat2_fwd_kernel
          ca.f[k][j] = (bf16)((float)a2.f[k][j] * a.wb);
        }
      pws_fence();                                              // (the previous tile's reads)
      wg_put(mine + 3 * WG_TILE, r, h, cu); wg_put(mine + 4 * WG_TILE, r, h, ca);
    }
    // gate_mix_bwd_vec_kernel
    // (the two row sums in that kernel's order: four partial sums over 8 consecutive channels each, p0 .. p3, met as (p0 + p2) + (p1 + p3);
    //  this lane holds p_h and p_{2 + h})
    Row32 dUm, dAm;
    float p0[2] = {0.f, 0.f}, p1[2] = {0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float go = (float)dm.f[k][j] * GATE_K;
        p0[k] += go * (float)U.f[k][j]; p1[k] += go * (float)a2.f[k][j];
        dUm.f[k][j] = (bf16)(go * (1.f + g0)); dAm.f[k][j] = (bf16)(go * gg1);
      }
    float d0 = p0[0] + p0[1], d1 = p1[0] + p1[1];
    d0 += __shfl_xor(d0, 32, 64); d1 += __shfl_xor(d1, 32, 64);
    if (a.dgate) { d0 += a.dgate[2 * rr]; d1 += a.dgate[2 * rr + 1]; }
    const float dot = d0 * g0 + d1 * gg1;
    const bf16 dl0 = (bf16)(g0 * (d0 - dot)), dl1 = (bf16)(gg1 * (d1 - dot));
    // gate2 input gradient: one 16-deep MFMA step over the (padded) output channels, dl in k-slots 0, 1 of the h = 0 lanes
    bf16x8 dlf = (bf16x8)(0);
    if (h == 0) { dlf[0] = dl0; dlf[1] = dl1; }
    const Row32 ds = pack(__builtin_amdgcn_mfma_f32_32x32x16_bf16(wd2, dlf, (f32x16)(0.f), 0, 0, 0), a.a2g, h);
    const Row32 g1 = ld_row(a.g1, rr, h);
    Row32 dg1;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) dg1.f[k][j] = (bf16)((float)ds.f[k][j] * mp_silu_grad_f((float)g1.f[k][j]));   // mp_silu_bwd_kernel (g * grad)
    if constexpr (WG) {
      Row32 s;
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) s.f[k][j] = (bf16)mp_silu_f((float)g1.f[k][j]);                                // mp_silu_fwd_kernel
      wg_put(mine + 2 * WG_TILE, r, h, wg_keep(dg1, ok));
      if (h == 0) {
        bf16x2 d; d[0] = ok ? dl0 : (bf16)0.f; d[1] = ok ? dl1 : (bf16)0.f;
        *reinterpret_cast<bf16x2*>(mine + 5 * WG_TILE + wg_off(r, 0)) = d;
      }
      wg_put(mine + 6 * WG_TILE, r, h, s);
      pws_fence();
      const WgFrag fg = wg_get(mine + 2 * WG_TILE, lane);
      wg_mma(gacc[1], fg, wg_get(mine + 3 * WG_TILE, lane));
      wg_mma(gacc[2], fg, wg_get(mine + 4 * WG_TILE, lane));
      wg_mma(gacc[3], wg_get(mine + 5 * WG_TILE, lane), wg_get(mine + 6 * WG_TILE, lane));
    }
    const Row32 dcu = proj(wd1u, dg1, a.a1, h), dca = proj(wd1a, dg1, a.a1, h);
    Row32 dU, da2;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bf16 cu = (bf16)((float)dcu.f[k][j] * a.wa), ca = (bf16)((float)dca.f[k][j] * a.wb);             // cat2_bwd_kernel
        dU.f[k][j] = (bf16)((float)dUm.f[k][j] + (float)cu);                                                    // fan-in of out_u from gate_mix and cat
        da2.f[k][j] = (bf16)((float)dAm.f[k][j] + (float)ca);                                                   // fan-in of a2
      }
    const Row32 o2 = ld_row(a.o2, rr, h), av = ld_row(a.a, rr, h);
    const Row32 at = out_res(mm32(wo, o2), av, a.ao, a.bo, h);
    Row32 dat, dal_;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = (float)da2.f[k][j];
        dal_.f[k][j] = (bf16)((1.f - al) * g);                                                                  // lerp_param_bwd_kernel
        dat.f[k][j] = (bf16)(al * g);
        if (ok) dal += g * ((float)at.f[k][j] - (float)av.f[k][j]);
      }
    if constexpr (WG) {
      wg_put(mine, r, h, wg_keep(dat, ok)); wg_put(mine + WG_TILE, r, h, o2);
      pws_fence();
      wg_mma(gacc[0], wg_get(mine, lane), wg_get(mine + WG_TILE, lane));
    }
    const Row32 do2 = proj(wdo, dat, a.ao, h);
    Row32 da;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) da.f[k][j] = (bf16)((float)dal_.f[k][j] + (float)(bf16)(a.bo * (float)dat.f[k][j]));   // lerp share + the residual's share
    if (ok) {
      st_row(a.do2, row, h, do2); st_row(a.da, row, h, da); st_row(a.dU, row, h, dU);
      if constexpr (!WG) {
        st_row(a.dat, row, h, dat); st_row(a.dg1, row, h, dg1);
        if (h == 0) { bf16x2 d; d[0] = dl0; d[1] = dl1; *reinterpret_cast<bf16x2*>(a.dl + 2 * row) = d; }
      }
    }
  }
  // dalpha: fp32, one flush per workgroup (lerp_param_bwd_kernel)
  dal = block_sum(dal, sm);
  if (threadIdx.x == 0) atomicAdd(a.dalpha, dal);
  if constexpr (WG) {
    float* red = reinterpret_cast<float*>(wg_lds);
    wg_flush(gacc[0], red, a.Go, 32, 32, threadIdx.x, blockIdx.x);
    wg_flush(gacc[1], red, a.G1, 32, 64, threadIdx.x, blockIdx.x + 1);
    wg_flush(gacc[2], red, a.G1 + 32, 32, 64, threadIdx.x, blockIdx.x + 2);
    wg_flush(gacc[3], red, a.G2, 2, 32, threadIdx.x, blockIdx.x + 3);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The chain between the two attention cores (models/_assembly.py _fusion_tail): out_proj of cross_attn with its residual, then q_proj of
// cross_attn_text.
//   forward   a = ao Wo o1 + bo query (the conv epilogue's rounding, out_res);  q2 = aq Wq a, from the bf16 a
//   backward  dq2x = aq Wq^T dq2;  da_t = da + dq2x (the gradient fan-in of a: fusion_out_bwd's da and q_proj's);  do1 = ao Wo^T da_t;
//             dres = bo da_t (the residual's share of query's gradient);  Gq += dq2^T a;  Go += da_t^T o1
// unfused: two conv launches forward; pw_bwd, an ATen bf16 add, pw_bwd and axpby backward, each rounding to bf16 where it stores.
struct FmidArgs {
  const bf16 *o1, *query, *wo, *wq; bf16 *a, *q2;
  long rows, tiles;
  float ao, bo, aq;
};

__global__ __launch_bounds__(256) void fusion_mid_fwd_kernel(FmidArgs a) {
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  if (wave >= a.tiles) return;
  const Row32 wo = ld_row(a.wo, r, h), wq = ld_row(a.wq, r, h);
  auto rowof = [&](long t) { const long row = t * 32 + r; return row < a.rows ? row : a.rows - 1; };
  Row32 o1 = ld_row(a.o1, rowof(wave), h), qy = ld_row(a.query, rowof(wave), h);
  for (long t = wave; t < a.tiles; t += nw) {
    const long row = t * 32 + r;
    Row32 no1 = o1, nqy = qy;
    if (t + nw < a.tiles) { no1 = ld_row(a.o1, rowof(t + nw), h); nqy = ld_row(a.query, rowof(t + nw), h); }
    const Row32 av = out_res(mm32(wo, o1), qy, a.ao, a.bo, h);
    const Row32 q2 = proj(wq, av, a.aq, h);
    if (row < a.rows) { st_row(a.a, row, h, av); st_row(a.q2, row, h, q2); }
    o1 = no1; qy = nqy;
  }
}

struct FmidBwdArgs {
  const bf16 *da, *dq2, *a, *o1, *wdo, *wdq; bf16 *do1, *dres;
  float *Go, *Gq;                                               // WG only
  long rows, tiles;
  float ao, bo, aq;
};

template <bool WG>
__global__ __launch_bounds__(256, WG ? 2 : 1) void fusion_mid_bwd_kernel(FmidBwdArgs a) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char wg_lds[];   // WG: [4 waves][dq2, a, da_t, o1] tiles, then the flush's sums
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (long)gridDim.x * 4;
  unsigned char* mine = wg_lds + (threadIdx.x >> 6) * 4 * WG_TILE;
  const Row32 wdo = ld_row(a.wdo, r, h), wdq = ld_row(a.wdq, r, h);
  f32x16 gacc[WG ? 2 : 1];
#pragma unroll
  for (int i = 0; i < (WG ? 2 : 1); ++i) gacc[i] = (f32x16)(0.f);
  auto rowof = [&](long t) { const long row = t * 32 + r; return row < a.rows ? row : a.rows - 1; };
  Row32 dq2 = {}, da = {}, av = {}, o1 = {};
  if (wave < a.tiles) {
    dq2 = ld_row(a.dq2, rowof(wave), h); da = ld_row(a.da, rowof(wave), h);
    if constexpr (WG) { av = ld_row(a.a, rowof(wave), h); o1 = ld_row(a.o1, rowof(wave), h); }
  }
  for (long t = wave; t < a.tiles; t += nw) {
    const long row = t * 32 + r;
    const bool ok = row < a.rows;
    Row32 ndq2 = dq2, nda = da, nav = av, no1 = o1;           // the next tile's rows, in flight over this tile's arithmetic
    if (t + nw < a.tiles) {
      const long nr = rowof(t + nw);
      ndq2 = ld_row(a.dq2, nr, h); nda = ld_row(a.da, nr, h);
      if constexpr (WG) { nav = ld_row(a.a, nr, h); no1 = ld_row(a.o1, nr, h); }
    }
    if constexpr (WG) {
      pws_fence();                                              // (the previous tile's reads)
      wg_put(mine, r, h, wg_keep(dq2, ok)); wg_put(mine + WG_TILE, r, h, av);
      wg_put(mine + 3 * WG_TILE, r, h, o1);
    }
    const Row32 dat = addsub(da, proj(wdq, dq2, a.aq, h), 1.f);
    const Row32 do1 = proj(wdo, dat, a.ao, h), dres = scaled(dat, a.bo);
    if (ok) { st_row(a.do1, row, h, do1); st_row(a.dres, row, h, dres); }
    if constexpr (WG) {
      wg_put(mine + 2 * WG_TILE, r, h, wg_keep(dat, ok));
      pws_fence();
      wg_mma(gacc[0], wg_get(mine, lane), wg_get(mine + WG_TILE, lane));
      wg_mma(gacc[1], wg_get(mine + 2 * WG_TILE, lane), wg_get(mine + 3 * WG_TILE, lane));
    }
    dq2 = ndq2; da = nda; av = nav; o1 = no1;
  }
  if constexpr (WG) {
    float* red = reinterpret_cast<float*>(wg_lds);
    wg_flush(gacc[0], red, a.Gq, 32, 32, threadIdx.x, blockIdx.x);
    wg_flush(gacc[1], red, a.Go, 32, 32, threadIdx.x, blockIdx.x + 1);
  }
}

static inline bool mis16(const void* p) { return ((uintptr_t)p & 15) != 0; }
// persistent grid: four waves per workgroup, a wave per 32-row tile up to eight workgroups per CU's worth, then grid-stride
static inline unsigned fusion_grid(long tiles) {
  long b = (tiles + 3) / 4;
  return (unsigned)(b > 2048 ? 2048 : b);
}
// the _wg kernels: every workgroup ends with a flush of the same slab words, so a few workgroups per CU and grid-stride from there
static inline unsigned wg_grid(long tiles, int max_wg) {
  const long b = (tiles + 3) / 4, cap = max_wg > 0 ? max_wg : WG_WGS;
  return (unsigned)(b > cap ? cap : b);
}

}  // namespace

extern "C" int hdmoe_fusion_in_fwd(const void* fu, const void* fv, const float* sw, const void* wq, const void* wk, const void* wv,
                                   void* query, void* ctx, void* q, void* k, void* v, long rows, long S, int C, float alpha_q,
                                   float alpha_k, float alpha_v, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || C != 32) return 1;
  if (!fu || !fv || !wq || !wk || !wv || !q || !k || !v || rows < 0 || (sw && (!query || !ctx || S < 1))) return HDMOE_EINVAL;
  if (mis16(fu) || mis16(fv) || mis16(wq) || mis16(wk) || mis16(wv) || mis16(query) || mis16(ctx) || mis16(q) || mis16(k) || mis16(v) ||
      ((uintptr_t)sw & 3) || rows >= (1l << 40)) return 1;
  if (rows == 0) return HDMOE_OK;
  FinArgs a;
  a.fu = (const bf16*)fu; a.fv = (const bf16*)fv; a.sw = sw; a.wq = (const bf16*)wq; a.wk = (const bf16*)wk; a.wv = (const bf16*)wv;
  a.query = (bf16*)query; a.ctx = (bf16*)ctx; a.q = (bf16*)q; a.k = (bf16*)k; a.v = (bf16*)v;
  a.rows = rows; a.S = S < 1 ? 1 : S; a.tiles = (rows + 31) / 32; a.aq = alpha_q; a.ak = alpha_k; a.av = alpha_v;
  hdmoe_count_selection(HDMOE_SEL_FUSION_IN);
  hipLaunchKernelGGL(fusion_in_fwd_kernel, dim3(fusion_grid(a.tiles)), dim3(256), 0, stream, a);
  return hdmoe_launch_status();
}

// both forms of the in chain's backward.  G != null: the _wg form on a persistent grid of at most max_wg workgroups (0: WG_WGS).
static int fusion_in_bwd_launch(const void* dq, const void* dk, const void* dv, const void* gquery, const void* gctx, const void* fu,
                                const void* fv, const float* sw, const void* wdq, const void* wdk, const void* wdv, void* dfu, void* dfv,
                                float* dsw, float* const* G, int max_wg, long rows, long S, int C, float alpha_q, float alpha_k,
                                float alpha_v, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || C != 32) return 1;
  if (!dq || !dk || !dv || !wdq || !wdk || !wdv || !dfu || !dfv || rows < 0 || (sw && (!fu || !fv || !dsw || S < 1))) return HDMOE_EINVAL;
  if (G && (!G[0] || !G[1] || !G[2] || !fu || !fv || max_wg < 0)) return HDMOE_EINVAL;
  if (mis16(dq) || mis16(dk) || mis16(dv) || mis16(gquery) || mis16(gctx) || mis16(fu) || mis16(fv) || mis16(wdq) || mis16(wdk) ||
      mis16(wdv) || mis16(dfu) || mis16(dfv) || (((uintptr_t)sw | (uintptr_t)dsw) & 3) || rows >= (1l << 40)) return 1;
  if (G && (((uintptr_t)G[0] | (uintptr_t)G[1] | (uintptr_t)G[2]) & 3)) return 1;
  if (rows == 0) return HDMOE_OK;
  FinBwdArgs a;
  a.dq = (const bf16*)dq; a.dk = (const bf16*)dk; a.dv = (const bf16*)dv; a.gquery = (const bf16*)gquery; a.gctx = (const bf16*)gctx;
  a.fu = (const bf16*)fu; a.fv = (const bf16*)fv; a.sw = sw; a.wdq = (const bf16*)wdq; a.wdk = (const bf16*)wdk; a.wdv = (const bf16*)wdv;
  a.dfu = (bf16*)dfu; a.dfv = (bf16*)dfv; a.dsw = dsw;
  a.Gq = G ? G[0] : nullptr; a.Gk = G ? G[1] : nullptr; a.Gv = G ? G[2] : nullptr;
  a.rows = rows; a.S = S < 1 ? 1 : S; a.tiles = (rows + 31) / 32; a.aq = alpha_q; a.ak = alpha_k; a.av = alpha_v;
  hdmoe_count_selection(HDMOE_SEL_FUSION_IN_BWD);
  if (G) hipLaunchKernelGGL(fusion_in_bwd_kernel<true>, dim3(wg_grid(a.tiles, max_wg)), dim3(256), 4 * 5 * WG_TILE, stream, a);
  else hipLaunchKernelGGL(fusion_in_bwd_kernel<false>, dim3(fusion_grid(a.tiles)), dim3(256), 0, stream, a);
  return hdmoe_launch_status();
}

extern "C" int hdmoe_fusion_in_bwd(const void* dq, const void* dk, const void* dv, const void* gquery, const void* gctx, const void* fu,
                                   const void* fv, const float* sw, const void* wdq, const void* wdk, const void* wdv, void* dfu, void* dfv,
                                   float* dsw, long rows, long S, int C, float alpha_q, float alpha_k, float alpha_v, int dtype,
                                   hipStream_t stream) {
  return fusion_in_bwd_launch(dq, dk, dv, gquery, gctx, fu, fv, sw, wdq, wdk, wdv, dfu, dfv, dsw, nullptr, 0, rows, S, C, alpha_q, alpha_k,
                              alpha_v, dtype, stream);
}

extern "C" int hdmoe_fusion_in_bwd_wg(const void* dq, const void* dk, const void* dv, const void* gquery, const void* gctx, const void* fu,
                                      const void* fv, const float* sw, const void* wdq, const void* wdk, const void* wdv, void* dfu,
                                      void* dfv, float* dsw, float* Gq, float* Gk, float* Gv, int max_wg, long rows, long S, int C,
                                      float alpha_q, float alpha_k, float alpha_v, int dtype, hipStream_t stream) {
  float* const G[3] = {Gq, Gk, Gv};
  return fusion_in_bwd_launch(dq, dk, dv, gquery, gctx, fu, fv, sw, wdq, wdk, wdv, dfu, dfv, dsw, G, max_wg, rows, S, C, alpha_q, alpha_k,
                              alpha_v, dtype, stream);
}

extern "C" int hdmoe_fusion_out_fwd(const void* o2, const void* a, const void* U, const float* alpha_txt, const void* wo, const void* w1,
                                    const void* w2, void* mixed, float* gate, void* a2, void* g1, void* cat, void* s, long rows, int C,
                                    float alpha_o, float beta_o, float wa, float wb, float alpha_1, float alpha_2, int dtype,
                                    hipStream_t stream) {
  if (dtype != HDMOE_BF16 || C != 32) return 1;
  if (!o2 || !a || !U || !alpha_txt || !wo || !w1 || !w2 || !mixed || !gate || rows < 0) return HDMOE_EINVAL;
  // the saved tensors: all four, none, or a2 and g1 alone (cat and s are then the backward's to recompute)
  if ((!a2) != (!g1) || (!cat) != (!s) || (cat && !a2)) return HDMOE_EINVAL;
  if (mis16(o2) || mis16(a) || mis16(U) || mis16(wo) || mis16(w1) || mis16(w2) || mis16(mixed) || mis16(a2) || mis16(g1) || mis16(cat) ||
      mis16(s) || ((uintptr_t)gate & 7) || ((uintptr_t)alpha_txt & 3) || rows >= (1l << 40)) return 1;
  if (rows == 0) return HDMOE_OK;
  FoutArgs k;
  k.o2 = (const bf16*)o2; k.a = (const bf16*)a; k.U = (const bf16*)U; k.alpha_txt = alpha_txt; k.wo = (const bf16*)wo; k.w1 = (const bf16*)w1;
  k.w2 = (const bf16*)w2; k.mixed = (bf16*)mixed; k.gate = gate; k.a2 = (bf16*)a2; k.g1 = (bf16*)g1; k.cat = (bf16*)cat; k.s = (bf16*)s;
  k.rows = rows; k.tiles = (rows + 31) / 32; k.ao = alpha_o; k.bo = beta_o; k.wa = wa; k.wb = wb; k.a1 = alpha_1; k.a2g = alpha_2;
  hdmoe_count_selection(HDMOE_SEL_FUSION_OUT);
  hipLaunchKernelGGL(fusion_out_fwd_kernel, dim3(fusion_grid(k.tiles)), dim3(256), 0, stream, k);
  return hdmoe_launch_status();
}

// both forms of the out chain's backward.  G != null: the _wg form (dat, dg1, dl unused) on at most max_wg workgroups (0: WG_WGS).
static int fusion_out_bwd_launch(const void* dmixed, const float* dgate, const float* gate, const void* U, const void* a2, const void* g1,
                                 const void* o2, const void* a, const float* alpha_txt, const void* wo, const void* wdo, const void* wd1,
                                 const void* wd2, void* do2, void* da, void* dU, void* dat, void* dg1, void* dl, float* dalpha,
                                 float* const* G, int max_wg, long rows, int C, float alpha_o, float beta_o, float wa, float wb,
                                 float alpha_1, float alpha_2, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || C != 32) return 1;
  if (!dmixed || !gate || !U || !a2 || !g1 || !o2 || !a || !alpha_txt || !wo || !wdo || !wd1 || !wd2 || !do2 || !da || !dU || !dalpha ||
      rows < 0) return HDMOE_EINVAL;
  if (G ? (!G[0] || !G[1] || !G[2] || max_wg < 0) : (!dat || !dg1 || !dl)) return HDMOE_EINVAL;
  if (mis16(dmixed) || mis16(U) || mis16(a2) || mis16(g1) || mis16(o2) || mis16(a) || mis16(wo) || mis16(wdo) || mis16(wd1) || mis16(wd2) ||
      mis16(do2) || mis16(da) || mis16(dU) || mis16(dat) || mis16(dg1) || ((uintptr_t)dl & 3) || (((uintptr_t)dgate | (uintptr_t)gate) & 7) ||
      (((uintptr_t)alpha_txt | (uintptr_t)dalpha) & 3) || rows >= (1l << 40)) return 1;
  if (G && (((uintptr_t)G[0] | (uintptr_t)G[1] | (uintptr_t)G[2]) & 3)) return 1;
  if (rows == 0) return HDMOE_OK;
  FoutBwdArgs k;
  k.dmixed = (const bf16*)dmixed; k.dgate = dgate; k.gate = gate; k.U = (const bf16*)U; k.a2 = (const bf16*)a2; k.g1 = (const bf16*)g1;
  k.o2 = (const bf16*)o2; k.a = (const bf16*)a; k.alpha_txt = alpha_txt; k.wo = (const bf16*)wo; k.wdo = (const bf16*)wdo;
  k.wd1 = (const bf16*)wd1; k.wd2 = (const bf16*)wd2; k.do2 = (bf16*)do2; k.da = (bf16*)da; k.dU = (bf16*)dU; k.dat = (bf16*)dat;
  k.dg1 = (bf16*)dg1; k.dl = (bf16*)dl; k.dalpha = dalpha;
  k.Go = G ? G[0] : nullptr; k.G1 = G ? G[1] : nullptr; k.G2 = G ? G[2] : nullptr;
  k.rows = rows; k.tiles = (rows + 31) / 32; k.ao = alpha_o; k.bo = beta_o; k.wa = wa; k.wb = wb; k.a1 = alpha_1; k.a2g = alpha_2;
  hdmoe_count_selection(HDMOE_SEL_FUSION_OUT_BWD);
  if (G) {
    static unsigned long long attr_set = 0;                    // 56 KB of dynamic LDS: above the 48 KB a kernel gets unasked
    if (hdmoe_first_on_device(attr_set))
      (void)hipFuncSetAttribute((const void*)fusion_out_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 4 * 7 * WG_TILE);
    hipLaunchKernelGGL(fusion_out_bwd_kernel<true>, dim3(wg_grid(k.tiles, max_wg)), dim3(256), 4 * 7 * WG_TILE, stream, k);
  } else {
    // (1024 workgroups at the most: one dalpha atomic each, as hdmoe_lerp_param_bwd caps its grid)
    const unsigned grid = fusion_grid(k.tiles);
    hipLaunchKernelGGL(fusion_out_bwd_kernel<false>, dim3(grid > 1024 ? 1024 : grid), dim3(256), 0, stream, k);
  }
  return hdmoe_launch_status();
}

extern "C" int hdmoe_fusion_out_bwd(const void* dmixed, const float* dgate, const float* gate, const void* U, const void* a2, const void* g1,
                                    const void* o2, const void* a, const float* alpha_txt, const void* wo, const void* wdo, const void* wd1,
                                    const void* wd2, void* do2, void* da, void* dU, void* dat, void* dg1, void* dl, float* dalpha, long rows,
                                    int C, float alpha_o, float beta_o, float wa, float wb, float alpha_1, float alpha_2, int dtype,
                                    hipStream_t stream) {
  return fusion_out_bwd_launch(dmixed, dgate, gate, U, a2, g1, o2, a, alpha_txt, wo, wdo, wd1, wd2, do2, da, dU, dat, dg1, dl, dalpha, nullptr,
                               0, rows, C, alpha_o, beta_o, wa, wb, alpha_1, alpha_2, dtype, stream);
}

extern "C" int hdmoe_fusion_out_bwd_wg(const void* dmixed, const float* dgate, const float* gate, const void* U, const void* a2,
                                       const void* g1, const void* o2, const void* a, const float* alpha_txt, const void* wo, const void* wdo,
                                       const void* wd1, const void* wd2, void* do2, void* da, void* dU, float* dalpha, float* Go, float* G1,
                                       float* G2, int max_wg, long rows, int C, float alpha_o, float beta_o, float wa, float wb,
                                       float alpha_1, float alpha_2, int dtype, hipStream_t stream) {
  float* const G[3] = {Go, G1, G2};
  return fusion_out_bwd_launch(dmixed, dgate, gate, U, a2, g1, o2, a, alpha_txt, wo, wdo, wd1, wd2, do2, da, dU, nullptr, nullptr, nullptr,
                               dalpha, G, max_wg, rows, C, alpha_o, beta_o, wa, wb, alpha_1, alpha_2, dtype, stream);
}

extern "C" int hdmoe_fusion_mid_fwd(const void* o1, const void* query, const void* wo, const void* wq, void* a, void* q2, long rows, int C,
                                    float alpha_o, float beta_o, float alpha_q, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || C != 32) return 1;
  if (!o1 || !query || !wo || !wq || !a || !q2 || rows < 0) return HDMOE_EINVAL;
  if (mis16(o1) || mis16(query) || mis16(wo) || mis16(wq) || mis16(a) || mis16(q2) || rows >= (1l << 40)) return 1;
  if (rows == 0) return HDMOE_OK;
  FmidArgs k;
  k.o1 = (const bf16*)o1; k.query = (const bf16*)query; k.wo = (const bf16*)wo; k.wq = (const bf16*)wq; k.a = (bf16*)a; k.q2 = (bf16*)q2;
  k.rows = rows; k.tiles = (rows + 31) / 32; k.ao = alpha_o; k.bo = beta_o; k.aq = alpha_q;
  hdmoe_count_selection(HDMOE_SEL_FUSION_MID);
  hipLaunchKernelGGL(fusion_mid_fwd_kernel, dim3(fusion_grid(k.tiles)), dim3(256), 0, stream, k);
  return hdmoe_launch_status();
}

extern "C" int hdmoe_fusion_mid_bwd(const void* da, const void* dq2, const void* a, const void* o1, const void* wdo, const void* wdq,
                                    void* do1, void* dres, float* Go, float* Gq, int max_wg, long rows, int C, float alpha_o, float beta_o,
                                    float alpha_q, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_BF16 || C != 32) return 1;
  if (!da || !dq2 || !wdo || !wdq || !do1 || !dres || rows < 0 || (!Go) != (!Gq) || (Go && (!a || !o1 || max_wg < 0))) return HDMOE_EINVAL;
  if (mis16(da) || mis16(dq2) || mis16(a) || mis16(o1) || mis16(wdo) || mis16(wdq) || mis16(do1) || mis16(dres) ||
      (((uintptr_t)Go | (uintptr_t)Gq) & 3) || rows >= (1l << 40)) return 1;
  if (rows == 0) return HDMOE_OK;
  FmidBwdArgs k;
  k.da = (const bf16*)da; k.dq2 = (const bf16*)dq2; k.a = (const bf16*)a; k.o1 = (const bf16*)o1; k.wdo = (const bf16*)wdo;
  k.wdq = (const bf16*)wdq; k.do1 = (bf16*)do1; k.dres = (bf16*)dres; k.Go = Go; k.Gq = Gq;
  k.rows = rows; k.tiles = (rows + 31) / 32; k.ao = alpha_o; k.bo = beta_o; k.aq = alpha_q;
  hdmoe_count_selection(HDMOE_SEL_FUSION_MID_BWD);
  if (Go) hipLaunchKernelGGL(fusion_mid_bwd_kernel<true>, dim3(wg_grid(k.tiles, max_wg)), dim3(256), 4 * 4 * WG_TILE, stream, k);
  else hipLaunchKernelGGL(fusion_mid_bwd_kernel<false>, dim3(fusion_grid(k.tiles)), dim3(256), 0, stream, k);
  return hdmoe_launch_status();
}
