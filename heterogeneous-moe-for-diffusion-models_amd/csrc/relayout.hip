// Data-movement passes around the expert banks with 16-byte global accesses on BOTH sides (round 7).  They do no arithmetic a
// predecessor did not do, in the same order: every kernel here writes, bit for bit, what the kernel it replaces writes (the one
// exception, the dsparse dot product of the combine backward, is noted there).  The predecessors stay as the fallback for the shapes
// these decline (return code 1: nothing launched).
//
// 1. patch <-> image relayout in PixelShuffle order (token feature f = c*p*p + i*p + j), tiled transpose through LDS
//    (replaces patch_to_tokens_o1_vec_kernel and the order-1 branch of patch_relayout_vec_kernel, csrc/elementwise.hip).
//    A tile is tw consecutive tokens of one token row: p image rows x (tw*p) pixels x C channels.  On the image side each of the p
//    rows is one contiguous run of tw*p*C elements, on the token side the whole tile is one contiguous run of tw*C*p*p elements, so
//    both sides move whole 16-byte vectors of fully used cache lines.  LDS holds the tile in IMAGE order [i][x][c] with one 16-byte
//    vector of padding per row i; the image side accesses it with 16-byte operations, the token side with element-size operations
//    (a token vector is 8 (bf16) / 4 (fp32) neighbouring pixels j of one channel, C elements apart in LDS).
//    Banks (2 x 32 lanes per element-size LDS operation, bank = dword address mod 32): consecutive lanes of the token side walk
//    (j-vector, i, c).  With C = 32 bf16 and p = 8, 32 lanes are 8 rows i x 4 channels (2 dwords): the row pad makes the row stride
//    = 4 dwords mod 32, 16 distinct banks, no conflict.  With p = 16 the two j-vectors of a row lie 8 pixels = 128 dwords apart, and
//    no pad that keeps the rows 16-byte aligned moves them off each other: a 2-way conflict on the element-size operation, left in
//    (the LDS traffic of a tile is a small fraction of its HBM time either way, see DESIGN section 3 "Round 7").
//    Persistent grid; a workgroup holds the NEXT tile's global loads in registers while it writes the current tile out of LDS.
// 2. combine_rows forward / backward with 16-byte accesses: a workgroup owns one (row, chunk), decodes the row once and reads
//    inv / perm / row_w once (wave-uniform), instead of a 64-bit division and an index load per 2-byte element.
#include "common.h"
#include "conv_args.h"
#include "hdmoe.h"

namespace {

constexpr int TPB = 256;
constexpr int RL_MAXV = 8;                                  // 16-byte vectors per thread and tile
constexpr int RL_TILE_MAX = RL_MAXV * TPB * 16;             // a tile (at least one token) is at most 32 KiB ...
constexpr int RL_TILE_TARGET = RL_TILE_MAX / 2;             // ... and as many whole tokens as fit 16 KiB
constexpr int RL_PMAX = 64;
constexpr int RL_LDS_BYTES = RL_TILE_MAX + RL_PMAX * 16;    // + one 16-byte pad per image row of the tile
constexpr int RL_GRID = 512;                                // two workgroups per CU, each with two tiles' loads in flight

struct RlArgs {
  void* tok; void* img;
  int H, W, C, p, hp, wp, TW, tpr;                          // TW tokens per full tile, tpr tiles per token row
  long ntiles;
  const int* rows;                                          // device {begin, end}: only the tiles of image rows [begin, end) (null: all N)
  int N;
};
// first tile and tile count of the launch: all of them, or those of the row window read from device memory (clamped to [0, N])
DEVI void rl_window(const RlArgs& a, long& t0, long& nt) {
  t0 = 0; nt = a.ntiles;
  if (a.rows) {
    int b = a.rows[0], e = a.rows[1];
    b = b < 0 ? 0 : (b > a.N ? a.N : b);
    e = e < b ? b : (e > a.N ? a.N : e);
    const long tpi = (long)a.hp * a.tpr;
    t0 = b * tpi; nt = (e - b) * tpi;
  }
}

// geometry of tile t
struct RlTile {
  long img0, tok0;        // element offsets: image (b, ph*p, pw0*p, 0) and token (b, ph, pw0, 0)
  int nvec, rowv, RS;     // 16-byte vectors in the tile / in one image row of it; LDS row stride in elements
  int ylim, xlimv;        // rows i < ylim and row vectors < xlimv lie inside the image
};
template <typename T, int P>
DEVI RlTile rl_tile(const RlArgs& a, long t) {
  constexpr int VW = VT<T>::W;
  const int p = P ? P : a.p;
  const long band = t / a.tpr;
  const int pw0 = (int)(t - band * a.tpr) * a.TW;
  const int tw = a.wp - pw0 < a.TW ? a.wp - pw0 : a.TW;
  const long b = band / a.hp;
  const int ph = (int)(band - b * a.hp);
  const int CV = a.C / VW;
  RlTile g;
  g.img0 = ((b * a.H + (long)ph * p) * a.W + (long)pw0 * p) * a.C;
  g.tok0 = (band * a.wp + pw0) * ((long)a.C * p * p);
  g.rowv = tw * p * CV;
  g.nvec = g.rowv * p;
  g.RS = g.rowv * VW + VW;
  g.ylim = a.H - ph * p;
  const int xl = a.W - pw0 * p;
  g.xlimv = xl <= 0 ? 0 : (xl >= tw * p ? g.rowv : xl * CV);
  return g;
}

// global -> registers: the tile's source side, vector v = tid + k * TPB
template <typename T, int P, bool TO_IMG>
DEVI void rl_load(uint4 (&r)[RL_MAXV], const RlArgs& a, const RlTile& g) {
  constexpr int VW = VT<T>::W;
#pragma unroll
  for (int k = 0; k < RL_MAXV; ++k) {
    const int v = (int)threadIdx.x + k * TPB;
    if (v < g.nvec) {
      if (TO_IMG) {
        r[k] = *reinterpret_cast<const uint4*>(static_cast<const T*>(a.tok) + g.tok0 + (long)v * VW);
      } else {
        const int ii = v / g.rowv, rest = v - ii * g.rowv;
        r[k] = (ii < g.ylim && rest < g.xlimv)
                   ? *reinterpret_cast<const uint4*>(static_cast<const T*>(a.img) + g.img0 + (long)ii * a.W * a.C + (long)rest * VW)
                   : make_uint4(0, 0, 0, 0);                                            // outside the image: zero tokens
      }
    }
  }
}

// token vector v of the tile -> LDS element offset of its first element (the others follow C elements apart)
template <typename T, int P>
DEVI int rl_tok_lds(const RlArgs& a, const RlTile& g, int v) {
  constexpr int VW = VT<T>::W;
  const int p = P ? P : a.p;
  const int jvn = p / VW, KV = a.C * p * jvn;
  const int tl = v / KV, rem = v - tl * KV;
  const int jv = rem % jvn, t2 = rem / jvn;
  const int ii = t2 % p, c = t2 / p;
  return ii * g.RS + (tl * p + jv * VW) * a.C + c;
}

template <typename T, int P, bool TO_IMG>
__global__ __launch_bounds__(TPB) void patch_relayout_tiled_kernel(RlArgs a) {
  constexpr int VW = VT<T>::W;
  __shared__ uint4 lds4[RL_LDS_BYTES / 16];
  T* lds = reinterpret_cast<T*>(lds4);
  uint4 r[RL_MAXV];
  long t0, nt;
  rl_window(a, t0, nt);
  long t = blockIdx.x;
  if (t >= nt) return;
  RlTile g = rl_tile<T, P>(a, t0 + t);
  rl_load<T, P, TO_IMG>(r, a, g);
  while (true) {
    // registers -> LDS (image order)
#pragma unroll
    for (int k = 0; k < RL_MAXV; ++k) {
      const int v = (int)threadIdx.x + k * TPB;
      if (v < g.nvec) {
        if (TO_IMG) {
          const int o = rl_tok_lds<T, P>(a, g, v);
          alignas(16) T e[VW];
          *reinterpret_cast<uint4*>(e) = r[k];
#pragma unroll
          for (int j = 0; j < VW; ++j) lds[o + j * a.C] = e[j];
        } else {
          const int ii = v / g.rowv, rest = v - ii * g.rowv;
          *reinterpret_cast<uint4*>(lds + ii * g.RS + rest * VW) = r[k];
        }
      }
    }
    __syncthreads();
    const long tn = t + gridDim.x;
    const RlTile gc = g;
    if (tn < nt) {                                         // the next tile's loads fly while this one leaves LDS
      g = rl_tile<T, P>(a, t0 + tn);
      rl_load<T, P, TO_IMG>(r, a, g);
    }
    // LDS -> global
#pragma unroll
    for (int k = 0; k < RL_MAXV; ++k) {
      const int v = (int)threadIdx.x + k * TPB;
      if (v < gc.nvec) {
        if (TO_IMG) {
          const int ii = v / gc.rowv, rest = v - ii * gc.rowv;
          if (ii < gc.ylim && rest < gc.xlimv)
            *reinterpret_cast<uint4*>(static_cast<T*>(a.img) + gc.img0 + (long)ii * a.W * a.C + (long)rest * VW) =
                *reinterpret_cast<const uint4*>(lds + ii * gc.RS + rest * VW);
        } else {
          const int o = rl_tok_lds<T, P>(a, gc, v);
          alignas(16) T e[VW];
#pragma unroll
          for (int j = 0; j < VW; ++j) e[j] = lds[o + j * a.C];
          *reinterpret_cast<uint4*>(static_cast<T*>(a.tok) + gc.tok0 + (long)v * VW) = *reinterpret_cast<const uint4*>(e);
        }
      }
    }
    if (tn >= nt) break;
    t = tn;
    __syncthreads();
  }
}

template <typename T, bool TO_IMG>
int rl_launch(const RlArgs& a, unsigned grid, hipStream_t stream) {
  constexpr int VW = VT<T>::W;
  if (a.p == VW) hipLaunchKernelGGL((patch_relayout_tiled_kernel<T, VW, TO_IMG>), dim3(grid), dim3(TPB), 0, stream, a);
  else if (a.p == 2 * VW) hipLaunchKernelGGL((patch_relayout_tiled_kernel<T, 2 * VW, TO_IMG>), dim3(grid), dim3(TPB), 0, stream, a);
  else if (a.p == 4 * VW) hipLaunchKernelGGL((patch_relayout_tiled_kernel<T, 4 * VW, TO_IMG>), dim3(grid), dim3(TPB), 0, stream, a);
  else hipLaunchKernelGGL((patch_relayout_tiled_kernel<T, 0, TO_IMG>), dim3(grid), dim3(TPB), 0, stream, a);
  return hdmoe_launch_status();
}

// ---------------------------------------------------------------- combine_rows, 16-byte forms
constexpr int CR_U = 4;                                     // vectors per thread: a workgroup owns TPB * CR_U vectors of one row

// out[b][:] = sum_j w[r_j] * ys[r_j][:], r_j = inv[b][j], j = 0..kcap-1 in this order in fp32, as combine_rows_fwd_kernel
template <typename T>
__global__ __launch_bounds__(TPB) void combine_rows_fwd_vec_kernel(T* out, const T* ys, const int* inv, const float* row_w, int kcap, long L,
                                                                   unsigned nck) {
  constexpr int VW = VT<T>::W;
  const long b = blockIdx.x / nck;
  const long p0 = (long)(blockIdx.x - b * nck) * (TPB * CR_U * VW) + (long)threadIdx.x * VW;
  float acc[CR_U][VW];
#pragma unroll
  for (int u = 0; u < CR_U; ++u)
#pragma unroll
    for (int k = 0; k < VW; ++k) acc[u][k] = 0.f;
  for (int j = 0; j < kcap; ++j) {
    const int r = inv[b * kcap + j];
    if (r < 0) continue;
    const float w = row_w ? row_w[r] : 1.f;
    if (!(w > 0.f)) continue;
    const T* src = ys + (long)r * L;
#pragma unroll
    for (int u = 0; u < CR_U; ++u) {
      const long i = p0 + (long)u * (TPB * VW);
      if (i < L) {
        float f[VW];
        vload<T>(f, src + i);
#pragma unroll
        for (int k = 0; k < VW; ++k) acc[u][k] += w * f[k];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < CR_U; ++u) {
    const long i = p0 + (long)u * (TPB * VW);
    if (i < L) vstore<T>(out + b * L + i, acc[u]);
  }
}

// dys[r][:] = w[r] * dout[perm[r]][:] (bit for bit as combine_rows_bwd_kernel);  dsparse[perm[r]][row_expert[r]] += <dout[perm[r]], ys[r]>:
// the partial dot product of a (row, chunk) is summed in another tree than the predecessor's (8 / 4 elements per thread first), and
// joins the other chunks' through the same float atomic.
template <typename T>
__global__ __launch_bounds__(TPB) void combine_rows_bwd_vec_kernel(T* dys, float* dsparse, const T* dout, const T* ys, const int* perm,
                                                                   const int* row_expert, const float* row_w, int E, long L, unsigned nck) {
  constexpr int VW = VT<T>::W;
  __shared__ float sm[16];
  const long r = blockIdx.x / nck;
  const int b = perm[r];
  const long p0 = (long)(blockIdx.x - r * nck) * (TPB * CR_U * VW) + (long)threadIdx.x * VW;
  const float w = b >= 0 ? (row_w ? row_w[r] : 1.f) : 0.f;
  const bool dot = dsparse && b >= 0;
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < CR_U; ++u) {
    const long i = p0 + (long)u * (TPB * VW);
    if (i < L) {
      float g[VW], o[VW];
#pragma unroll
      for (int k = 0; k < VW; ++k) g[k] = 0.f;
      if (b >= 0) vload<T>(g, dout + (long)b * L + i);
#pragma unroll
      for (int k = 0; k < VW; ++k) o[k] = w * g[k];
      vstore<T>(dys + r * L + i, o);
      if (dot) {
        float y[VW];
        vload<T>(y, ys + r * L + i);
#pragma unroll
        for (int k = 0; k < VW; ++k) acc += g[k] * y[k];
      }
    }
  }
  if (dsparse) {
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0 && b >= 0) atomicAdd(&dsparse[(long)b * E + row_expert[r]], acc);
  }
}

}  // namespace

extern "C" {

// 0: launched; 1: outside the tiled kernel's domain, nothing launched (the caller runs hdmoe_patch_relayout)
static int rl_entry(void* out, const void* in, const int* rows, int N, int H, int W, int C, int p, int hp, int wp, int order, int to_img, int dtype,
                    hipStream_t stream) {
  if (!out || !in || N < 0 || H < 1 || W < 1 || C < 1 || p < 1 || hp < 1 || wp < 1 || (long)hp * p < H || (long)wp * p < W) return HDMOE_EINVAL;
  if (order != 1 || (dtype != HDMOE_BF16 && dtype != HDMOE_F32)) return 1;
  const int VW = dtype == HDMOE_BF16 ? 8 : 4, esz = dtype == HDMOE_BF16 ? 2 : 4;
  if (p % VW || C % VW || p > RL_PMAX || !al16(out) || !al16(in)) return 1;
  const long tokb = (long)C * p * p * esz;
  if (tokb > RL_TILE_MAX) return 1;
  if (N == 0) return HDMOE_OK;
  RlArgs a;
  a.tok = to_img ? const_cast<void*>(in) : out;
  a.img = to_img ? out : const_cast<void*>(in);
  a.H = H; a.W = W; a.C = C; a.p = p; a.hp = hp; a.wp = wp; a.rows = rows; a.N = N;
  long TW = RL_TILE_TARGET / tokb;
  if (TW < 1) TW = 1;
  if (TW > wp) TW = wp;
  a.TW = (int)TW;
  a.tpr = (wp + a.TW - 1) / a.TW;
  a.ntiles = (long)N * hp * a.tpr;
  if ((long)N * hp * wp * (tokb / esz) >= (1l << 40)) return 1;
  const unsigned grid = (unsigned)(a.ntiles < RL_GRID ? a.ntiles : RL_GRID);
  hdmoe_count_selection(rows ? HDMOE_SEL_ROW_WINDOW : HDMOE_SEL_RELAYOUT_TILED);
  if (dtype == HDMOE_BF16) return to_img ? rl_launch<bf16, true>(a, grid, stream) : rl_launch<bf16, false>(a, grid, stream);
  return to_img ? rl_launch<float, true>(a, grid, stream) : rl_launch<float, false>(a, grid, stream);
}
int hdmoe_patch_relayout_tiled(void* out, const void* in, int N, int H, int W, int C, int p, int hp, int wp, int order, int to_img,
                               int dtype, hipStream_t stream) {
  return rl_entry(out, in, nullptr, N, H, W, C, p, hp, wp, order, to_img, dtype, stream);
}
// The same over the image rows [rows[0], rows[1]) only (rows: DEVICE pointer to two ints, read by the kernel): the launch has the
// all-rows grid, rows outside the window are neither read nor written, an empty window does nothing.
int hdmoe_patch_relayout_tiled_rows(void* out, const void* in, const int* rows, int N, int H, int W, int C, int p, int hp, int wp, int order,
                                    int to_img, int dtype, hipStream_t stream) {
  if (!rows) return HDMOE_EINVAL;
  return rl_entry(out, in, rows, N, H, W, C, p, hp, wp, order, to_img, dtype, stream);
}

// 0: launched; 1: L is not a whole number of 16-byte vectors or a pointer is not 16-byte aligned, nothing launched
int hdmoe_combine_rows_fwd_vec(void* out, const void* ys, const int* inv, const float* row_w, long B, int kcap, long L, int dtype,
                               hipStream_t stream) {
  if (dtype != HDMOE_F32 && dtype != HDMOE_BF16) return HDMOE_EDTYPE;
  if (!out || !ys || !inv || B < 0 || kcap < 1 || L < 1) return HDMOE_EINVAL;
  const int VW = dtype == HDMOE_BF16 ? 8 : 4;
  if (L % VW || !al16(out) || !al16(ys)) return 1;
  if (B == 0) return HDMOE_OK;
  const long nck = cdiv(L, (long)TPB * CR_U * VW);
  if (B * nck >= (1l << 31)) return 1;
  hdmoe_count_selection(HDMOE_SEL_COMBINE_FWD_VEC);
  if (dtype == HDMOE_F32) hipLaunchKernelGGL(combine_rows_fwd_vec_kernel<float>, dim3((unsigned)(B * nck)), dim3(TPB), 0, stream, (float*)out, (const float*)ys, inv, row_w, kcap, L, (unsigned)nck);
  else hipLaunchKernelGGL(combine_rows_fwd_vec_kernel<bf16>, dim3((unsigned)(B * nck)), dim3(TPB), 0, stream, (bf16*)out, (const bf16*)ys, inv, row_w, kcap, L, (unsigned)nck);
  return hdmoe_launch_status();
}
int hdmoe_combine_rows_bwd_vec(void* dys, float* dsparse, const void* dout, const void* ys, const int* perm, const int* row_expert,
                               const float* row_w, long R, int E, long L, int dtype, hipStream_t stream) {
  if (dtype != HDMOE_F32 && dtype != HDMOE_BF16) return HDMOE_EDTYPE;
  if (!dys || !dout || !perm || R < 0 || L < 1 || (dsparse && (!ys || !row_expert || E < 1))) return HDMOE_EINVAL;
  const int VW = dtype == HDMOE_BF16 ? 8 : 4;
  if (L % VW || !al16(dys) || !al16(dout) || !al16(ys)) return 1;
  if (R == 0) return HDMOE_OK;
  const long nck = cdiv(L, (long)TPB * CR_U * VW);
  if (R * nck >= (1l << 31)) return 1;
  hdmoe_count_selection(HDMOE_SEL_COMBINE_BWD_VEC);
  if (dtype == HDMOE_F32) hipLaunchKernelGGL(combine_rows_bwd_vec_kernel<float>, dim3((unsigned)(R * nck)), dim3(TPB), 0, stream, (float*)dys, dsparse, (const float*)dout, (const float*)ys, perm, row_expert, row_w, E, L, (unsigned)nck);
  else hipLaunchKernelGGL(combine_rows_bwd_vec_kernel<bf16>, dim3((unsigned)(R * nck)), dim3(TPB), 0, stream, (bf16*)dys, dsparse, (const bf16*)dout, (const bf16*)ys, perm, row_expert, row_w, E, L, (unsigned)nck);
  return hdmoe_launch_status();
}

}  // extern "C"
