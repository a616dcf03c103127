// Tiled sampling (include/hdmoe.h: hdmoe_tile_gather / hdmoe_tile_blend): crop the model-sized windows of a large fp32 NCHW latent into a
// tile batch, and blend the tile batch of denoiser outputs back with the plan's normalised window weights.  Both are HBM-bound passes:
// grid-stride loops, <= 2048 workgroups of 256 threads (guide G11), one body per kernel over V lanes -- V = 4 is one 16-byte access per
// thread on both sides, V = 1 one element.  The origins live in device memory (static buffers of the sampler's stage state, like the
// schedule t), so the host cannot see whether they allow 16-byte accesses: the launcher checks what it can (W, w, the pointers) and the
// kernel checks the x origins, a wave-uniform loop over <= 32 ints, before it picks the arm.
#include "common.h"
#include "hdmoe.h"

namespace {

constexpr int TPB = 256;

// an origin as the kernels use it: inside [0, L - n] whatever the device array holds, so no access leaves a tensor
DEVI int origin(const int* o, int k, int room) {
  const int v = o[k];
  return v < 0 ? 0 : (v > room ? room : v);
}
// may a thread own four consecutive x?  (W % 4 == 0 and w % 4 == 0 are the launcher's; a clamped origin W - w is then a multiple of 4 too)
DEVI bool origins_x4(const int* ox, int Tx, int room) {
  bool ok = true;
  for (int k = 0; k < Tx; ++k) ok = ok && (origin(ox, k, room) & 3) == 0;
  return ok;
}

struct TileGeom { int C, H, W, h, w, Ty, Tx; };

// tiles[r - row0][c][i][j] = x[b][c][oy[ky] + i][ox[kx] + j], r = (b Ty + ky) Tx + kx.  An item is V consecutive j of one tile line.
template <int V>
DEVI void tile_gather_body(float* tiles, const float* x, const int* oy, const int* ox, TileGeom g, long row0, long rows) {
  const int wv = g.w / V;
  const int per = g.C * g.h * wv;                             // items of one tile-batch row
  const int T = g.Ty * g.Tx;
  GRID_STRIDE(v, rows * per) {
    const long rl = v / per;
    int rem = (int)(v - rl * per);
    const int c = rem / (g.h * wv); rem -= c * (g.h * wv);
    const int i = rem / wv, j = (rem - i * wv) * V;
    const long r = row0 + rl;
    const long b = r / T;
    const int k = (int)(r - b * T), ky = k / g.Tx, kx = k - ky * g.Tx;
    const int y = origin(oy, ky, g.H - g.h) + i, xx = origin(ox, kx, g.W - g.w) + j;
    float f[V];
    ldw<float, V>(f, x + ((b * g.C + c) * g.H + y) * g.W + xx);
    stw<float, V>(tiles + v * V, f);
  }
}

// out[b][c][y][x] = sum_ky sum_kx fl(ny[ky][y] nx[kx][x]) tiles[(b Ty + ky) Tx + kx][c][y - oy[ky]][x - ox[kx]] over the covering tiles, in
// that order.  An item is V consecutive x of one output line; on the V = 4 arm they lie wholly inside or outside any tile.  The cover test
// reads the origins (wave-uniform, scalar loads); the tables and the tiles are read for covering tiles only.  The accumulator starts at
// -0: fma(w, t, -0) = fl(w t) with its sign, so one covering tile of weight 1 returns its value bit for bit.
template <int V>
DEVI void tile_blend_body(float* out, const float* tiles, const int* oy, const int* ox, const float* ny, const float* nx, TileGeom g, long lines) {
#pragma clang fp contract(off)
  const int Wv = g.W / V;
  GRID_STRIDE(v, lines * Wv) {
    const long line = v / Wv;                                 // (b C + c) H + y
    const int x0 = (int)(v - line * Wv) * V;
    const long bc = line / g.H;
    const int y = (int)(line - bc * g.H);
    const long b = bc / g.C;
    const int c = (int)(bc - b * g.C);
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = -0.f;
    for (int ky = 0; ky < g.Ty; ++ky) {
      const int i = y - origin(oy, ky, g.H - g.h);
      if ((unsigned)i >= (unsigned)g.h) continue;
      const float wy = ny[(long)ky * g.H + y];
      if (wy == 0.f) continue;
      for (int kx = 0; kx < g.Tx; ++kx) {
        const int j0 = x0 - origin(ox, kx, g.W - g.w);
        if ((unsigned)j0 >= (unsigned)g.w) continue;          // V == 4: j0 % 4 == 0 and w % 4 == 0, so j0 + 3 < w as well
        float wx[V], t[V];
        ldw<float, V>(wx, nx + (long)kx * g.W + x0);
        ldw<float, V>(t, tiles + ((((b * g.Ty + ky) * g.Tx + kx) * g.C + c) * g.h + i) * g.w + j0);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float wgt = wy * wx[j];
          acc[j] = wx[j] == 0.f ? acc[j] : __builtin_fmaf(wgt, t[j], acc[j]);
        }
      }
    }
    stw<float, V>(out + v * V, acc);
  }
}

// VEC: the launcher found W % 4 == 0, w % 4 == 0 and aligned pointers; the x origins decide between the two arms of the one body
template <bool VEC>
__global__ __launch_bounds__(TPB) void tile_gather_kernel(float* tiles, const float* x, const int* oy, const int* ox, TileGeom g, long row0,
                                                          long rows) {
  if constexpr (VEC) {
    if (origins_x4(ox, g.Tx, g.W - g.w)) { tile_gather_body<4>(tiles, x, oy, ox, g, row0, rows); return; }
  }
  tile_gather_body<1>(tiles, x, oy, ox, g, row0, rows);
}
template <bool VEC>
__global__ __launch_bounds__(TPB) void tile_blend_kernel(float* out, const float* tiles, const int* oy, const int* ox, const float* ny,
                                                         const float* nx, TileGeom g, long lines) {
  if constexpr (VEC) {
    if (origins_x4(ox, g.Tx, g.W - g.w)) { tile_blend_body<4>(out, tiles, oy, ox, ny, nx, g, lines); return; }
  }
  tile_blend_body<1>(out, tiles, oy, ox, ny, nx, g, lines);
}

bool geom_ok(int B, int C, int H, int W, int h, int w, int Ty, int Tx) {
  return B >= 1 && C >= 1 && H >= 1 && W >= 1 && h >= 1 && w >= 1 && h <= H && w <= W && Ty >= 1 && Ty <= HDMOE_TILE_MAX_AXIS && Tx >= 1 &&
         Tx <= HDMOE_TILE_MAX_AXIS && (long)C * h * w <= 0x7fffffffL;   // one tile-batch row is indexed in 32 bits
}

}  // namespace

extern "C" {

int hdmoe_tile_gather(float* tiles, const float* x, const int* oy, const int* ox, int B, int C, int H, int W, int h, int w, int Ty, int Tx,
                      long row0, long rows, hipStream_t stream) {
  if (!tiles || !x || !oy || !ox || !geom_ok(B, C, H, W, h, w, Ty, Tx)) return HDMOE_EINVAL;
  if (row0 < 0 || rows < 1 || row0 + rows > (long)B * Ty * Tx) return HDMOE_EINVAL;
  const TileGeom g{C, H, W, h, w, Ty, Tx};
  const long n = rows * C * h * w;
  if (W % 4 == 0 && w % 4 == 0 && al16(tiles) && al16(x))
    hipLaunchKernelGGL(tile_gather_kernel<true>, dim3(grid_for(n / 4)), dim3(TPB), 0, stream, tiles, x, oy, ox, g, row0, rows);
  else
    hipLaunchKernelGGL(tile_gather_kernel<false>, dim3(grid_for(n)), dim3(TPB), 0, stream, tiles, x, oy, ox, g, row0, rows);
  return hdmoe_launch_status();
}

int hdmoe_tile_blend(float* out, const float* tiles, const int* oy, const int* ox, const float* ny, const float* nx, int B, int C, int H, int W,
                     int h, int w, int Ty, int Tx, hipStream_t stream) {
  if (!out || !tiles || !oy || !ox || !ny || !nx || !geom_ok(B, C, H, W, h, w, Ty, Tx)) return HDMOE_EINVAL;
  const TileGeom g{C, H, W, h, w, Ty, Tx};
  const long lines = (long)B * C * H, n = lines * W;
  if (W % 4 == 0 && w % 4 == 0 && al16(out) && al16(tiles) && al16(nx))
    hipLaunchKernelGGL(tile_blend_kernel<true>, dim3(grid_for(n / 4)), dim3(TPB), 0, stream, out, tiles, oy, ox, ny, nx, g, lines);
  else
    hipLaunchKernelGGL(tile_blend_kernel<false>, dim3(grid_for(n)), dim3(TPB), 0, stream, out, tiles, oy, ox, ny, nx, g, lines);
  return hdmoe_launch_status();
}

}  // extern "C"
