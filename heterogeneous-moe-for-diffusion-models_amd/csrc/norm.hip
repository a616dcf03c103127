// K6: normalisation kernels (fwd + bwd), NHWC / [rows][C]; statistics always in fp32.
//   pixel-norm  : normalize(x, dim=[1])            reference models/model_internals.py:8-30, model_components.py:238
//   GroupNorm   : nn.GroupNorm(G, C) (+ReLU / +mp_silu fused)   model_components.py:102-109, :491, :530
//   LayerNorm   : nn.LayerNorm(C)                  model_components.py:495-496, :645
#include "common.h"
#include "hdmoe.h"

namespace {

constexpr int TPB = 256;

// ---------------------------------------------------------------- pixel norm (one thread per pixel row)
template <typename T>
__global__ void pixelnorm_fwd_kernel(T* xn, T* h, const T* x, int C, long rows) {
  const float rc = rsqrtf((float)C);
  GRID_STRIDE(r, rows) {
    const T* p = x + r * C;
    float ss = 0.f;
    for (int c = 0; c < C; ++c) { const float v = to_f(p[c]); ss += v * v; }
    const float inv = 1.f / (1e-4f + sqrtf(ss) * rc);
    for (int c = 0; c < C; ++c) {
      const float v = to_f(p[c]) * inv;
      xn[r * C + c] = from_f<T>(v);
      if (h) h[r * C + c] = from_f<T>(mp_silu_f(v));
    }
  }
}
// g = dxn + dh * mp_silu'(xn);  dx = g/d - x * (sum g*x) * rc / (d^2 * n)
template <typename T>
__global__ void pixelnorm_bwd_kernel(T* dx, const T* dxn, const T* dh, const T* x, int C, long rows, float sx) {
  const float rc = rsqrtf((float)C);
  GRID_STRIDE(r, rows) {
    const T* p = x + r * C;
    float ss = 0.f;
    for (int c = 0; c < C; ++c) { const float v = to_f(p[c]); ss += v * v; }
    const float nrm = sqrtf(ss);
    const float d = 1e-4f + nrm * rc, inv = 1.f / d;
    float dot = 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = to_f(p[c]);
      float g = dxn ? sx * to_f(dxn[r * C + c]) : 0.f;
      if (dh) g += to_f(dh[r * C + c]) * mp_silu_grad_f(v * inv);
      dot += g * v;
    }
    const float k2 = nrm > 0.f ? dot * rc * inv * inv / nrm : 0.f;
    for (int c = 0; c < C; ++c) {
      const float v = to_f(p[c]);
      float g = dxn ? sx * to_f(dxn[r * C + c]) : 0.f;
      if (dh) g += to_f(dh[r * C + c]) * mp_silu_grad_f(v * inv);
      dx[r * C + c] = from_f<T>(g * inv - k2 * v);
    }
  }
}

// ---------------------------------------------------------------- GroupNorm (the arithmetic: gn_fwd_f / gn_xhat / gn_dz / gn_dx of common.h)
// per-group block reduction: thread t owns group t % G (requires blockDim % G == 0); result for group g in red[g]
DEVI void group_reduce(float v, int G, float* part, float* red) {
  __syncthreads();
  part[threadIdx.x] = v;
  __syncthreads();
  if ((int)threadIdx.x < G) {
    float s = 0.f;
    for (int t = threadIdx.x; t < (int)blockDim.x; t += G) s += part[t];
    red[threadIdx.x] = s;
  }
  __syncthreads();
}

// one block per sample; items = (position s, group g) pairs, item -> Cg contiguous channels; two-pass variance
template <typename T>
__global__ __launch_bounds__(512) void groupnorm_stats_kernel(float* mean, float* rstd, const T* x, long S, int C, int G, float eps) {
  __shared__ float part[512];
  __shared__ float red[64];
  const int n = blockIdx.x, Cg = C / G;
  const T* xs = x + (long)n * S * C;
  const long items = S * G;
  float acc = 0.f;
  for (long it = threadIdx.x; it < items; it += blockDim.x) {
    const T* p = xs + (it / G) * C + (it % G) * Cg;
    for (int c = 0; c < Cg; ++c) acc += to_f(p[c]);
  }
  group_reduce(acc, G, part, red);
  const float m = red[threadIdx.x % G] / (float)(S * Cg);
  acc = 0.f;
  for (long it = threadIdx.x; it < items; it += blockDim.x) {
    const T* p = xs + (it / G) * C + (it % G) * Cg;
    for (int c = 0; c < Cg; ++c) { const float d = to_f(p[c]) - m; acc += d * d; }
  }
  group_reduce(acc, G, part, red);
  if ((int)threadIdx.x < G) {
    mean[(long)n * G + threadIdx.x] = m;
    rstd[(long)n * G + threadIdx.x] = rsqrtf(red[threadIdx.x] / (float)(S * Cg) + eps);
  }
}
// y = act(GroupNorm(x)), W channels of one group per thread: W = 1, or 16-byte vectors where gn_vec_ok
template <typename T, int W>
__global__ void groupnorm_apply_kernel(T* y, const T* x, const float* gamma, const float* beta, const float* mean,
                                       const float* rstd, long S, int C, int G, int act, long nvec) {
  const int Cg = C / G, cv = C / W;
  GRID_STRIDE(v, nvec) {
    const long row = v / cv; const int c0 = (int)(v - row * cv) * W;
    const long sg = (row / S) * G + c0 / Cg;
    const float m = mean[sg], rs = rstd[sg];
    float f[W];
    ldw<T, W>(f, x + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] = gn_fwd_f(f[j], m, rs, gamma[c0 + j], beta[c0 + j], act);
    stw<T, W>(y + v * W, f);
  }
}
// bwd pass 1: per (sample, group) s1 = sum dz*gamma, s2 = sum dz*gamma*xhat ; per-channel dgamma/dbeta (atomics)
template <typename T>
__global__ __launch_bounds__(512) void groupnorm_bwd_stats_kernel(float* s1, float* s2, float* dgamma, float* dbeta, const T* dy,
                                                                 const T* x, const float* gamma, const float* beta,
                                                                 const float* mean, const float* rstd, long S, int C, int G, int act) {
  extern __shared__ float sm[];          // [2*C] per-channel partials
  __shared__ float part[512];
  __shared__ float red[64];
  const int n = blockIdx.x, Cg = C / G;
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) sm[c] = 0.f;
  __syncthreads();
  const long base = (long)n * S * C;
  const long items = S * G;
  const int g = threadIdx.x % G;
  const float m = mean[(long)n * G + g], rs = rstd[(long)n * G + g];
  float a1 = 0.f, a2 = 0.f;
  for (long it = threadIdx.x; it < items; it += blockDim.x) {
    const long off = base + (it / G) * C + g * Cg;
    for (int c = 0; c < Cg; ++c) {
      const int ch = g * Cg + c;
      const float xh = gn_xhat(to_f(x[off + c]), m, rs);
      const float dz = gn_dz(to_f(dy[off + c]), xh, gamma[ch], beta[ch], act);
      a1 += dz * gamma[ch];
      a2 += dz * gamma[ch] * xh;
      atomicAdd(&sm[ch], dz * xh);
      atomicAdd(&sm[C + ch], dz);
    }
  }
  group_reduce(a1, G, part, red);
  if ((int)threadIdx.x < G) s1[(long)n * G + threadIdx.x] = red[threadIdx.x];
  group_reduce(a2, G, part, red);
  if ((int)threadIdx.x < G) s2[(long)n * G + threadIdx.x] = red[threadIdx.x];
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    atomicAdd(&dgamma[c], sm[c]);
    atomicAdd(&dbeta[c], sm[C + c]);
  }
}
// bwd pass 2, one element per thread.  Not the W = 1 form of groupnorm_bwd_apply_vec_kernel: as compiled, this kernel rounds dz * gamma and
// invm * (s1 + xh * s2) each on its own (one packed multiply) and the vector kernel contracts the difference into an fma, at every width,
// so one body cannot keep the bits of both
template <typename T>
__global__ void groupnorm_bwd_apply_kernel(T* dx, const T* dy, const T* x, const float* gamma, const float* beta, const float* mean,
                                           const float* rstd, const float* s1, const float* s2, long S, int C, int G, int act, long n) {
  const int Cg = C / G;
  const float invm = 1.f / (float)(S * Cg);
  GRID_STRIDE(i, n) {
    const long row = i / C; const int c = (int)(i - row * C);
    const long sg = (row / S) * G + c / Cg;
    const float rs = rstd[sg];
    const float xh = gn_xhat(to_f(x[i]), mean[sg], rs);
    dx[i] = from_f<T>(gn_dx(gn_dz(to_f(dy[i]), xh, gamma[c], beta[c], act), xh, rs, gamma[c], invm, s1[sg], s2[sg]));
  }
}
// bwd pass 2, W channels of one group per thread in 16-byte (or, bf16 next to fp32, 8-byte) accesses.  TD: the type of dy and dx where it
// is not x's (router-trunk backward in bf16 mode: fp32 activations next to bf16 gradients, 4 of each per thread).
// dyb (or null): the incoming gradient is dyb[n][c] * dybs at every position (the backward of a mean over the positions) -- read from
// the (N, C) tensor instead of a materialised broadcast
template <typename T, typename TD = T, int W = VT<T>::W>
__global__ void groupnorm_bwd_apply_vec_kernel(TD* dx, const TD* dy, const T* x, const float* gamma, const float* beta, const float* mean,
                                               const float* rstd, const float* s1, const float* s2, long S, int C, int G, int act, long nvec,
                                               const float* dyb, float dybs) {
  const int Cg = C / G, cv = C / W;
  const float invm = 1.f / (float)(S * Cg);
  GRID_STRIDE(v, nvec) {
    const long row = v / cv; const int c0 = (int)(v - row * cv) * W;
    const long sg = (row / S) * G + c0 / Cg;
    const float m = mean[sg], rs = rstd[sg], u = s1[sg], w = s2[sg];
    float f[W], d[W];
    ldw<T, W>(f, x + v * W);
    if (dyb) {
#pragma unroll
      for (int j = 0; j < W; ++j) d[j] = dyb[(row / S) * C + c0 + j] * dybs;
    } else {
      ldw<TD, W>(d, dy + v * W);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float xh = gn_xhat(f[j], m, rs);
      d[j] = gn_dx(gn_dz(d[j], xh, gamma[c0 + j], beta[c0 + j], act), xh, rs, gamma[c0 + j], invm, u, w);
    }
    stw<TD, W>(dx + v * W, d);
  }
}

// ---------------------------------------------------------------- LayerNorm (one thread per row, C <= ~1024)
template <typename T>
__global__ void layernorm_fwd_kernel(T* y, float* mean, float* rstd, const T* x, const float* gamma, const float* beta, int C, float eps, long rows) {
  GRID_STRIDE(r, rows) {
    const T* p = x + r * C;
    float m = 0.f;
    for (int c = 0; c < C; ++c) m += to_f(p[c]);
    m /= (float)C;
    float v = 0.f;
    for (int c = 0; c < C; ++c) { const float d = to_f(p[c]) - m; v += d * d; }
    const float rs = rsqrtf(v / (float)C + eps);
    mean[r] = m; rstd[r] = rs;
    for (int c = 0; c < C; ++c) y[r * C + c] = from_f<T>((to_f(p[c]) - m) * rs * gamma[c] + beta[c]);
  }
}
template <typename T>
__global__ void layernorm_bwd_kernel(T* dx, float* dgamma, float* dbeta, const T* dy, const T* x, const float* gamma,
                                     const float* mean, const float* rstd, int C, long rows) {
  extern __shared__ float sm[];     // [2*C]
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) sm[c] = 0.f;
  __syncthreads();
  GRID_STRIDE(r, rows) {
    const float m = mean[r], rs = rstd[r];
    float a1 = 0.f, a2 = 0.f;
    for (int c = 0; c < C; ++c) {
      const float g = to_f(dy[r * C + c]), xh = (to_f(x[r * C + c]) - m) * rs;
      a1 += g * gamma[c];
      a2 += g * gamma[c] * xh;
      atomicAdd(&sm[c], g * xh);
      atomicAdd(&sm[C + c], g);
    }
    const float ic = 1.f / (float)C;
    for (int c = 0; c < C; ++c) {
      const float g = to_f(dy[r * C + c]), xh = (to_f(x[r * C + c]) - m) * rs;
      dx[r * C + c] = from_f<T>(rs * (g * gamma[c] - ic * (a1 + xh * a2)));
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    atomicAdd(&dgamma[c], sm[c]);
    atomicAdd(&dbeta[c], sm[C + c]);
  }
}


// =====================================================================================================================
// Vectorised variants (16-byte accesses, guide G13).  A row of C channels is spread over LPR = pow2 >= C/VW lanes, one
// 16-byte vector per lane; row reductions are xor-shuffles inside the LPR-lane group (no LDS).
// =====================================================================================================================
template <int LPR> DEVI float group_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T, int LPR>
__global__ __launch_bounds__(256) void pixelnorm_fwd_vec_kernel(T* xn, T* h, const T* x, int C, long rows) {
  constexpr int W = VT<T>::W;
  const int sub = threadIdx.x % LPR;
  const bool act = sub * W < C;
  const float rc = rsqrtf((float)C);
  for (long r = ((long)blockIdx.x * blockDim.x + threadIdx.x) / LPR; r < rows; r += (long)gridDim.x * blockDim.x / LPR) {
    float v[W];
    float ss = 0.f;
    if (act) {
      vload<T>(v, x + r * C + sub * W);
#pragma unroll
      for (int j = 0; j < W; ++j) ss += v[j] * v[j];
    }
    ss = group_sum<LPR>(ss);
    const float inv = 1.f / (1e-4f + sqrtf(ss) * rc);
    if (act) {
      float o[W];
#pragma unroll
      for (int j = 0; j < W; ++j) o[j] = v[j] * inv;
      vstore<T>(xn + r * C + sub * W, o);
      if (h) {
#pragma unroll
        for (int j = 0; j < W; ++j) o[j] = mp_silu_f(o[j]);
        vstore<T>(h + r * C + sub * W, o);
      }
    }
  }
}
template <typename T, int LPR>
__global__ __launch_bounds__(256) void pixelnorm_bwd_vec_kernel(T* dx, const T* dxn, const T* dh, const T* x, int C, long rows, float sx) {
  constexpr int W = VT<T>::W;
  const int sub = threadIdx.x % LPR;
  const bool act = sub * W < C;
  const float rc = rsqrtf((float)C);
  for (long r = ((long)blockIdx.x * blockDim.x + threadIdx.x) / LPR; r < rows; r += (long)gridDim.x * blockDim.x / LPR) {
    float v[W], g[W], t[W];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < W; ++j) { v[j] = 0.f; g[j] = 0.f; }
    if (act) {
      vload<T>(v, x + r * C + sub * W);
      if (dxn) {
        vload<T>(g, dxn + r * C + sub * W);
#pragma unroll
        for (int j = 0; j < W; ++j) g[j] *= sx;
      }
#pragma unroll
      for (int j = 0; j < W; ++j) ss += v[j] * v[j];
    }
    ss = group_sum<LPR>(ss);
    const float nrm = sqrtf(ss);
    const float inv = 1.f / (1e-4f + nrm * rc);
    float dot = 0.f;
    if (act) {
      if (dh) {
        vload<T>(t, dh + r * C + sub * W);
#pragma unroll
        for (int j = 0; j < W; ++j) g[j] += t[j] * mp_silu_grad_f(v[j] * inv);
      }
#pragma unroll
      for (int j = 0; j < W; ++j) dot += g[j] * v[j];
    }
    dot = group_sum<LPR>(dot);
    const float k2 = nrm > 0.f ? dot * rc * inv * inv / nrm : 0.f;
    if (act) {
#pragma unroll
      for (int j = 0; j < W; ++j) t[j] = g[j] * inv - k2 * v[j];
      vstore<T>(dx + r * C + sub * W, t);
    }
  }
}

template <typename T, int LPR>
__global__ __launch_bounds__(256) void layernorm_fwd_vec_kernel(T* y, float* mean, float* rstd, const T* x, const float* gamma,
                                                               const float* beta, int C, float eps, long rows) {
  constexpr int W = VT<T>::W;
  const int sub = threadIdx.x % LPR;
  const bool act = sub * W < C;
  float gm[W], bt[W];
#pragma unroll
  for (int j = 0; j < W; ++j) { gm[j] = act ? gamma[sub * W + j] : 0.f; bt[j] = act ? beta[sub * W + j] : 0.f; }
  for (long r = ((long)blockIdx.x * blockDim.x + threadIdx.x) / LPR; r < rows; r += (long)gridDim.x * blockDim.x / LPR) {
    float v[W];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < W; ++j) v[j] = 0.f;
    if (act) vload<T>(v, x + r * C + sub * W);
#pragma unroll
    for (int j = 0; j < W; ++j) s += v[j];
    const float m = group_sum<LPR>(s) / (float)C;
    float q = 0.f;
    if (act) {
#pragma unroll
      for (int j = 0; j < W; ++j) { const float d = v[j] - m; q += d * d; }
    }
    const float rs = rsqrtf(group_sum<LPR>(q) / (float)C + eps);
    if (sub == 0) { mean[r] = m; rstd[r] = rs; }
    if (act) {
#pragma unroll
      for (int j = 0; j < W; ++j) v[j] = (v[j] - m) * rs * gm[j] + bt[j];
      vstore<T>(y + r * C + sub * W, v);
    }
  }
}
template <typename T, int LPR>
__global__ __launch_bounds__(256) void layernorm_bwd_vec_kernel(T* dx, float* dgamma, float* dbeta, const T* dy, const T* x,
                                                               const float* gamma, const float* mean, const float* rstd, int C, long rows) {
  constexpr int W = VT<T>::W;
  extern __shared__ float sm[];     // [2*C]
  for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) sm[c] = 0.f;
  __syncthreads();
  const int sub = threadIdx.x % LPR;
  const bool act = sub * W < C;
  float gm[W], dg[W], db[W];
#pragma unroll
  for (int j = 0; j < W; ++j) { gm[j] = act ? gamma[sub * W + j] : 0.f; dg[j] = 0.f; db[j] = 0.f; }
  const float ic = 1.f / (float)C;
  for (long r = ((long)blockIdx.x * blockDim.x + threadIdx.x) / LPR; r < rows; r += (long)gridDim.x * blockDim.x / LPR) {
    float v[W], g[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { v[j] = 0.f; g[j] = 0.f; }
    const float m = mean[r], rs = rstd[r];
    float a1 = 0.f, a2 = 0.f;
    if (act) {
      vload<T>(v, x + r * C + sub * W);
      vload<T>(g, dy + r * C + sub * W);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        v[j] = (v[j] - m) * rs;                      // xhat
        a1 += g[j] * gm[j]; a2 += g[j] * gm[j] * v[j];
        dg[j] += g[j] * v[j]; db[j] += g[j];
      }
    }
    a1 = group_sum<LPR>(a1); a2 = group_sum<LPR>(a2);
    if (act) {
#pragma unroll
      for (int j = 0; j < W; ++j) g[j] = rs * (g[j] * gm[j] - ic * (a1 + v[j] * a2));
      vstore<T>(dx + r * C + sub * W, g);
    }
  }
  if (act) {
#pragma unroll
    for (int j = 0; j < W; ++j) { atomicAdd(&sm[sub * W + j], dg[j]); atomicAdd(&sm[C + sub * W + j], db[j]); }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) { atomicAdd(&dgamma[c], sm[c]); atomicAdd(&dbeta[c], sm[C + c]); }
}

// block reduction per group for the vectorised GroupNorm kernels: thread t carries channel chunk (t % cv); first a strided
// tree over the 512/cv threads of each chunk, then the cv chunk sums are folded into their groups.  Result in red[g].
DEVI void vec_group_reduce(float v, int cv, int W, int Cg, int G, float* part, float* red) {
  __syncthreads();
  part[threadIdx.x] = v;
  __syncthreads();
  for (int stride = (int)blockDim.x >> 1; stride >= cv; stride >>= 1) {
    if ((int)threadIdx.x < stride) part[threadIdx.x] += part[threadIdx.x + stride];
    __syncthreads();
  }
  if ((int)threadIdx.x < G) {
    float s = 0.f;
    const int per = Cg / W;                                  // chunks per group
    for (int c = threadIdx.x * per; c < (threadIdx.x + 1) * per; ++c) s += part[c];
    red[threadIdx.x] = s;
  }
  __syncthreads();
}

// ---- GroupNorm, vectorised: 512-thread blocks; a thread's vectors all belong to one group and one channel chunk (requires
// 512 % (C/W) == 0 and (C/G) % W == 0)
// Two-pass moments of `rows` rows at xs, per group, with a fixed summation order: mean and M2 = sum (x - mean)^2 of the thread's group g;
// `writer`: the thread that stores its group's result (the first channel chunk of each group)
struct GnMoments { float mean, m2; int g; bool writer; };
template <typename T>
DEVI GnMoments groupnorm_moments(const T* xs, long rows, int C, int G) {
  constexpr int W = VT<T>::W;
  __shared__ float part[512];
  __shared__ float red[64];
  const int Cg = C / G, cv = C / W;
  const long nv = rows * cv;
  const int mych = (threadIdx.x % cv) * W;
  const int g = mych / Cg;
  const float cnt = (float)(rows * Cg);
  float acc = 0.f;
  for (long v = threadIdx.x; v < nv; v += blockDim.x) {
    float f[W];
    vload<T>(f, xs + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) acc += f[j];
  }
  vec_group_reduce(acc, cv, W, Cg, G, part, red);
  const float m = cnt > 0.f ? red[g] / cnt : 0.f;
  acc = 0.f;
  for (long v = threadIdx.x; v < nv; v += blockDim.x) {
    float f[W];
    vload<T>(f, xs + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) { const float d = f[j] - m; acc += d * d; }
  }
  vec_group_reduce(acc, cv, W, Cg, G, part, red);
  return {m, red[g], g, (int)threadIdx.x < cv && (mych % Cg) == 0};
}
// one block per sample
template <typename T>
__global__ __launch_bounds__(512) void groupnorm_stats_vec_kernel(float* mean, float* rstd, const T* x, long S, int C, int G, float eps) {
  const int n = blockIdx.x;
  const GnMoments r = groupnorm_moments<T>(x + (long)n * S * C, S, C, G);
  if (r.writer) {
    mean[(long)n * G + r.g] = r.mean;
    rstd[(long)n * G + r.g] = rsqrtf(r.m2 / (float)(S * (C / G)) + eps);
  }
}
// Small batches: one 512-thread block per sample leaves most of the chip idle (32 samples = 32 blocks).  Split each sample's
// rows over `parts` blocks: every block reduces its row range to per-group (mean, M2) with the same two-pass scheme, and a
// second kernel merges the partials in a fixed order (Chan et al.), so the result stays deterministic.
template <typename T>
__global__ __launch_bounds__(512) void groupnorm_part_stats_vec_kernel(float* ws, const T* x, long S, int C, int G, int parts) {
  const int n = blockIdx.x, pi = blockIdx.y;
  const long rpp = (S + parts - 1) / parts;
  const long r0 = min((long)pi * rpp, S), r1 = min(r0 + rpp, S);
  const GnMoments r = groupnorm_moments<T>(x + ((long)n * S + r0) * C, r1 - r0, C, G);
  if (r.writer) {
    float* o = ws + (((long)n * parts + pi) * G + r.g) * 2;
    o[0] = r.mean; o[1] = r.m2;
  }
}
__global__ void groupnorm_merge_kernel(float* mean, float* rstd, const float* ws, long S, int C, int G, int parts, float eps, long NG) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;      // (sample, group)
  if (i >= NG) return;
  const long n = i / G; const int g = (int)(i - n * G);
  const int Cg = C / G;
  const long rpp = (S + parts - 1) / parts;
  float cnt = 0.f, m = 0.f, M2 = 0.f;
  for (int pi = 0; pi < parts; ++pi) {
    const long r0 = min((long)pi * rpp, S), r1 = min(r0 + rpp, S);
    const float c2 = (float)((r1 - r0) * Cg);
    if (c2 <= 0.f) continue;
    const float* o = ws + ((n * parts + pi) * G + g) * 2;
    const float d = o[0] - m, tot = cnt + c2;
    m += d * (c2 / tot);
    M2 += o[1] + d * d * (cnt * c2 / tot);
    cnt = tot;
  }
  mean[i] = m;
  rstd[i] = rsqrtf(M2 / cnt + eps);
}

// (TD, WV: as in groupnorm_bwd_apply_vec_kernel)
template <typename T, typename TD = T, int WV = VT<T>::W>
__global__ __launch_bounds__(512) void groupnorm_bwd_stats_vec_kernel(float* s1, float* s2, float* dgamma, float* dbeta, const TD* dy,
                                                                     const T* x, const float* gamma, const float* beta, const float* mean,
                                                                     const float* rstd, long S, int C, int G, int act, int parts,
                                                                     const float* dyb, float dybs) {
  // dyb (or null): the incoming gradient is dyb[n][c] * dybs at every position (the backward of a mean over the positions) -- read from
  // the (N, C) tensor instead of a materialised broadcast
  constexpr int W = WV;
  __shared__ float part[512], part2[512];
  const int n = blockIdx.x, Cg = C / G, cv = C / W;
  // parts > 1 (small batches): blockIdx.y owns a row range and adds its sums into the pre-zeroed s1 / s2
  const long rpp = (S + parts - 1) / parts;
  const long r0 = min((long)blockIdx.y * rpp, S), r1 = min(r0 + rpp, S);
  const long base = ((long)n * S + r0) * C;
  const long nv = (r1 - r0) * cv;
  const int mych = (threadIdx.x % cv) * W;
  const int g = mych / Cg;
  const float m = mean[(long)n * G + g], rs = rstd[(long)n * G + g];
  float gm[W], bt[W], dg[W], db[W];
#pragma unroll
  for (int j = 0; j < W; ++j) { gm[j] = gamma[mych + j]; bt[j] = beta[mych + j]; dg[j] = 0.f; db[j] = 0.f; }
  float a1 = 0.f, a2 = 0.f;
  float gb[W];
#pragma unroll
  for (int j = 0; j < W; ++j) gb[j] = dyb ? dyb[(long)n * C + mych + j] * dybs : 0.f;
  for (long v = threadIdx.x; v < nv; v += blockDim.x) {
    float f[W], d[W];
    ldw<T, W>(f, x + base + v * W);
    if (dyb) {
#pragma unroll
      for (int j = 0; j < W; ++j) d[j] = gb[j];
    } else {
      ldw<TD, W>(d, dy + base + v * W);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float xh = gn_xhat(f[j], m, rs);
      const float dz = gn_dz(d[j], xh, gm[j], bt[j], act);
      a1 += dz * gm[j]; a2 += dz * gm[j] * xh;
      dg[j] += dz * xh; db[j] += dz;
    }
  }
  __shared__ float red[64];
  vec_group_reduce(a1, cv, W, Cg, G, part, red);
  if ((int)threadIdx.x < G) { if (parts > 1) atomicAdd(&s1[(long)n * G + threadIdx.x], red[threadIdx.x]); else s1[(long)n * G + threadIdx.x] = red[threadIdx.x]; }
  vec_group_reduce(a2, cv, W, Cg, G, part, red);
  if ((int)threadIdx.x < G) { if (parts > 1) atomicAdd(&s2[(long)n * G + threadIdx.x], red[threadIdx.x]); else s2[(long)n * G + threadIdx.x] = red[threadIdx.x]; }
  // per-channel partials: strided tree over the threads that share a channel chunk, then one global atomic per channel
#pragma unroll
  for (int j = 0; j < W; ++j) {
    __syncthreads();
    part[threadIdx.x] = dg[j]; part2[threadIdx.x] = db[j];
    __syncthreads();
    for (int stride = (int)blockDim.x >> 1; stride >= cv; stride >>= 1) {
      if ((int)threadIdx.x < stride) { part[threadIdx.x] += part[threadIdx.x + stride]; part2[threadIdx.x] += part2[threadIdx.x + stride]; }
      __syncthreads();
    }
    if ((int)threadIdx.x < cv) { atomicAdd(&dgamma[threadIdx.x * W + j], part[threadIdx.x]); atomicAdd(&dbeta[threadIdx.x * W + j], part2[threadIdx.x]); }
  }
}

// eight consecutive fp32 as two 16-byte loads (the router-trunk kernels: 8 channels per thread, next to one 16-byte bf16 access)
DEVI void ld8(float* f, const float* p) { vload<float>(f, p); vload<float>(f + 4, p + 4); }
// a = relu(y * scale[n][c] + shift[n][c]) as bf16 (scale == null: a plain fp32 -> bf16 conversion): the input of a router-trunk conv as the
// bf16 weight-gradient program reads it (the forward never materialises it: conv6s applies the same transform while it stages its tiles)
__global__ void gn1t_act_kernel(bf16* out, const float* y, const float* scale, const float* shift, long S, int C, long nvec) {
  const int cv = C / 8;
  GRID_STRIDE(v, nvec) {
    const long row = v / cv; const int c0 = (int)(v - row * cv) * 8;
    float f[8];
    ld8(f, y + v * 8);
    if (scale) {
      const long sc = (row / S) * C + c0;
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = fmaxf(f[j] * scale[sc + j] + shift[sc + j], 0.f);
    }
    vstore<bf16>(out + v * 8, f);
  }
}

template <typename T> static inline int lpr_for(int C) {
  const int nv = C / VT<T>::W;
  int l = 1;
  while (l < nv) l <<= 1;
  return l;
}
#define LPR_SWITCH(lpr, CALL)                         \
  switch (lpr) {                                      \
    case 1: { constexpr int L = 1; CALL; } break;     \
    case 2: { constexpr int L = 2; CALL; } break;     \
    case 4: { constexpr int L = 4; CALL; } break;     \
    case 8: { constexpr int L = 8; CALL; } break;     \
    case 16: { constexpr int L = 16; CALL; } break;   \
    case 32: { constexpr int L = 32; CALL; } break;   \
    default: { constexpr int L = 64; CALL; } break;   \
  }
template <typename T> static inline bool row_vec_ok(int C, const void* a, const void* b, const void* c, const void* d) {
  const int W = VT<T>::W;
  return C % W == 0 && C / W <= 64 && al16(a) && al16(b) && al16(c) && al16(d);
}
static inline unsigned rows_grid(long rows, int lpr, long cap) {
  long b = (rows * lpr + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}
// The arm of a row-norm entry point (dtype, C, rows, stream in scope; both kernels take the same arguments): VEC<T, LPR>, LPR lanes and
// 16-byte accesses per row, where the row length and the pointers a..d allow it, else SCALAR<T>, a thread per row.  At most vcap / scap
// workgroups; `lds` bytes of dynamic LDS
#define ROW_NORM_LAUNCH(VEC, SCALAR, vcap, scap, lds, a, b, c, d, ...)                                                                   \
  DT_SWITCH(dtype, if (row_vec_ok<T>(C, a, b, c, d)) {                                                                                   \
    const int lpr = lpr_for<T>(C);                                                                                                       \
    LPR_SWITCH(lpr, hipLaunchKernelGGL((VEC<T, L>), dim3(rows_grid(rows, lpr, vcap)), dim3(256), lds, stream, __VA_ARGS__))              \
  } else hipLaunchKernelGGL(SCALAR<T>, dim3(grid_for(rows, scap)), dim3(TPB), lds, stream, __VA_ARGS__))                                 \
  return hdmoe_launch_status();
// ---- GroupNorm(1, C) backward on SINGLE-POSITION rows (S == 1: the norms of the conditioning MLPs, (N, 512 or 1024) fp32).  The image
// kernels above run it as a statistics launch with one 512-thread workgroup per row -- two block reductions and 2 C global atomics per
// row, 39 us for 1 MB -- and an apply launch.  Here a wave owns a row: it holds the row in registers (NJ = ceil(C / 256) float4 pieces
// per lane), the two sums meet by cross-lane adds and dx is written at once, so a row's result depends on that row alone.  A workgroup
// takes GNR_ROWS rows; its per-channel dgamma / dbeta partials are added over the rows in registers, over the four waves in LDS in a
// fixed order, and leave as one atomic per channel and workgroup (N / 8 per address instead of N).
// The backward only: everything it writes ends in fp32 parameter gradients.  The forward of these rows stays on the two image kernels
// (5 us each): its output feeds the bf16 experts, and another summation order there moves the step's results (DESIGN Round 14).
constexpr int GNR_ROWS = 8;
template <int NJ>
__global__ __launch_bounds__(256) void groupnorm_rows_bwd_kernel(float* dx, float* dgamma, float* dbeta, const float* dy, const float* x,
                                                                const float* gamma, const float* beta, const float* mean,
                                                                const float* rstd, int N, int C, int act) {
  __shared__ __attribute__((aligned(16))) float sm[2][4][NJ * 256];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float invm = 1.f / (float)C;
  f32x4 gm[NJ], bt[NJ], dg[NJ], db[NJ];
  bool ok[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int c = 4 * (lane + 64 * j);
    ok[j] = c < C;
    gm[j] = ok[j] ? *reinterpret_cast<const f32x4*>(gamma + c) : (f32x4)(0.f);
    bt[j] = ok[j] ? *reinterpret_cast<const f32x4*>(beta + c) : (f32x4)(0.f);
    dg[j] = (f32x4)(0.f); db[j] = (f32x4)(0.f);
  }
  for (int k = wave; k < GNR_ROWS; k += 4) {
    const int n = blockIdx.x * GNR_ROWS + k;
    if (n >= N) break;
    const float m = mean[n], rs = rstd[n];
    f32x4 xh[NJ], dz[NJ];
    float a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const long at = (long)n * C + 4 * (lane + 64 * j);
      const f32x4 f = ok[j] ? *reinterpret_cast<const f32x4*>(x + at) : (f32x4)(0.f);
      const f32x4 d = ok[j] ? *reinterpret_cast<const f32x4*>(dy + at) : (f32x4)(0.f);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xh[j][e] = gn_xhat(f[e], m, rs);
        dz[j][e] = ok[j] ? gn_dz(d[e], xh[j][e], gm[j][e], bt[j][e], act) : 0.f;
        a1 += dz[j][e] * gm[j][e]; a2 += dz[j][e] * gm[j][e] * xh[j][e];
        dg[j][e] += dz[j][e] * xh[j][e]; db[j][e] += dz[j][e];
      }
    }
    a1 = wave_sum(a1); a2 = wave_sum(a2);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (!ok[j]) continue;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = gn_dx(dz[j][e], xh[j][e], rs, gm[j][e], invm, a1, a2);
      *reinterpret_cast<f32x4*>(dx + (long)n * C + 4 * (lane + 64 * j)) = o;
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    *reinterpret_cast<f32x4*>(&sm[0][wave][4 * (lane + 64 * j)]) = dg[j];
    *reinterpret_cast<f32x4*>(&sm[1][wave][4 * (lane + 64 * j)]) = db[j];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    atomicAdd(&dgamma[c], ((sm[0][0][c] + sm[0][1][c]) + sm[0][2][c]) + sm[0][3][c]);
    atomicAdd(&dbeta[c], ((sm[1][0][c] + sm[1][1][c]) + sm[1][2][c]) + sm[1][3][c]);
  }
}

template <typename T> static inline bool gn_vec_ok(int C, int G, const void* a, const void* b, const void* c) {
  const int W = VT<T>::W;
  if (C % W || (C / G) % W) return false;
  const int cv = C / W;
  return cv <= 512 && 512 % cv == 0 && al16(a) && al16(b) && al16(c);
}

// ---------------------------------------------------------------- GroupNorm(1, C) fused into the neighbouring convs (router trunks)
// Router.hard_route is conv -> GroupNorm(1, C) -> ReLU three times, then AdaptiveAvgPool2d(1) (reference model_components.py:100-112).
// The split-bf16 conv kernel leaves per-sample partial (sum, sum of squares) slots of its OUTPUT (conv6s_body.h); this kernel turns
// them into mean / rstd and the per-(sample, channel) affine  scale = gamma * rstd, shift = beta - mean * rstd * gamma  that the NEXT
// conv (and its weight gradient) apply to the tensor while staging it: the normalised activation is never written.
// The statistics of sample n from its slots, by every thread of the workgroup (`threads` of them): sm[0] = mean, sm[1] = rstd, also stored
// to mean[n] / rstd[n], then scale / shift [n][C]; sm is valid for all threads on return.
// wave 0: lane l takes slots l, l + 64, .. (independent loads), then a fixed-shape shuffle tree -- the order depends on `slots` only,
// never on the batch; fp64 for the few dozen partials (the cancellation in E[y^2] - mean^2)
DEVI void gn1_slot_stats(float* sm, float* scale, float* shift, float* mean, float* rstd, const float* ws, const float* gamma, const float* beta,
                         int n, int slots, int C, float inv_count, float eps, int threads) {
  double s1 = 0.0, s2 = 0.0;
  if (threadIdx.x < 64) {
    for (int k = threadIdx.x; k < slots; k += 64) {
      const float2 v = *reinterpret_cast<const float2*>(ws + ((long)n * slots + k) * 2);
      s1 += v.x; s2 += v.y;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { s1 += __shfl_down(s1, d, 64); s2 += __shfl_down(s2, d, 64); }
  }
  if (threadIdx.x == 0) {
    const double m = s1 * inv_count;
    double var = s2 * inv_count - m * m;
    if (var < 0.0) var = 0.0;
    sm[0] = (float)m; sm[1] = (float)(1.0 / sqrt(var + (double)eps));
    mean[n] = sm[0]; rstd[n] = sm[1];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += threads) {
    const float g = gamma[c] * sm[1];
    scale[(long)n * C + c] = g;
    shift[(long)n * C + c] = beta[c] - sm[0] * g;
  }
}
__global__ void gn1_finalize_kernel(float* scale, float* shift, float* mean, float* rstd, const float* ws, const float* gamma, const float* beta,
                                    int slots, int C, float inv_count, float eps) {
  __shared__ float sm[2];
  gn1_slot_stats(sm, scale, shift, mean, rstd, ws, gamma, beta, blockIdx.x, slots, C, inv_count, eps, blockDim.x);
}
// out[n][c] = mean over the S positions of relu(y[n][s][c] * scale[n][c] + shift[n][c]): the last GroupNorm + ReLU + average pool of the
// trunk in one read of y (fixed summation order)
constexpr int GN1_POOL_THREADS = 1024;                          // one block per sample: 16 waves keep enough 16-byte loads in flight
// ws != null: the statistics of y come as the producing conv's partial slots (the gn1_finalize step folded in: a launch less in the
// router's serial chain -- where a tiny kernel queues behind the other branch's persistent conv); scale / shift / mean / rstd are
// then OUTPUTS (kept for the backward).
// PQ (with ws): also pcnt[n][c] = the number of positions where the ReLU is open and qsum[n][c] = the sum of xh = (y - mean) * rstd over
// them -- everything the backward's statistics of this layer need, since its incoming gradient is g[n][c] / S at every position.  The mask
// is the backward's expression (act_grad_f of (y - mean) * rstd * gamma + beta), not y * scale + shift, so the two agree bit for bit.
template <bool PQ>
__global__ __launch_bounds__(GN1_POOL_THREADS) void gn1_relu_mean_kernel(float* out, const float* y, float* scale, float* shift, long S, int C,
                                                                       const float* ws, const float* gamma, const float* beta, float* mean,
                                                                       float* rstd, int slots, float inv_count, float eps, float* pcnt, float* qsum) {
  extern __shared__ float part[];                              // [threads / C4][C]
  __shared__ float smr[2];
  const int n = blockIdx.x, C4 = C / 4, rows = GN1_POOL_THREADS / C4;
  const int cq = threadIdx.x % C4, rw = threadIdx.x / C4;
  typedef __attribute__((ext_vector_type(4))) float f4;
  if (ws) gn1_slot_stats(smr, scale, shift, mean, rstd, ws, gamma, beta, n, slots, C, inv_count, eps, GN1_POOL_THREADS);
  f4 acc = (f4)(0.f), pc = (f4)(0.f), qc = (f4)(0.f);
  if (rw < rows) {
    f4 sc, sh, gm, bt;
    float m = 0.f, rs = 0.f;
    if (ws) {
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float g = gamma[4 * cq + e] * smr[1]; sc[e] = g; sh[e] = beta[4 * cq + e] - smr[0] * g; }
    } else {
      sc = *reinterpret_cast<const f4*>(scale + (long)n * C + 4 * cq); sh = *reinterpret_cast<const f4*>(shift + (long)n * C + 4 * cq);
    }
    if (PQ) {
      m = smr[0]; rs = smr[1];
#pragma unroll
      for (int e = 0; e < 4; ++e) { gm[e] = gamma[4 * cq + e]; bt[e] = beta[4 * cq + e]; }
    }
    // the ReLU-open count and sum of xh of one loaded vector (PQ only)
    auto pq = [&](const f4& v) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xh = gn_xhat(v[e], m, rs);
        const bool open = gn_dz(1.f, xh, gm[e], bt[e], 1) > 0.f;
        pc[e] += open ? 1.f : 0.f;
        qc[e] += open ? xh : 0.f;
      }
    };
    const float* yp = y + (long)n * S * C + 4 * cq;
    long s2 = rw;
    for (; s2 + 3 * rows < S; s2 += 4 * rows) {                 // four independent 16-byte loads in flight per thread (one block per sample:
      f4 v[4];                                                  //  the kernel lives on memory-level parallelism, not on occupancy)
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f4*>(yp + (s2 + (long)u * rows) * C);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += fmaxf(v[u][e] * sc[e] + sh[e], 0.f);
        if (PQ) pq(v[u]);
      }
    }
    for (; s2 < S; s2 += rows) {
      const f4 v = *reinterpret_cast<const f4*>(yp + s2 * C);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += fmaxf(v[e] * sc[e] + sh[e], 0.f);
      if (PQ) pq(v);
    }
    *reinterpret_cast<f4*>(part + (long)rw * C + 4 * cq) = acc;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += GN1_POOL_THREADS) {
    float t = 0.f;
    for (int k = 0; k < rows; ++k) t += part[(long)k * C + c];
    out[(long)n * C + c] = t / (float)S;
  }
  if (PQ) {                                                    // the same fixed-order reduction for the two extra sums
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      __syncthreads();
      if (rw < rows) *reinterpret_cast<f4*>(part + (long)rw * C + 4 * cq) = k2 ? qc : pc;
      __syncthreads();
      for (int c = threadIdx.x; c < C; c += GN1_POOL_THREADS) {
        float t = 0.f;
        for (int k = 0; k < rows; ++k) t += part[(long)k * C + c];
        (k2 ? qsum : pcnt)[(long)n * C + c] = t;
      }
    }
  }
}

// ---- router-trunk GroupNorm(1, C) + ReLU backward with bf16 gradients (ops._TrunkFn.backward on the streaming bf16 kernels).  Per layer
// at most two launches: gn1t_stats_kernel (none for the pooled last layer, whose sums come from the forward's pcnt / qsum) and
// gn1t_apply_kernel, which writes both bf16 operands of the conv's backward.  Every sum runs in an order fixed by S and C alone -- never by
// the other samples of the batch -- and none uses a float atomic.  8 channels per thread: 16-byte accesses to every tensor.
constexpr int GN1T_THREADS = 256;
// fixed-shape shuffle tree; the total lands in lane 0 ONLY (common.h's wave_sum leaves it in every lane)
DEVI float wave_sum0(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}
// One thread's rows r, r + R, r + 2 R, .. < r1: body(Rows<2>, r) takes the rows r and r + R together, so that the loads of both (up to six
// 16-byte accesses) are in flight at once, and body(Rows<1>, r) an odd last row
template <int K> struct Rows { static constexpr int n = K; };
template <typename F>
DEVI void gn1t_rows(long r, long r1, int R, F body) {
  for (; r + R < r1; r += 2 * R) body(Rows<2>{}, r);
  if (r < r1) body(Rows<1>{}, r);
}
// grid (N, parts): block (n, p) takes the rows [p * rpp, (p + 1) * rpp) of sample n; thread t the channels 8 (t % cv) .. + 7 of the rows
// t / cv + k * R (R = 256 / cv; threads past R * cv idle).  Writes ws[n][p][2] = the (s1, s2) partials, s1 = sum dz' gamma, s2 = sum dz' gamma xh,
// and wsc[k][c][n * parts + p] (k = 0: dgamma = sum dz' xh, k = 1: dbeta = sum dz'), channel-major so that the reduction reads them contiguously.
__global__ __launch_bounds__(GN1T_THREADS) void gn1t_stats_kernel(float* ws, float* wsc, const bf16* dz, const float* x, const float* gamma,
                                                                const float* beta, const float* mean, const float* rstd, long S, int C, int parts, long NP) {
  __shared__ float lds[2][GN1T_THREADS * 8];                    // [R][C] per-thread channel partials (R * C <= 2048)
  __shared__ float red[2][GN1T_THREADS / 64];
  const int n = blockIdx.x, p = blockIdx.y, cv = C / 8, R = GN1T_THREADS / cv;
  const int c0 = ((int)threadIdx.x % cv) * 8, rt = (int)threadIdx.x / cv;
  const long rpp = (S + parts - 1) / parts;
  const long r0 = min((long)p * rpp, S), r1 = min(r0 + rpp, S);
  const float m = mean[n], rs = rstd[n];
  float gm[8], bt[8], dg[8], db[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { gm[j] = gamma[c0 + j]; bt[j] = beta[c0 + j]; dg[j] = 0.f; db[j] = 0.f; }
  float a1 = 0.f, a2 = 0.f;
  if (rt < R) {
    const float* xp = x + (long)n * S * C + c0;
    const bf16* dp = dz + (long)n * S * C + c0;
    gn1t_rows(r0 + rt, r1, R, [&](auto rows, long r) {
      constexpr int K = decltype(rows)::n;
      float f[K][8], d[K][8];
#pragma unroll
      for (int k = 0; k < K; ++k) { ld8(f[k], xp + (r + k * R) * C); vload<bf16>(d[k], dp + (r + k * R) * C); }
#pragma unroll
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = gn_xhat(f[k][j], m, rs);
          const float dzz = gn_dz(d[k][j], xh, gm[j], bt[j], 1);
          a1 += dzz * gm[j]; a2 += dzz * gm[j] * xh;
          dg[j] += dzz * xh; db[j] += dzz;
        }
      }
    });
#pragma unroll
    for (int j = 0; j < 8; ++j) { lds[0][rt * C + c0 + j] = dg[j]; lds[1][rt * C + c0 + j] = db[j]; }
  }
  a1 = wave_sum0(a1); a2 = wave_sum0(a2);
  const int wv = threadIdx.x / 64;
  if (threadIdx.x % 64 == 0) { red[0][wv] = a1; red[1][wv] = a2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float u = 0.f, w = 0.f;
#pragma unroll
    for (int k = 0; k < GN1T_THREADS / 64; ++k) { u += red[0][k]; w += red[1][k]; }
    ws[((long)n * parts + p) * 2] = u; ws[((long)n * parts + p) * 2 + 1] = w;
  }
  for (int c = threadIdx.x; c < C; c += GN1T_THREADS) {
    float tg = 0.f, tb = 0.f;
    for (int k = 0; k < R; ++k) { tg += lds[0][k * C + c]; tb += lds[1][k * C + c]; }
    wsc[(long)c * NP + (long)n * parts + p] = tg; wsc[((long)C + c) * NP + (long)n * parts + p] = tb;
  }
}
// grid: N * P2 row-range blocks, then ceil(C / 4) channel blocks.
// Row-range block (n, p) first forms s1 / s2 of sample n: the sum of its `parts` statistics slots (dz given) or, for the pooled layer (g
// given: the incoming gradient is g[n][c] * gscale at every position), s1 = sum_c g gscale gamma pcnt[n][c] and s2 = the same with qsum.
// Every block of the sample runs the same code in the same order and gets the same bits.  Then, over its rows:
//   dx[n][s][c] = bf16(rstd (dz' gamma - (s1 + xh s2) / (S C))),  dz' = dz relu'(xh gamma + beta),  xh = (x - mean) rstd
//   a[n][s][i]  = bf16(relu(xin * scale[n][i] + shift[n][i]))     (scale == null: bf16(xin))  -- gn1t_act_kernel's arithmetic
// Channel block b: channels 4 b .. 4 b + 3, one wave each: dgamma[c] += the sum over (n, p) of the slots (or of g gscale qsum), dbeta likewise.
__global__ __launch_bounds__(GN1T_THREADS) void gn1t_apply_kernel(bf16* dx, bf16* a, float* dgamma, float* dbeta, const float* ws, const float* wsc,
                                                                int parts, const bf16* dz, const float* g, float gscale, const float* pcnt,
                                                                const float* qsum, const float* x, const float* gamma, const float* beta,
                                                                const float* mean, const float* rstd, const float* xin, const float* scale,
                                                                const float* shift, int N, long S, int C, int CI, int P2) {
  const int nrb = N * P2, lane = threadIdx.x % 64, wv = threadIdx.x / 64;
  if ((int)blockIdx.x >= nrb) {
    const int c = ((int)blockIdx.x - nrb) * (GN1T_THREADS / 64) + wv;
    if (c >= C) return;
    float sg = 0.f, sb = 0.f;
    if (g) {
      for (int i = lane; i < N; i += 64) {
        const float gs = g[(long)i * C + c] * gscale;
        sg += gs * qsum[(long)i * C + c]; sb += gs * pcnt[(long)i * C + c];
      }
    } else {
      const long NP = (long)N * parts;
      const float* pg = wsc + (long)c * NP;
      const float* pb = wsc + ((long)C + c) * NP;
#pragma unroll 4
      for (long i = lane; i < NP; i += 64) { sg += pg[i]; sb += pb[i]; }
    }
    sg = wave_sum0(sg); sb = wave_sum0(sb);
    if (lane == 0) { dgamma[c] += sg; dbeta[c] += sb; }
    return;
  }
  __shared__ float red[2][GN1T_THREADS / 64];
  __shared__ float su[2];
  const int n = blockIdx.x / P2, p = blockIdx.x % P2;
  if (g) {
    float u = 0.f, w = 0.f;
    for (int c = threadIdx.x; c < C; c += GN1T_THREADS) {
      const float gg = g[(long)n * C + c] * gscale * gamma[c];
      u += gg * pcnt[(long)n * C + c]; w += gg * qsum[(long)n * C + c];
    }
    u = wave_sum0(u); w = wave_sum0(w);
    if (lane == 0) { red[0][wv] = u; red[1][wv] = w; }
    __syncthreads();
    if (threadIdx.x == 0) {
      u = 0.f; w = 0.f;
#pragma unroll
      for (int k = 0; k < GN1T_THREADS / 64; ++k) { u += red[0][k]; w += red[1][k]; }
      su[0] = u; su[1] = w;
    }
  } else if (threadIdx.x == 0) {
    float u = 0.f, w = 0.f;
    for (int k = 0; k < parts; ++k) { u += ws[((long)n * parts + k) * 2]; w += ws[((long)n * parts + k) * 2 + 1]; }
    su[0] = u; su[1] = w;
  }
  __syncthreads();
  const long rpp = (S + P2 - 1) / P2;
  const long r0 = min((long)p * rpp, S), r1 = min(r0 + rpp, S);
  {                                                             // dx
    const int cv = C / 8, R = GN1T_THREADS / cv;
    const int c0 = ((int)threadIdx.x % cv) * 8, rt = (int)threadIdx.x / cv;
    const float m = mean[n], rs = rstd[n], u = su[0], w = su[1], invm = 1.f / (float)(S * C);
    float gm[8], bt[8], gd[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { gm[j] = gamma[c0 + j]; bt[j] = beta[c0 + j]; gd[j] = g ? g[(long)n * C + c0 + j] * gscale : 0.f; }
    auto out = [&](float* f, const float* d) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = gn_xhat(f[j], m, rs);
        f[j] = gn_dx(gn_dz(d[j], xh, gm[j], bt[j], 1), xh, rs, gm[j], invm, u, w);
      }
    };
    if (rt < R) {
      const float* xp = x + (long)n * S * C + c0;
      const bf16* dp = dz ? dz + (long)n * S * C + c0 : nullptr;
      bf16* op = dx + (long)n * S * C + c0;
      // gn1t_rows written out: this kernel sits at 96 VGPRs, the most that 5 waves per SIMD allow, and every form of this loop over the
      // helper (the branch on dp inside a row's lambda) took 98 to 116
      long r = r0 + rt;
      for (; r + R < r1; r += 2 * R) {
        float f0[8], f1[8], d0[8], d1[8];
        ld8(f0, xp + r * C); ld8(f1, xp + (r + R) * C);
        if (dp) { vload<bf16>(d0, dp + r * C); vload<bf16>(d1, dp + (r + R) * C); }
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) { d0[j] = gd[j]; d1[j] = gd[j]; }
        }
        out(f0, d0); out(f1, d1);
        vstore<bf16>(op + r * C, f0); vstore<bf16>(op + (r + R) * C, f1);
      }
      if (r < r1) {
        float f0[8], d0[8];
        ld8(f0, xp + r * C);
        if (dp) vload<bf16>(d0, dp + r * C);
        else {
#pragma unroll
          for (int j = 0; j < 8; ++j) d0[j] = gd[j];
        }
        out(f0, d0);
        vstore<bf16>(op + r * C, f0);
      }
    }
  }
  {                                                             // a
    const int cv = CI / 8, R = GN1T_THREADS / cv;
    const int c0 = ((int)threadIdx.x % cv) * 8, rt = (int)threadIdx.x / cv;
    float sc[8], sh[8];
    if (scale) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { sc[j] = scale[(long)n * CI + c0 + j]; sh[j] = shift[(long)n * CI + c0 + j]; }
    }
    if (rt < R) {
      const float* ip = xin + (long)n * S * CI + c0;
      bf16* op = a + (long)n * S * CI + c0;
      gn1t_rows(r0 + rt, r1, R, [&](auto rows, long r) {
        constexpr int K = decltype(rows)::n;
        float f[K][8];
#pragma unroll
        for (int k = 0; k < K; ++k) ld8(f[k], ip + (r + k * R) * CI);
        if (scale) {
#pragma unroll
          for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[k][j] = fmaxf(f[k][j] * sc[j] + sh[j], 0.f);
          }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) vstore<bf16>(op + (r + k * R) * CI, f[k]);
      });
    }
  }
}
static inline int gn1t_parts(long S) { const long p = S / 128; return (int)(p < 1 ? 1 : (p > 16 ? 16 : p)); }
}  // namespace

extern "C" {

int hdmoe_pixelnorm_fwd(void* xn, void* h, const void* x, long rows, int C, int dtype, hipStream_t stream) {
  ROW_NORM_LAUNCH(pixelnorm_fwd_vec_kernel, pixelnorm_fwd_kernel, 4096, 2048, 0, xn, h, x, nullptr, (T*)xn, (T*)h, (const T*)x, C, rows)
}
int hdmoe_pixelnorm_bwd(void* dx, const void* dxn, const void* dh, const void* x, long rows, int C, float sx, int dtype, hipStream_t stream) {
  if (!dxn && !dh) return HDMOE_EINVAL;
  ROW_NORM_LAUNCH(pixelnorm_bwd_vec_kernel, pixelnorm_bwd_kernel, 4096, 2048, 0, dx, dxn, dh, x, (T*)dx, (const T*)dxn, (const T*)dh, (const T*)x, C,
                  rows, sx)
}
static int gn_check(int N, int C, int G) {
  if (N < 1 || G < 1 || G > 64 || (G & (G - 1)) || C % G || C > 4096) return HDMOE_EINVAL;   // G must divide 512 (thread<->group map)
  return HDMOE_OK;
}
static int groupnorm_fwd_impl(void* y, float* mean, float* rstd, float* ws, int parts, const void* x, const float* gamma, const float* beta,
                              int N, long S, int C, int G, int act, float eps, int dtype, hipStream_t stream) {
  if (gn_check(N, C, G) || parts < 1 || parts > 64) return HDMOE_EINVAL;
  const long n = (long)N * S * C;
  DT_SWITCH(dtype, if (gn_vec_ok<T>(C, G, y, x, nullptr)) {
    const long nvec = n / VT<T>::W;
    if (ws && parts > 1) {
      hipLaunchKernelGGL(groupnorm_part_stats_vec_kernel<T>, dim3(N, parts), dim3(512), 0, stream, ws, (const T*)x, S, C, G, parts);
      hipLaunchKernelGGL(groupnorm_merge_kernel, dim3(cdiv((long)N * G, 64)), dim3(64), 0, stream, mean, rstd, ws, S, C, G, parts, eps, (long)N * G);
    } else {
      hipLaunchKernelGGL(groupnorm_stats_vec_kernel<T>, dim3(N), dim3(512), 0, stream, mean, rstd, (const T*)x, S, C, G, eps);
    }
    hipLaunchKernelGGL((groupnorm_apply_kernel<T, VT<T>::W>), dim3(grid_for(nvec)), dim3(TPB), 0, stream, (T*)y, (const T*)x, gamma, beta, mean, rstd, S, C, G, act, nvec);
    return hdmoe_launch_status();
  })
  DT_SWITCH(dtype, {
    hipLaunchKernelGGL(groupnorm_stats_kernel<T>, dim3(N), dim3(512), 0, stream, mean, rstd, (const T*)x, S, C, G, eps);
    hipLaunchKernelGGL((groupnorm_apply_kernel<T, 1>), dim3(grid_for(n)), dim3(TPB), 0, stream, (T*)y, (const T*)x, gamma, beta, mean, rstd, S, C, G, act, n);
  })
  return hdmoe_launch_status();
}
int hdmoe_groupnorm_fwd(void* y, float* mean, float* rstd, const void* x, const float* gamma, const float* beta, int N,
                        long S, int C, int G, int act, float eps, int dtype, hipStream_t stream) {
  return groupnorm_fwd_impl(y, mean, rstd, nullptr, 1, x, gamma, beta, N, S, C, G, act, eps, dtype, stream);
}
int hdmoe_groupnorm_fwd_split(void* y, float* mean, float* rstd, float* ws, int parts, const void* x, const float* gamma,
                              const float* beta, int N, long S, int C, int G, int act, float eps, int dtype, hipStream_t stream) {
  return groupnorm_fwd_impl(y, mean, rstd, ws, parts, x, gamma, beta, N, S, C, G, act, eps, dtype, stream);
}
// ws: 2*N*G floats of scratch; dgamma/dbeta accumulate (caller zeroes)
static int groupnorm_bwd_impl(void* dx, float* dgamma, float* dbeta, float* ws, int parts, const void* dy, const void* x, const float* gamma,
                              const float* beta, const float* mean, const float* rstd, int N, long S, int C, int G, int act,
                              int dtype, hipStream_t stream, const float* dyb = nullptr, float dybs = 1.f) {
  if (gn_check(N, C, G) || parts < 1 || parts > 64) return HDMOE_EINVAL;
  if (dyb && dy == nullptr) dy = x;                           // (only for the vector-path alignment check; never read)
  const long n = (long)N * S * C;
  float* s1 = ws; float* s2 = ws + (long)N * G;
  if (dtype == HDMOE_F32 && S == 1 && G == 1 && parts == 1 && !dyb && C % 4 == 0 && C <= 1024 && al16(dx) && al16(dy) && al16(x) &&
      al16(gamma) && al16(beta)) {                            // single-position rows: statistics and apply in one launch, a wave per row
#define GNR_LAUNCH(NJ) hipLaunchKernelGGL(groupnorm_rows_bwd_kernel<NJ>, dim3(cdiv(N, GNR_ROWS)), dim3(256), 0, stream, (float*)dx, dgamma, dbeta, \
                                          (const float*)dy, (const float*)x, gamma, beta, mean, rstd, N, C, act)
    switch ((C + 255) / 256) { case 1: GNR_LAUNCH(1); break; case 2: GNR_LAUNCH(2); break; case 3: GNR_LAUNCH(3); break; default: GNR_LAUNCH(4); break; }
#undef GNR_LAUNCH
    return hdmoe_launch_status();
  }
  DT_SWITCH(dtype, if (gn_vec_ok<T>(C, G, dx, dy, x)) {
    const long nvec = n / VT<T>::W;
    hipLaunchKernelGGL(groupnorm_bwd_stats_vec_kernel<T>, dim3(N, parts), dim3(512), 0, stream, s1, s2, dgamma, dbeta, (const T*)dy, (const T*)x,
                       gamma, beta, mean, rstd, S, C, G, act, parts, dyb, dybs);
    // 512, not 2048 blocks: this pass belongs to the router trunks' backward, which has slack, and a chip-filling grid of it holds up the
    // expert branch's kernels on the critical stream (same-box A/B 2048 -> 512: 15.52 -> 15.40 ms/step; the reverse experiment, four
    // row-range blocks per sample in the statistics pass, cost +0.4 ms)
    hipLaunchKernelGGL(groupnorm_bwd_apply_vec_kernel<T>, dim3(grid_for(nvec, 512)), dim3(TPB), 0, stream, (T*)dx, (const T*)dy,
                       (const T*)x, gamma, beta, mean, rstd, s1, s2, S, C, G, act, nvec, dyb, dybs);
    return hdmoe_launch_status();
  })
  if (dyb) return HDMOE_EINVAL;                               // the broadcast form exists for the vector kernels only
  DT_SWITCH(dtype, {
    hipLaunchKernelGGL(groupnorm_bwd_stats_kernel<T>, dim3(N), dim3(512), 2 * C * sizeof(float), stream, s1, s2, dgamma, dbeta,
                       (const T*)dy, (const T*)x, gamma, beta, mean, rstd, S, C, G, act);
    hipLaunchKernelGGL(groupnorm_bwd_apply_kernel<T>, dim3(grid_for(n)), dim3(TPB), 0, stream, (T*)dx, (const T*)dy, (const T*)x,
                       gamma, beta, mean, rstd, s1, s2, S, C, G, act, n);
  })
  return hdmoe_launch_status();
}
int hdmoe_groupnorm_bwd(void* dx, float* dgamma, float* dbeta, float* ws, const void* dy, const void* x, const float* gamma,
                        const float* beta, const float* mean, const float* rstd, int N, long S, int C, int G, int act,
                        int dtype, hipStream_t stream) {
  return groupnorm_bwd_impl(dx, dgamma, dbeta, ws, 1, dy, x, gamma, beta, mean, rstd, N, S, C, G, act, dtype, stream);
}
/* The same with the incoming gradient given as g[n][c] * scale at every position (backward of a mean over the S positions that follows
 * the norm): nothing of size N*S*C is read but x.  fp32 / bf16 vector shapes only (C % vector width == 0). */
int hdmoe_groupnorm_bwd_bcast(void* dx, float* dgamma, float* dbeta, float* ws, const float* g, float scale, const void* x,
                              const float* gamma, const float* beta, const float* mean, const float* rstd, int N, long S, int C, int G,
                              int act, int dtype, hipStream_t stream) {
  if (!g) return HDMOE_EINVAL;
  return groupnorm_bwd_impl(dx, dgamma, dbeta, ws, 1, nullptr, x, gamma, beta, mean, rstd, N, S, C, G, act, dtype, stream, g, scale);
}
/* parts > 1: ws (2*N*G floats) must be zeroed by the caller; the row-range blocks add into it */
int hdmoe_groupnorm_bwd_split(void* dx, float* dgamma, float* dbeta, float* ws, int parts, const void* dy, const void* x,
                              const float* gamma, const float* beta, const float* mean, const float* rstd, int N, long S, int C,
                              int G, int act, int dtype, hipStream_t stream) {
  return groupnorm_bwd_impl(dx, dgamma, dbeta, ws, parts, dy, x, gamma, beta, mean, rstd, N, S, C, G, act, dtype, stream);
}
/* Router-trunk backward in bf16 mode (GroupNorm(1, C) + ReLU; x = the conv output y_l, fp32): the incoming gradient dz is bf16 [N][S][C] (or, dz ==
 * null, g[n][c] * gscale at every position), the result dx is written as bf16 -- the operands of the bf16 dgrad / weight-gradient programs.
 * ws: 2 * N floats; dgamma / dbeta accumulate.  C % 4 == 0 and 512 % (C / 4) == 0. */
int hdmoe_gn1t_bwd(void* dx, float* dgamma, float* dbeta, float* ws, const void* dz, const float* g, float gscale, const float* x, const float* gamma,
                   const float* beta, const float* mean, const float* rstd, int N, long S, int C, hipStream_t stream) {
  if (!dx || !dgamma || !dbeta || !ws || !x || (!dz && !g) || gn_check(N, C, 1)) return HDMOE_EINVAL;
  // 4 channels per thread: 8-byte accesses to the bf16 tensors (measured against 8 channels with 16-byte accesses: 171 vs 214 us for stats
  // + apply at C = 128, 13.58 vs 13.93 ms/step)
  if (C % 4 || C / 4 > 512 || 512 % (C / 4) || ((uintptr_t)x & 15) || ((uintptr_t)dx & 15) || ((uintptr_t)dz & 15)) return HDMOE_EINVAL;
  const long nvec = (long)N * S * C / 4;
  float* s1 = ws; float* s2 = ws + N;
  hipLaunchKernelGGL((groupnorm_bwd_stats_vec_kernel<float, bf16, 4>), dim3(N, 1), dim3(512), 0, stream, s1, s2, dgamma, dbeta, (const bf16*)dz, x, gamma, beta,
                     mean, rstd, S, C, 1, 1, 1, dz ? nullptr : g, gscale);
  hipLaunchKernelGGL((groupnorm_bwd_apply_vec_kernel<float, bf16, 4>), dim3(grid_for(nvec, 512)), dim3(TPB), 0, stream, (bf16*)dx, (const bf16*)dz, x, gamma, beta, mean, rstd,
                     s1, s2, S, C, 1, 1, nvec, dz ? nullptr : g, gscale);
  return hdmoe_launch_status();
}
/* out (bf16 [N][S][C]) = relu(y * scale[n][c] + shift[n][c])  (scale == null: out = bf16(y)); C % 8 == 0 */
int hdmoe_gn1t_act(void* out, const float* y, const float* scale, const float* shift, int N, long S, int C, hipStream_t stream) {
  if (!out || !y || (scale == nullptr) != (shift == nullptr) || N < 1 || S < 1 || C % 8 || !al16(out) || !al16(y)) return HDMOE_EINVAL;
  const long nvec = (long)N * S * C / 8;
  hipLaunchKernelGGL(gn1t_act_kernel, dim3(grid_for(nvec, 1024)), dim3(TPB), 0, stream, (bf16*)out, y, scale, shift, S, C, nvec);
  return hdmoe_launch_status();
}
/* Floats of the statistics workspace of hdmoe_gn1t_stats: 2 N parts (s1 / s2 slots) + 2 C N parts (per-channel slots); parts a function of S. */
int hdmoe_gn1t_stats_floats(int N, long S, int C) {
  const long f = 2L * N * gn1t_parts(S) * (1 + (long)C);
  return f > 0x7fffffffL ? -1 : (int)f;
}
/* Router-trunk backward, bf16 mode, layers whose gradient dz (bf16 [N][S][C]) comes from the next conv: the GroupNorm(1, C) + ReLU backward sums
 * of every (sample, row range) into fixed slots of ws (hdmoe_gn1t_stats_floats floats).  x = the conv output y (fp32).  C % 8 == 0, C <= 2048. */
int hdmoe_gn1t_stats(float* ws, const void* dz, const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd, int N,
                     long S, int C, hipStream_t stream) {
  if (!ws || !dz || !x || !gamma || !beta || !mean || !rstd || N < 1 || S < 1 || C < 8 || C % 8 || C > 2048 || !al16(dz) || !al16(x)) return HDMOE_EINVAL;
  const int parts = gn1t_parts(S);
  const long NP = (long)N * parts;
  hipLaunchKernelGGL(gn1t_stats_kernel, dim3(N, parts), dim3(GN1T_THREADS), 0, stream, ws, ws + 2 * NP, (const bf16*)dz, x, gamma, beta, mean, rstd,
                     S, C, parts, NP);
  return hdmoe_launch_status();
}
/* ... and in one launch both bf16 operands of that layer's conv backward: dx = the GroupNorm(1, C) + ReLU input gradient (from dz and ws of
 * hdmoe_gn1t_stats, or -- dz == null, the pooled last layer -- from g[n][c] * gscale at every position and the forward's pcnt / qsum) and
 * a = relu(xin * scale[n][i] + shift[n][i]) ([N][S][CI]; scale == null: bf16(xin)), bit for bit what hdmoe_gn1t_act writes.  dgamma / dbeta
 * accumulate.  C, CI % 8 == 0 and <= 2048. */
int hdmoe_gn1t_apply(void* dx, void* a, float* dgamma, float* dbeta, const float* ws, const void* dz, const float* g, float gscale, const float* pcnt,
                     const float* qsum, const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd, const float* xin,
                     const float* scale, const float* shift, int N, long S, int C, int CI, hipStream_t stream) {
  if (!dx || !a || !dgamma || !dbeta || !x || !gamma || !beta || !mean || !rstd || !xin || (scale == nullptr) != (shift == nullptr)) return HDMOE_EINVAL;
  if (dz ? !ws : (!g || !pcnt || !qsum)) return HDMOE_EINVAL;
  if (N < 1 || S < 1 || C < 8 || C % 8 || C > 2048 || CI < 8 || CI % 8 || CI > 2048 || !al16(dx) || !al16(a) || !al16(dz) || !al16(x) || !al16(xin))
    return HDMOE_EINVAL;
  int P2 = (2048 + N - 1) / N;                                  // row ranges per sample: ~2048 row-range blocks (the results do not depend on it)
  if (P2 > S / 16) P2 = (int)(S / 16);
  if (P2 < 1) P2 = 1;
  const int parts = gn1t_parts(S);
  const long NP = (long)N * parts;
  const unsigned grid = (unsigned)(N * P2 + (C + GN1T_THREADS / 64 - 1) / (GN1T_THREADS / 64));
  hipLaunchKernelGGL(gn1t_apply_kernel, dim3(grid), dim3(GN1T_THREADS), 0, stream, (bf16*)dx, (bf16*)a, dgamma, dbeta, ws, dz ? ws + 2 * NP : nullptr,
                     parts, (const bf16*)dz, g, gscale, pcnt, qsum, x, gamma, beta, mean, rstd, xin, scale, shift, N, S, C, CI, P2);
  return hdmoe_launch_status();
}
int hdmoe_layernorm_fwd(void* y, float* mean, float* rstd, const void* x, const float* gamma, const float* beta, long rows,
                        int C, float eps, int dtype, hipStream_t stream) {
  ROW_NORM_LAUNCH(layernorm_fwd_vec_kernel, layernorm_fwd_kernel, 4096, 2048, 0, y, x, nullptr, nullptr, (T*)y, mean, rstd, (const T*)x, gamma, beta,
                  C, eps, rows)
}
int hdmoe_layernorm_bwd(void* dx, float* dgamma, float* dbeta, const void* dy, const void* x, const float* gamma,
                        const float* mean, const float* rstd, long rows, int C, int dtype, hipStream_t stream) {
  if (C > 4096) return HDMOE_EINVAL;
  ROW_NORM_LAUNCH(layernorm_bwd_vec_kernel, layernorm_bwd_kernel, 512, 256, 2 * C * sizeof(float), dx, dy, x, nullptr, (T*)dx, dgamma, dbeta,
                  (const T*)dy, (const T*)x, gamma, mean, rstd, C, rows)
}

/* partial slots [N][slots][2] of a conv output (hdmoe_conv_fwd_split_gn) -> mean / rstd [N] and scale / shift [N][C] of GroupNorm(1, C) */
int hdmoe_gn1_finalize(float* scale, float* shift, float* mean, float* rstd, const float* ws, const float* gamma, const float* beta, int N,
                       int slots, int C, long count, float eps, hipStream_t stream) {
  if (!scale || !shift || !mean || !rstd || !ws || !gamma || !beta || N < 1 || slots < 1 || C < 1 || count < 1) return HDMOE_EINVAL;
  hipLaunchKernelGGL(gn1_finalize_kernel, dim3(N), dim3(128), 0, stream, scale, shift, mean, rstd, ws, gamma, beta, slots, C, 1.f / (float)count, eps);
  return hdmoe_launch_status();
}
/* The three hdmoe_gn1_*relu_mean* forms: ws == null, scale / shift are inputs; else they, mean and rstd are written from the slots; pcnt (with
 * qsum) != null, the PQ kernel */
static int gn1_relu_mean_impl(float* out, float* scale, float* shift, float* mean, float* rstd, float* pcnt, float* qsum, const float* y, const float* ws,
                              const float* gamma, const float* beta, int N, int slots, long S, int C, float eps, hipStream_t stream) {
  if (!out || !y || !scale || !shift || N < 1 || S < 1 || C < 4 || C % 4 || C > 1024) return HDMOE_EINVAL;
  if (ws && (!mean || !rstd || !gamma || !beta || slots < 1)) return HDMOE_EINVAL;
  const int rows = GN1_POOL_THREADS / (C / 4);
  hipLaunchKernelGGL(pcnt ? gn1_relu_mean_kernel<true> : gn1_relu_mean_kernel<false>, dim3(N), dim3(GN1_POOL_THREADS), (size_t)rows * C * sizeof(float),
                     stream, out, y, scale, shift, S, C, ws, gamma, beta, mean, rstd, slots, ws ? 1.f / ((float)S * (float)C) : 0.f, ws ? eps : 0.f, pcnt, qsum);
  return hdmoe_launch_status();
}
/* out [N][C] = mean_s relu(y [N][S][C] * scale [N][C] + shift [N][C])   (fp32; C % 4 == 0, C <= 1024) */
int hdmoe_gn1_relu_mean(float* out, const float* y, const float* scale, const float* shift, int N, long S, int C, hipStream_t stream) {
  return gn1_relu_mean_impl(out, (float*)scale, (float*)shift, nullptr, nullptr, nullptr, nullptr, y, nullptr, nullptr, nullptr, N, 0, S, C, 0.f, stream);
}
/* hdmoe_gn1_finalize + hdmoe_gn1_relu_mean in one launch: statistics from the conv's partial slots ws [N][slots][2]; scale / shift [N][C] and
 * mean / rstd [N] are written (for the backward), out [N][C] = mean_s relu(GroupNorm(1, C)(y)). */
int hdmoe_gn1_finalize_relu_mean(float* out, float* scale, float* shift, float* mean, float* rstd, const float* y, const float* ws,
                                 const float* gamma, const float* beta, int N, int slots, long S, int C, float eps, hipStream_t stream) {
  if (!ws) return HDMOE_EINVAL;
  return gn1_relu_mean_impl(out, scale, shift, mean, rstd, nullptr, nullptr, y, ws, gamma, beta, N, slots, S, C, eps, stream);
}
/* The same, and pcnt / qsum [N][C] (fp32): per channel, the number of positions where the ReLU is open and the sum of the normalised value
 * (y - mean) * rstd over them -- the statistics hdmoe_gn1t_apply derives this layer's backward sums from when its gradient comes from the pool. */
int hdmoe_gn1_finalize_relu_mean_pq(float* out, float* scale, float* shift, float* mean, float* rstd, float* pcnt, float* qsum, const float* y,
                                    const float* ws, const float* gamma, const float* beta, int N, int slots, long S, int C, float eps, hipStream_t stream) {
  if (!ws || !pcnt || !qsum) return HDMOE_EINVAL;
  return gn1_relu_mean_impl(out, scale, shift, mean, rstd, pcnt, qsum, y, ws, gamma, beta, N, slots, S, C, eps, stream);
}

}  // extern "C"
