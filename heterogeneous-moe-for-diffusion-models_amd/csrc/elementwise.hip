// K4 / K7: HBM-bound pointwise, broadcast and relayout kernels of the HDMOE hot path (fwd + bwd).
// All activation tensors are NHWC / [rows][C]; "vector path" tensors ((B,F) embeddings, per-sample
// scalars) are always fp32.  Grid-stride loops, <= 2048 workgroups of 256 threads (guide G11).
#include "common.h"
#include "conv_args.h"
#include "hdmoe.h"

namespace {

constexpr int TPB = 256;

// Row window of a kernel over n = N * per work items (per items for each leading row): rows = DEVICE {begin, end} restricts the launch
// to the items [i0, i0 + n) of rows [begin, end), clamped to [0, N]; null leaves all n items.  The grid stays the all-rows one.
DEVI void row_window(const int* rows, long per, long& i0, long& n) {
  i0 = 0;
  if (!rows) return;
  const long N = per > 0 ? n / per : 0;
  long b = rows[0], e = rows[1];
  b = b < 0 ? 0 : (b > N ? N : b);
  e = e < b ? b : (e > N ? N : e);
  i0 = b * per; n = (e - b) * per;
}

// ---------------------------------------------------------------- generic pointwise
// Kernels written once over W lanes (ldw / stw, common.h) are instantiated at W = VT<T>::W, one 16-byte vector per thread, and at W = 1;
// they take their counts in elements and divide by W themselves, and L1D_W below picks the arm.
//
// f <- a f + b h, the rounding of hdmoe_axpby.  a x + b y has two roundings or three depending on which product is folded into a
// multiply-add; the rule, spelled out with contraction off so that no compiler chooses it, is per arm and per lane:
//   W == 1:  fma(b, y, round(a x))
//   W > 1:   fma(a, x, round(b y)) in lanes 0 .. W - 3, round(a x) + round(b y) in the last two
// (every mp_sum of the model goes through hdmoe_axpby: lanes that round alike would move the bits of all of them).  hdmoe_lerp_rows blends
// through the same function, so the two entry points agree bit for bit by construction; tests/test_sampler_guidance_interval.py compares
// them on every arm.
template <int W>
DEVI void axpby_lanes(float* f, const float* h, float a, float b) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < W; ++j) {
    const float p = b * h[j], q = a * f[j];
    if (W == 1) f[j] = __builtin_fmaf(b, h[j], q);
    else if (j < W - 2) f[j] = __builtin_fmaf(a, f[j], p);
    else f[j] = q + p;
  }
}
template <typename T, int W>
__global__ void axpby_kernel(T* out, const T* x, const T* y, float a, float b, long n) {
  GRID_STRIDE(v, n / W) {
    float f[W], g[W];
    ldw<T, W>(f, x + v * W);
    if (y) {
      ldw<T, W>(g, y + v * W);
      axpby_lanes<W>(f, g, a, b);
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j) f[j] = a * f[j];
    }
    stw<T, W>(out + v * W, f);
  }
}
template <typename T>
__global__ void affine_kernel(T* out, const T* x, float a, float c, long n) {
  GRID_STRIDE(i, n) out[i] = from_f<T>(a * to_f(x[i]) + c);
}
template <typename T>
__global__ void mul_kernel(T* out, const T* x, const T* y, long n) {
  GRID_STRIDE(i, n) out[i] = from_f<T>(to_f(x[i]) * to_f(y[i]));
}
template <typename TI, typename TO>
__global__ void cast_kernel(TO* out, const TI* x, long n) {
  GRID_STRIDE(i, n) out[i] = from_f<TO>(to_f(x[i]));
}
// fp16 exists at the module boundary only (`.half()` callers, reference tests/test_model/test_Unet_expert.py:106-115): converted to fp32
// at ingest and back at egress, the arithmetic in between is fp32 / bf16
__global__ void cast_h2f_kernel(float* out, const _Float16* x, long n) { GRID_STRIDE(i, n) out[i] = (float)x[i]; }
__global__ void cast_f2h_kernel(_Float16* out, const float* x, long n) { GRID_STRIDE(i, n) out[i] = (_Float16)x[i]; }
// Separable FIR resampling with an even-length filter f (resample(x, f, mode), reference model_internals.py:95-127), channel-last:
//   down: y[oy][ox] = scale * sum_{i,j} k[i] k[j] x[2 oy - pad + i][2 ox - pad + j]           (F.conv2d, stride 2, padding pad, depthwise)
//   up:   y[oy][ox] = scale * sum over (iy, i) with 2 iy - pad + i == oy (and likewise in x) of k[i] k[j] x[iy][ix]   (F.conv_transpose2d)
// each is the other's adjoint, so the same two kernels serve the backward passes (with the other one's scale).
// ---- EDM sampler, one Heun solver stage on the device (reference Utils/EDM_sampler.py:90-107): the sigma schedule t[0..N] (float64, as the
// host computes it) and the stage index live in device memory, so a captured hipGraph of a stage replays for every stage without host arithmetic
__global__ void sched_pick_kernel(float* sigma, const double* t, const int* idx, int off) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *sigma = (float)t[*idx + off];
}
__global__ void idx_advance_kernel(int* idx) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *idx += 1;
}
// (randn4 / ldw / stw / eps_w live in common.h: the training-input generator, csrc/traingen.hip, draws the same values)
// Philox key of sampler stage i: the key of hdmoe_randn(seed = *seed, *seed_dev = i).  Both words come from device memory, so a captured
// stage replays with the noise of the current call and stage.
DEVI void stage_key(const unsigned long long* seed, int i, uint32_t& lo, uint32_t& hi) {
  const unsigned long long s = *seed, c = (unsigned long long)i;
  lo = (uint32_t)s; hi = (uint32_t)(s >> 32);
  mix_seed(lo, hi, &c);
}
// Known region (inpainting) on its probability-flow path at sigma = s: x <- m (x0 + s noise) + (1 - m) x.  Evaluated in exactly this form
// (not as a lerp) so that m = 1 at s = 0 gives x0 and m = 0 gives x bit-for-bit.  Epilogue of the stage kernels, and the host-loop form.
template <typename T, int W> DEVI void known_blend_w(float* x, const T* x0, const T* nz, const float* m, float s, long off) {
#pragma clang fp contract(off)
  float a[W], z[W], k[W];
  ldw<T, W>(a, x0 + off); ldw<T, W>(z, nz + off); ldw<float, W>(k, m + off);
#pragma unroll
  for (int j = 0; j < W; ++j) x[j] = k[j] * (a[j] + s * z[j]) + (1.f - k[j]) * x[j];
}
// The update arithmetic is spelled out with contraction off, in the roundings of the earlier scalar kernels (euler: two products, one sum;
// correct: u = fma(a1, x_hat, b1 den), v = a2 x_next + b2 den2 unfused, u + v), so the result does not depend on how the compiler fuses it.
// x_next = x_hat + (t_next - t_hat) * (x_hat - denoised) / t_hat;  with x0 / nz / m (all or none): the known-region blend at t_next.
// t_hat = *that (the churned sigma heun_churn_kernel left on the device), or t[i] when that is NULL (no churn).
template <int W>
__global__ void heun_euler_kernel(float* xn, const float* xh, const float* den, const double* t, const int* idx, const double* that, long nv,
                                  const float* x0, const float* nz, const float* m) {
#pragma clang fp contract(off)
  const int i = *idx;
  const double th = that ? *that : t[i], h = t[i + 1] - th;
  const float a = (float)(1.0 + h / th), b = (float)(-h / th), s = (float)t[i + 1];
  GRID_STRIDE(v, nv) {
    float p[W], d[W];
    ldw<float, W>(p, xh + v * W); ldw<float, W>(d, den + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) p[j] = a * p[j] + b * d[j];
    if (m) known_blend_w<float, W>(p, x0, nz, m, s, v * W);
    stw<float, W>(xn + v * W, p);
  }
}
// x_out = x_hat + h * (0.5 * (x_hat - denoised) / t_hat + 0.5 * (x_next - denoised') / t_next);  x0 / nz / m: as heun_euler_kernel
template <int W>
__global__ void heun_correct_kernel(float* out, const float* xh, const float* den, const float* xn, const float* den2, const double* t, const int* idx,
                                    const double* that, long nv, const float* x0, const float* nz, const float* m) {
#pragma clang fp contract(off)
  const int i = *idx;
  const double th = that ? *that : t[i], tn = t[i + 1], h = tn - th;
  const float a1 = (float)(1.0 + 0.5 * h / th), b1 = (float)(-0.5 * h / th), a2 = (float)(0.5 * h / tn), b2 = (float)(-0.5 * h / tn);
  const float s = (float)tn;
  GRID_STRIDE(v, nv) {
    float p[W], d[W], q[W], d2[W];
    ldw<float, W>(p, xh + v * W); ldw<float, W>(d, den + v * W); ldw<float, W>(q, xn + v * W); ldw<float, W>(d2, den2 + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float u = __builtin_fmaf(a1, p[j], b1 * d[j]);
      const float w = a2 * q[j] + b2 * d2[j];
      p[j] = u + w;
    }
    if (m) known_blend_w<float, W>(p, x0, nz, m, s, v * W);
    stw<float, W>(out + v * W, p);
  }
}
// Churn of one Heun stage (reference Utils/EDM_sampler.py:90-97) on the device: i = *idx, tc = t[i], gamma = gcap inside [smin, smax] else 0,
// t_hat = tc + gamma tc -> *t_hat and (float) -> *sigma (what sched_pick(0) writes without churn), x_hat = x + c eps with
// c = (float)(sqrt(t_hat^2 - tc^2) snoise) and eps the stage's draw (stage_key / eps_w).  The scalars are computed in double exactly as the
// host loop computes them.  gamma == 0: nothing is drawn, x_hat = x bit-for-bit (no pass at all when in place).
template <int W>
__global__ void heun_churn_kernel(float* xh, const float* x, float* sigma, double* t_hat, const double* t, const int* idx,
                                  const unsigned long long* seed, double gcap, double smin, double smax, double snoise, long nv) {
#pragma clang fp contract(off)
  const int i = *idx;
  const double tc = t[i];
  const double gamma = (smin <= tc && tc <= smax) ? gcap : 0.0;
  const double th = tc + gamma * tc;
  if (blockIdx.x == 0 && threadIdx.x == 0) { *t_hat = th; *sigma = (float)th; }
  const bool noisy = gamma != 0.0;
  if (!noisy && xh == x) return;
  const float c = (float)(sqrt(th * th - tc * tc) * snoise);
  uint32_t lo = 0u, hi = 0u;
  if (noisy) stage_key(seed, i, lo, hi);
  GRID_STRIDE(v, nv) {
    float p[W];
    ldw<float, W>(p, x + v * W);
    if (noisy) {
      float e[W];
      eps_w<W>(e, v * W, lo, hi);
#pragma unroll
      for (int j = 0; j < W; ++j) p[j] = p[j] + c * e[j];
    }
    stw<float, W>(xh + v * W, p);
  }
}
// One DPM-Solver++(2M) stage (multistep, data prediction) on the same device schedule, one evaluation per stage: i = *idx, a = t[i+1] / t[i];
//   t[i+1] == 0:  x_out = den                                           (last stage)
//   i == *i0:     x_out = a x + (1 - a) den                             (no history yet: first order)
//   otherwise:    x_out = a x + (1 - a) ((1 + 1/(2r)) den - 1/(2r) den_prev),  r = log(t[i-1] / t[i]) / log(t[i] / t[i+1])
// then the known-region blend at s = t[i+1] (x0 / nz / m: as heun_euler_kernel), and den_prev <- den, each thread on its own elements (so a
// captured graph needs no ping-pong buffers).  Roundings, contraction off: a, b = 1 - a, w1 = 1 + 1/(2r), w0 = 1/(2r) are computed in double
// and rounded to float once; u = w1 den - w0 den_prev (two products, one difference), x_out = a x + b u (two products, one sum); first order
// a x + b den.  den_prev is read only by the second-order branch, x not at all by the last stage.
// SDE (DPM-Solver++(2M) SDE, midpoint form): with h = log(t[i] / t[i+1]) and e = exp(-eta h), a = (t[i+1] / t[i]) e and b = 1 - a replace
// the two above, and after the update (before the blend) x_out += c eps, c = (float)(t[i+1] sqrt(1 - e^2) snoise), eps the stage's draw
// (stage_key / eps_w) -- only when eta > 0 and not on the last stage.  eta == 0: e = 1, the deterministic stage bit-for-bit.
template <int W, bool SDE>
__global__ void dpm2m_step_kernel(float* xo, const float* x, const float* den, float* dp, const double* t, const int* idx, const int* i0, long nv,
                                  const float* x0, const float* nz, const float* m, float eta, float snoise, const unsigned long long* seed) {
#pragma clang fp contract(off)
  const int i = *idx;
  const double ti = t[i], tn = t[i + 1];
  const int order = tn == 0.0 ? 0 : (i <= *i0 ? 1 : 2);       // <=, not ==: an idx below i0 never reads t[i - 1]
  const double hr = order == 2 ? 0.5 * log(ti / tn) / log(t[i - 1] / ti) : 0.0;
  const double e = SDE && order != 0 ? exp(-(double)eta * log(ti / tn)) : 1.0, ad = tn / ti * e;
  const float a = (float)ad, b = (float)(1.0 - ad), w1 = (float)(1.0 + hr), w0 = (float)hr, s = (float)tn;
  const bool noisy = SDE && order != 0 && eta > 0.f;
  const float c = noisy ? (float)(tn * sqrt(1.0 - e * e) * (double)snoise) : 0.f;
  uint32_t lo = 0u, hi = 0u;
  if (noisy) stage_key(seed, i, lo, hi);
  GRID_STRIDE(v, nv) {
    float p[W], d[W];
    ldw<float, W>(d, den + v * W);
    if (order == 0) {
#pragma unroll
      for (int j = 0; j < W; ++j) p[j] = d[j];
    } else if (order == 1) {
      ldw<float, W>(p, x + v * W);
#pragma unroll
      for (int j = 0; j < W; ++j) p[j] = a * p[j] + b * d[j];
    } else {
      float q[W];
      ldw<float, W>(p, x + v * W); ldw<float, W>(q, dp + v * W);
#pragma unroll
      for (int j = 0; j < W; ++j) {
        const float u = w1 * d[j] - w0 * q[j];
        p[j] = a * p[j] + b * u;
      }
    }
    if (noisy) {
      float z[W];
      eps_w<W>(z, v * W, lo, hi);
#pragma unroll
      for (int j = 0; j < W; ++j) p[j] = p[j] + c * z[j];
    }
    if (m) known_blend_w<float, W>(p, x0, nz, m, s, v * W);
    stw<float, W>(dp + v * W, d);
    stw<float, W>(xo + v * W, p);
  }
}
// host-scalar form of the blend (host-driven sampler loop: churn or non-fp32 latents); x, x0, nz in T, m fp32.  The mask is fp32 whatever T
// is, so only <float, 4> has a 16-byte arm; bf16 latents take W = 1.
template <typename T, int W>
__global__ void known_blend_kernel(T* x, const T* x0, const T* nz, const float* m, float s, long n) {
  GRID_STRIDE(v, n / W) {
    float p[W];
    ldw<T, W>(p, x + v * W);
    known_blend_w<T, W>(p, x0, nz, m, s, v * W);
    stw<T, W>(x + v * W, p);
  }
}
struct FirTaps { float k[8]; };
template <typename T>
__global__ void fir_down_kernel(T* y, const T* x, FirTaps f, int L, int pad, float scale, int H, int W, int Ho, int Wo, int C, long total) {
  GRID_STRIDE(e, total) {
    const int c = (int)(e % C); long t = e / C;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho); const long n = t / Ho;
    float acc = 0.f;
    for (int i = 0; i < L; ++i) {
      const int iy = 2 * oy - pad + i;
      if ((unsigned)iy >= (unsigned)H) continue;
      for (int j = 0; j < L; ++j) {
        const int ix = 2 * ox - pad + j;
        if ((unsigned)ix >= (unsigned)W) continue;
        acc += f.k[i] * f.k[j] * to_f(x[((n * H + iy) * W + ix) * C + c]);
      }
    }
    y[e] = from_f<T>(scale * acc);
  }
}
template <typename T>
__global__ void fir_up_kernel(T* y, const T* x, FirTaps f, int L, int pad, float scale, int H, int W, int Ho, int Wo, int C, long total) {
  GRID_STRIDE(e, total) {                                    // (H, W): input size; (Ho, Wo): output size
    const int c = (int)(e % C); long t = e / C;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho); const long n = t / Ho;
    float acc = 0.f;
    for (int i = 0; i < L; ++i) {
      const int ty = oy + pad - i;
      if (ty < 0 || (ty & 1)) continue;
      const int iy = ty >> 1;
      if (iy >= H) continue;
      for (int j = 0; j < L; ++j) {
        const int tx = ox + pad - j;
        if (tx < 0 || (tx & 1)) continue;
        const int ix = tx >> 1;
        if (ix >= W) continue;
        acc += f.k[i] * f.k[j] * to_f(x[((n * H + iy) * W + ix) * C + c]);
      }
    }
    y[e] = from_f<T>(scale * acc);
  }
}
template <typename T, int W>
__global__ void mp_silu_fwd_kernel(T* out, const T* x, long n) {
  GRID_STRIDE(v, n / W) {
    float f[W];
    ldw<T, W>(f, x + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] = mp_silu_f(f[j]);
    stw<T, W>(out + v * W, f);
  }
}
template <typename T, int W>
__global__ void mp_silu_bwd_kernel(T* dx, const T* dy, const T* x, long n) {
  GRID_STRIDE(v, n / W) {
    float f[W], g[W];
    ldw<T, W>(f, x + v * W); ldw<T, W>(g, dy + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] = g[j] * mp_silu_grad_f(f[j]);
    stw<T, W>(dx + v * W, f);
  }
}
template <typename T>
__global__ void sigmoid_fwd_kernel(T* out, const T* x, float a, long n) {   // sigmoid(a*x)
  GRID_STRIDE(i, n) out[i] = from_f<T>(1.f / (1.f + __expf(-a * to_f(x[i]))));
}
template <typename T>
__global__ void sigmoid_bwd_kernel(T* dx, const T* dy, const T* y, float a, long n) {
  GRID_STRIDE(i, n) { const float s = to_f(y[i]); dx[i] = from_f<T>(to_f(dy[i]) * a * s * (1.f - s)); }
}

// (the counter RNG -- philox / u01 / mix_seed -- lives in common.h: the conv epilogue with fused FiLM + dropout draws the same bits)
__global__ void seed_advance_kernel(unsigned long long* seed_dev) { *seed_dev += 1ull; }

// ---------------------------------------------------------------- FiLM + mp_silu   (Unet_block, model_components.py:242-243)
// out = mp_silu(u * e[sample]), then F.dropout(p) fused (model_components.py:245-246).  A Philox block is four elements, so only the
// 16-byte arm draws: the W = 1 arm is reached with p == 0 only.
template <typename T, int W>
__global__ void film_silu_fwd_kernel(T* out, const T* u, const float* e, long HW, int C, long n, uint32_t seed_lo, uint32_t seed_hi,
                                     const unsigned long long* seed_dev, float p, unsigned char* mask = nullptr) {
  const int cv = C / W;
  const bool drop = W % 4 == 0 && p > 0.f;
  if (drop) mix_seed(seed_lo, seed_hi, seed_dev);
  const float inv = drop ? 1.f / (1.f - p) : 1.f;
  GRID_STRIDE(v, n / W) {
    const long row = v / cv; const int c0 = (int)(v - row * cv) * W;
    const float* ep = e + (row / HW) * C + c0;
    float f[W];
    ldw<T, W>(f, u + v * W);
    uint32_t r4[W];
    if constexpr (W % 4 == 0) {
      if (drop) {
#pragma unroll
        for (int q = 0; q < W / 4; ++q) { const long qi = (v * W) / 4 + q; philox((uint32_t)qi, (uint32_t)(qi >> 32), seed_lo, seed_hi, r4 + 4 * q); }
        if constexpr (W == 8) {
          if (mask) {                                        // the keep decisions for the backward: one byte per vector, bit j = element j kept
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < W; ++j) m |= (u01(r4[j]) >= p ? 1u : 0u) << j;
            mask[v] = (unsigned char)m;
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      float a = mp_silu_f(f[j] * ep[j]);
      if (drop) a = u01(r4[j]) >= p ? a * inv : 0.f;
      f[j] = a;
    }
    stw<T, W>(out + v * W, f);
  }
}
// one block per (pixel chunk, sample): du = da*silu'(u*e)*e ; de[n,c] += sum_pix da*silu'(u*e)*u
template <typename T>
__global__ void film_silu_bwd_kernel(T* du, float* de, const T* da, const T* u, const float* e, long HW, int C, int chunk) {
  extern __shared__ float sm[];
  const int s = blockIdx.y;
  for (int c = threadIdx.x; c < C; c += blockDim.x) sm[c] = 0.f;
  __syncthreads();
  const long p0 = (long)blockIdx.x * chunk;
  const long p1 = (p0 + chunk < HW) ? p0 + chunk : HW;
  const long base = (long)s * HW * C;
  for (long i = p0 * C + threadIdx.x; i < p1 * C; i += blockDim.x) {
    const int c = (int)(i % C);
    const float ev = e[(long)s * C + c], uv = to_f(u[base + i]);
    const float g = to_f(da[base + i]) * mp_silu_grad_f(uv * ev);
    du[base + i] = from_f<T>(g * ev);
    atomicAdd(&sm[c], g * uv);
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) atomicAdd(&de[(long)s * C + c], sm[c]);
}

// ---------------------------------------------------------------- per-sample scalar scale
template <typename T, int W>
__global__ void scale_rows_fwd_kernel(T* out, const T* x, const float* s, long L, long n) {
  const long Lv = L / W;
  GRID_STRIDE(v, n / W) {
    const float sv = s[v / Lv];
    float f[W];
    ldw<T, W>(f, x + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] *= sv;
    stw<T, W>(out + v * W, f);
  }
}
// block = (chunk of `chunk` W-wide items, row); the chunks of a row meet in ds through atomicAdd
template <typename T, int W>
__global__ void scale_rows_bwd_kernel(T* dx, float* ds, const T* dy, const T* x, const float* s, long L, int chunk) {
  __shared__ float sm[16];
  const int r = blockIdx.y;
  const long Lv = L / W;
  const long p0 = (long)blockIdx.x * chunk;
  const long p1 = (p0 + chunk < Lv) ? p0 + chunk : Lv;
  const float sv = s[r];
  float acc = 0.f;
  for (long i = p0 + threadIdx.x; i < p1; i += blockDim.x) {
    float g[W], xv[W];
    ldw<T, W>(g, dy + ((long)r * Lv + i) * W);
    if (ds) {
      ldw<T, W>(xv, x + ((long)r * Lv + i) * W);
#pragma unroll
      for (int j = 0; j < W; ++j) acc += g[j] * xv[j];
    }
    if (dx) {
#pragma unroll
      for (int j = 0; j < W; ++j) g[j] *= sv;
      stw<T, W>(dx + ((long)r * Lv + i) * W, g);
    }
  }
  if (ds) {
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) atomicAdd(&ds[r], acc);
  }
}

// ---------------------------------------------------------------- mp_cat  (model_internals.py:69-92)
// a thread owns W channels of one row: cva = Ca / W items of a row come from a, the other cv - cva from b
template <typename T, int W>
__global__ void cat2_fwd_kernel(T* out, const T* a, const T* b, float wa, float wb, int Ca, int Cb, long rows) {
  const int cva = Ca / W, cv = (Ca + Cb) / W;
  GRID_STRIDE(v, rows * cv) {
    const long r = v / cv; const int c = (int)(v - r * cv);
    float f[W];
    const bool first = c < cva;
    ldw<T, W>(f, first ? a + (r * cva + c) * W : b + (r * (cv - cva) + c - cva) * W);
    const float wgt = first ? wa : wb;
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] *= wgt;
    stw<T, W>(out + v * W, f);
  }
}
template <typename T, int W>
__global__ void cat2_bwd_kernel(T* da, T* db, const T* dout, float wa, float wb, int Ca, int Cb, long rows) {
  const int cva = Ca / W, cv = (Ca + Cb) / W;
  GRID_STRIDE(v, rows * cv) {
    const long r = v / cv; const int c = (int)(v - r * cv);
    float f[W];
    ldw<T, W>(f, dout + v * W);
    const bool first = c < cva;
    const float wgt = first ? wa : wb;
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] *= wgt;
    stw<T, W>(first ? da + (r * cva + c) * W : db + (r * (cv - cva) + c - cva) * W, f);
  }
}

// ---------------------------------------------------------------- resample (model_internals.py:95-127)
// one thread per W output channels (cv = C / W items a pixel), 32-bit index math per row
template <typename T, int W>   // out[n][h][w][c] = scale * sum_{2x2} x[n][2h+i][2w+j][c]
__global__ void pool2_kernel(T* out, const T* x, int Ho, int Wo, int C, float scale, long n) {
  const int cv = C / W;
  GRID_STRIDE(i, n / W) {
    const long row = i / ((long)Wo * cv);                      // (sample, output row)
    const int rem = (int)(i - row * ((long)Wo * cv));
    const int w = rem / cv, c = rem - w * cv;
    const T* p = x + ((row * 2) * (2 * Wo) + 2 * w) * (long)cv * W + (long)c * W;
    const long rs = (long)2 * Wo * cv * W;
    float a[W], b[W], d[W], e[W];
    ldw<T, W>(a, p); ldw<T, W>(b, p + (long)cv * W); ldw<T, W>(d, p + rs); ldw<T, W>(e, p + rs + (long)cv * W);
#pragma unroll
    for (int j = 0; j < W; ++j) a[j] = scale * (a[j] + b[j] + d[j] + e[j]);
    stw<T, W>(out + i * W, a);
  }
}
template <typename T, int W>   // out[n][h][w][c] = scale * x[n][h/2][w/2][c]
__global__ void upsample2_kernel(T* out, const T* x, int Ho, int Wo, int C, float scale, long n) {
  const int cv = C / W;
  GRID_STRIDE(i, n / W) {
    const long row = i / ((long)Wo * cv);                      // (sample, output row): sample = row / Ho, h = row % Ho
    const int rem = (int)(i - row * ((long)Wo * cv));
    const int w = rem / cv, c = rem - w * cv;
    const long s = row / Ho; const int h = (int)(row - s * Ho);
    float a[W];
    ldw<T, W>(a, x + (((s * (Ho / 2) + h / 2) * (Wo / 2) + w / 2) * (long)cv + c) * W);
#pragma unroll
    for (int j = 0; j < W; ++j) a[j] *= scale;
    stw<T, W>(out + i * W, a);
  }
}

// ---------------------------------------------------------------- sequence reduce / broadcast  ([N][S][C] <-> fp32 [N][C])
template <typename T>   // out = (x ? x : 0) + scale * t[n][c]
__global__ void seq_bcast_add_kernel(T* out, const T* x, const float* t, long S, int C, float scale, long n) {
  GRID_STRIDE(i, n) {
    const long row = i / C; const int c = (int)(i - row * C);
    const float v = scale * t[(row / S) * C + c];
    out[i] = from_f<T>(x ? to_f(x[i]) + v : v);
  }
}
// out[r][i] = x[r][i] + bias[i]   /   colsum: dbias[i] += sum_r dy[r][i]
template <typename T>
__global__ void bias_add_kernel(T* out, const T* x, const float* bias, long L, long n, const int* rows, long per) {
  long i0;
  row_window(rows, per, i0, n);                              // (per % L == 0)
  GRID_STRIDE(j, n) { const long i = i0 + j; out[i] = from_f<T>(to_f(x[i]) + bias[i % L]); }
}
template <typename T>
__global__ void colsum_kernel(float* out, const T* dy, long rows, long L, int rchunk, const int* win, long per) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  long rb;
  row_window(win, per, rb, rows);                            // matrix rows [rb, rb + rows) of the window (per matrix rows each)
  const long r0 = rb + (long)blockIdx.y * rchunk;
  const long r1 = (r0 + rchunk < rb + rows) ? r0 + rchunk : rb + rows;
  if (r0 >= r1) return;
  float acc = 0.f;
  for (long r = r0; r < r1; ++r) acc += to_f(dy[r * L + i]);
  atomicAdd(&out[i], acc);
}

// ---------------------------------------------------------------- lerp with a learnable scalar  (model_config2.py:291)
template <typename T>
__global__ void lerp_param_fwd_kernel(T* out, const T* a, const T* b, const float* alpha, long n) {
  const float al = *alpha;
  GRID_STRIDE(i, n) { const float av = to_f(a[i]); out[i] = from_f<T>(av + al * (to_f(b[i]) - av)); }
}
template <typename T, int W>
__global__ void lerp_param_bwd_kernel(T* da, T* db, float* dalpha, const T* g, const T* a, const T* b, const float* alpha, long n) {
  __shared__ float sm[16];
  const float al = *alpha;
  float acc = 0.f;
  GRID_STRIDE(v, n / W) {
    float gv[W], av[W], bv[W], o1[W], o2[W];
    ldw<T, W>(gv, g + v * W); ldw<T, W>(av, a + v * W); ldw<T, W>(bv, b + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) { o1[j] = (1.f - al) * gv[j]; o2[j] = al * gv[j]; acc += gv[j] * (bv[j] - av[j]); }
    stw<T, W>(da + v * W, o1); stw<T, W>(db + v * W, o2);
  }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) atomicAdd(dalpha, acc);
}

// ---------------------------------------------------------------- output gate  (model_config2.py:297-301)
// g = softmax(logits[.,2]); mixed = g0*U + g1*A; out = ((1-t)*U + t*mixed)/sqrt((1-t)^2+t^2), t = 0.5
template <typename T>
__global__ void gate_mix_fwd_kernel(T* out, float* gate, const T* logits, const T* U, const T* A, int C, long rows) {
  const float k = 0.70710678118654752f;   // 0.5 / sqrt(0.5)
  GRID_STRIDE(i, rows * C) {
    const long r = i / C; const int c = (int)(i - r * C);
    const float l0 = to_f(logits[2 * r]), l1 = to_f(logits[2 * r + 1]);
    const float m = fmaxf(l0, l1);
    const float e0 = __expf(l0 - m), e1 = __expf(l1 - m);
    const float g0 = e0 / (e0 + e1), g1 = e1 / (e0 + e1);
    if (c == 0) { gate[2 * r] = g0; gate[2 * r + 1] = g1; }
    const float u = to_f(U[i]), a = to_f(A[i]);
    out[i] = from_f<T>(k * (u + g0 * u + g1 * a));
  }
}
// one thread per pixel row
template <typename T>
__global__ void gate_mix_bwd_kernel(T* dU, T* dA, T* dlogits, const T* dout, const float* dgate, const float* gate,
                                    const T* U, const T* A, int C, long rows) {
  const float k = 0.70710678118654752f;
  GRID_STRIDE(r, rows) {
    const float g0 = gate[2 * r], g1 = gate[2 * r + 1];
    float d0 = dgate ? dgate[2 * r] : 0.f, d1 = dgate ? dgate[2 * r + 1] : 0.f;
    for (int c = 0; c < C; ++c) {
      const long i = r * C + c;
      const float go = k * to_f(dout[i]);
      const float u = to_f(U[i]), a = to_f(A[i]);
      dU[i] = from_f<T>(go * (1.f + g0));
      dA[i] = from_f<T>(go * g1);
      d0 += go * u; d1 += go * a;
    }
    const float dot = d0 * g0 + d1 * g1;
    dlogits[2 * r] = from_f<T>(g0 * (d0 - dot));
    dlogits[2 * r + 1] = from_f<T>(g1 * (d1 - dot));
  }
}

// 16-byte vector forms: LPR = C / W consecutive lanes own one pixel row (LPR a power of two <= 64, so rows never straddle a wave)
template <typename T>
__global__ void gate_mix_fwd_vec_kernel(T* out, float* gate, const T* logits, const T* U, const T* A, int lpr, long nvec) {
  constexpr int W = VT<T>::W;
  const float k = 0.70710678118654752f;
  GRID_STRIDE(v, nvec) {
    const long r = v / lpr;
    const float l0 = to_f(logits[2 * r]), l1 = to_f(logits[2 * r + 1]);
    const float m = fmaxf(l0, l1);
    const float e0 = __expf(l0 - m), e1 = __expf(l1 - m);
    const float g0 = e0 / (e0 + e1), g1 = e1 / (e0 + e1);
    if (v - r * lpr == 0) { gate[2 * r] = g0; gate[2 * r + 1] = g1; }
    float u[W], a[W];
    vload<T>(u, U + v * W); vload<T>(a, A + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) u[j] = k * (u[j] + g0 * u[j] + g1 * a[j]);
    vstore<T>(out + v * W, u);
  }
}
template <typename T>
__global__ void gate_mix_bwd_vec_kernel(T* dU, T* dA, T* dlogits, const T* dout, const float* dgate, const float* gate,
                                        const T* U, const T* A, int lpr, long nvec, long nvec_pad) {
  constexpr int W = VT<T>::W;
  const float k = 0.70710678118654752f;
  // nvec_pad is a multiple of 64: every lane of a wave takes part in the shuffles (tail lanes carry zeros)
  GRID_STRIDE(v, nvec_pad) {
    const long r = v / lpr;
    const bool ok = v < nvec;
    float g0 = 0.f, g1 = 0.f, d0 = 0.f, d1 = 0.f;
    if (ok) {
      g0 = gate[2 * r]; g1 = gate[2 * r + 1];
      float go[W], u[W], a[W];
      vload<T>(go, dout + v * W); vload<T>(u, U + v * W); vload<T>(a, A + v * W);
#pragma unroll
      for (int j = 0; j < W; ++j) { go[j] *= k; d0 += go[j] * u[j]; d1 += go[j] * a[j]; u[j] = go[j] * (1.f + g0); a[j] = go[j] * g1; }
      vstore<T>(dU + v * W, u); vstore<T>(dA + v * W, a);
    }
    for (int o = lpr >> 1; o > 0; o >>= 1) { d0 += __shfl_xor(d0, o, 64); d1 += __shfl_xor(d1, o, 64); }
    if (ok && v - r * lpr == 0) {
      if (dgate) { d0 += dgate[2 * r]; d1 += dgate[2 * r + 1]; }
      const float dot = d0 * g0 + d1 * g1;
      dlogits[2 * r] = from_f<T>(g0 * (d0 - dot));
      dlogits[2 * r + 1] = from_f<T>(g1 * (d1 - dot));
    }
  }
}

// ---------------------------------------------------------------- row softmax for tiny C (Scaling_router, model_components.py:64)
__global__ void softmax_rows_fwd_kernel(float* out, const float* x, int C, float scale, long rows) {
  GRID_STRIDE(r, rows) {
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, x[r * C + c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += __expf(x[r * C + c] - m);
    for (int c = 0; c < C; ++c) out[r * C + c] = scale * __expf(x[r * C + c] - m) / s;
  }
}
__global__ void softmax_rows_bwd_kernel(float* dx, const float* dy, const float* y, int C, float scale, long rows) {
  GRID_STRIDE(r, rows) {    // y = scale * p
    float dot = 0.f;
    for (int c = 0; c < C; ++c) dot += dy[r * C + c] * y[r * C + c];
    for (int c = 0; c < C; ++c) dx[r * C + c] = y[r * C + c] * (dy[r * C + c] - dot / scale);
  }
}

// ---------------------------------------------------------------- layout: NCHW fp32 <-> NHWC T with per-sample scale
template <typename T>   // out_nhwc[n][p][c] = s[n] * x_nchw[n][c][p]
__global__ void nchw_to_nhwc_kernel(T* out, const float* x, const float* s, int C, long HW, long n) {
  GRID_STRIDE(i, n) {
    long t = i; const int c = (int)(t % C); t /= C;
    const long p = t % HW; const long b = t / HW;
    const float v = x[(b * C + c) * HW + p];
    out[i] = from_f<T>(s ? v * s[b] : v);
  }
}
template <typename T>   // out_nchw = sf[n]*F_nhwc + (x ? sx[n]*x_nchw : 0)
__global__ void nhwc_to_nchw_kernel(float* out, const T* F, const float* sf, const float* x, const float* sx, int C, long HW, long n) {
  GRID_STRIDE(i, n) {
    long t = i; const long p = t % HW; t /= HW;
    const int c = (int)(t % C); const long b = t / C;
    float v = to_f(F[(b * HW + p) * C + c]);
    if (sf) v *= sf[b];
    if (x) v += (sx ? sx[b] : 1.f) * x[i];
    out[i] = v;
  }
}

// Guided egress: F holds the head output of a [conditional ; unconditional] stack of 2N rows (the second half starts `half` = N*HW*C
// elements in).  out_nchw[n] = sx[n]*x_nchw[n] + sf[n]*((1 - g)*F[N + n] + g*F[n]): the EDM egress above and the classifier-free-guidance
// lerp of the two denoiser outputs in one read of F and one write of out.  Written so that g == 1 reduces to the kernel above operation
// by operation (the lerp then returns F[n] exactly).
template <typename T>
__global__ void nhwc_to_nchw_guided_kernel(float* out, const T* F, const float* sf, const float* x, const float* sx, float g, int C, long HW,
                                           long n) {
  const float gu = 1.f - g;
  GRID_STRIDE(i, n) {
    long t = i; const long p = t % HW; t /= HW;
    const int c = (int)(t % C); const long b = t / C;
    const long f = (b * HW + p) * C + c;
    float v = gu * to_f(F[n + f]) + g * to_f(F[f]);
    if (sf) v *= sf[b];
    if (x) v += (sx ? sx[b] : 1.f) * x[i];
    out[i] = v;
  }
}
// The guided egress with one scale per sample, g[n] read from device memory (a batch that carries a sweep of scales; a scale that changes
// between replays of one captured graph).  The kernel above operation for operation with gu = 1 - g[b] taken per row: a constant vector
// reproduces it bit for bit.
template <typename T>
__global__ void nhwc_to_nchw_guided_rows_kernel(float* out, const T* F, const float* sf, const float* x, const float* sx, const float* g, int C,
                                                long HW, long n) {
  GRID_STRIDE(i, n) {
    long t = i; const long p = t % HW; t /= HW;
    const int c = (int)(t % C); const long b = t / C;
    const long f = (b * HW + p) * C + c;
    const float gb = g[b], gu = 1.f - gb;
    float v = gu * to_f(F[n + f]) + gb * to_f(F[f]);
    if (sf) v *= sf[b];
    if (x) v += (sx ? sx[b] : 1.f) * x[i];
    out[i] = v;
  }
}
// out[r][:] = (1 - g[r]) ref[r][:] + g[r] d[r][:]: the classifier-free-guidance blend of the two-pass path with one scale per sample.
// A constant vector gives the bits of hdmoe_axpby(ref, d, 1 - g, g), the blend of a float scale, on the same arm: both kernels round
// through axpby_lanes.  perv = per / W items in a row (per % W == 0 on the 16-byte arm, so no vector holds elements of two rows).
template <typename T, int W>
__global__ void lerp_rows_kernel(T* out, const T* ref, const T* d, const float* g, long per, long n) {
  const long perv = per / W;
  GRID_STRIDE(v, n / W) {
    const float b = g[v / perv], a = 1.f - b;
    float f[W], h[W];
    ldw<T, W>(f, ref + v * W);
    ldw<T, W>(h, d + v * W);
    axpby_lanes<W>(f, h, a, b);
    stw<T, W>(out + v * W, f);
  }
}

// ---------------------------------------------------------------- guidance combine: rescale + projected guidance (APG), hdmoe.h
// One workgroup of GC_TPB threads per sample.  Thread t owns the W-element vectors t, t + GC_TPB, ... of its sample.  Resident arm
// (RES, per <= GC_TPB * GC_R): the GC_R / W vectors of D_c and M stay in registers across the reduction, so ref / d / F / x and the
// momentum are read once and out and the momentum written once.  Re-read arm: the operands are read again after the reduction (from L2 for
// any sample that fits it) and M is formed a second time by the same fp32 operations, so both passes see the same M.  The five sums are
// fp64 per thread, then wave shuffle, then one LDS slot per wave and a second butterfly over the slots: no atomics, and every thread of the
// workgroup computes the same scalars.
constexpr int GC_TPB = 1024, GC_R = 16;
static_assert(GC_TPB * GC_R == HDMOE_GUIDE_COMBINE_RESIDENT, "the resident limit of hdmoe.h");
struct GcPar { float g; const float* g_rows; float eta, r, beta, phi; };
// the two loaders: D_c / D_u of elements e ... e + W - 1 of sample n
template <typename T> struct GcPair {                    // two-pass: ref = D_u, d = D_c, (B, per)
  const T* ref; const T* d;
  struct Cur {};
  template <int W> DEVI Cur seek(long) const { return {}; }
  DEVI void advance(Cur&) const {}
  DEVI void rewind(Cur&) const {}
  template <int W> DEVI void load(float* dc, float* du, long n, long per, long e, const Cur&) const {
    ldw<T, W>(dc, d + n * per + e);
    ldw<T, W>(du, ref + n * per + e);
  }
};
template <typename T> struct GcEgress {                  // shared-routing egress: sx x + sf F[n] and sx x + sf F[N + n], NCHW element e = c HW + p
  const T* F; const float* sf; const float* x; const float* sx; int C; unsigned HW; long half;       // per = C HW < 2^31: 32-bit division
  // (c, p) of a thread's current vector, carried from vector to vector by the step's quotient and remainder: one division per pass
  struct Cur { unsigned c, p, dq, dr; };
  template <int W> DEVI Cur seek(long e) const {
    const unsigned c = (unsigned)e / HW, step = GC_TPB * W;
    return {c, (unsigned)e - c * HW, step / HW, step % HW};
  }
  DEVI void advance(Cur& k) const {
    k.c += k.dq; k.p += k.dr;
    if (k.p >= HW) { k.p -= HW; ++k.c; }
  }
  DEVI void rewind(Cur& k) const { k.c = 0; k.p = 0; }     // element 0
  template <int W> DEVI void load(float* dc, float* du, long n, long per, long e, const Cur& k) const {
#pragma clang fp contract(off)
    const T* f = F + ((long)n * HW + k.p) * C + k.c;     // W > 1: HW % W == 0, the W elements share c
    const float a = sf[n], s = sx[n];
    float xs[W];
    ldw<float, W>(xs, x + n * per + e);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const float t = s * xs[j];
      dc[j] = t + a * to_f(f[(long)j * C]);
      du[j] = t + a * to_f(f[half + (long)j * C]);
    }
  }
};
template <int W> DEVI void gc_ldf(float* f, const float* p) {      // W floats: 16-byte loads, two of them at the bf16 width
  if constexpr (W == 8) { ldw<float, 4>(f, p); ldw<float, 4>(f + 4, p + 4); }
  else ldw<float, W>(f, p);
}
template <int W> DEVI void gc_stf(float* p, const float* f) {
  if constexpr (W == 8) { stw<float, 4>(p, f); stw<float, 4>(p + 4, f + 4); }
  else stw<float, W>(p, f);
}
// Composed guidance (hdmoe.h): the two loaders below put D_c = c_0 D_u + sum_k c_k D_k in front of the unchanged combine steps.  K is a
// run-time count; the coefficients are walked twice (c_0 first, then the sum) so that no array indexed by k has to live in registers.
// c_k of positions p ... p + W - 1: a[n][k], times the mask plane (n, k) -- mk, a uniform pointer, or null: no masks -- at p (one load:
// on the W > 1 arm HW % W == 0)
template <int W> DEVI void gc_coef(float* c, float ak, const float* mk, unsigned p) {
#pragma clang fp contract(off)
  if (mk) {
    float mv[W];
    gc_ldf<W>(mv, mk + p);
#pragma unroll
    for (int j = 0; j < W; ++j) c[j] = ak * mv[j];
  } else {
#pragma unroll
    for (int j = 0; j < W; ++j) c[j] = ak;
  }
}
// c_0 = (((1 - c_1) - c_2) - ...) - c_K;  an: a[n][0 .. K-1], mn: mask plane (n, 0), planes HW apart (or null), p: the vector's position
template <int W> DEVI void gc_coef0(float* c0, const float* an, const float* mn, int K, unsigned HW, unsigned p) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < W; ++j) c0[j] = 1.f;
#pragma nounroll                                          // K <= 8 at run time: a rolled loop, the resident arm holds 16 / W copies of it
  for (int k = 0; k < K; ++k) {
    float c[W];
    gc_coef<W>(c, an[k], mn ? mn + (long)k * HW : nullptr, p);
#pragma unroll
    for (int j = 0; j < W; ++j) c0[j] = c0[j] - c[j];
  }
}
template <typename T> struct GcCompose {                 // two-pass: ref = D_u, d[k] = D_{k+1}, (B, per) each; a (B, K); m (B, K, HW) or null, per = C HW
  const T* d[HDMOE_COMPOSE_MAX]; const T* ref; const float* a; const float* m; int K; unsigned HW;
  struct Cur { unsigned p, dr; };                        // p = e % HW of a thread's current vector (masks only), carried by the step's remainder
  template <int W> DEVI Cur seek(long e) const {
    if (!m) return {0u, 0u};
    return {(unsigned)(e % (long)HW), (unsigned)(((long)GC_TPB * W) % (long)HW)};
  }
  DEVI void advance(Cur& k) const {
    k.p += k.dr;
    if (k.p >= HW) k.p -= HW;
  }
  DEVI void rewind(Cur& k) const { k.p = 0; }
  template <int W> DEVI void load(float* dc, float* du, long n, long per, long e, const Cur& cur) const {
#pragma clang fp contract(off)
    const float* an = a + n * K;
    const float* mn = m ? m + n * K * (long)HW : nullptr;
    float c0[W];
    gc_coef0<W>(c0, an, mn, K, HW, cur.p);
    ldw<T, W>(du, ref + n * per + e);
#pragma unroll
    for (int j = 0; j < W; ++j) dc[j] = c0[j] * du[j];
#pragma nounroll
    for (int k = 0; k < K; ++k) {
      float c[W], dk[W];
      gc_coef<W>(c, an[k], mn ? mn + (long)k * HW : nullptr, cur.p);
      ldw<T, W>(dk, d[k] + n * per + e);
#pragma unroll
      for (int j = 0; j < W; ++j) dc[j] = dc[j] + c[j] * dk[j];
    }
    __builtin_amdgcn_sched_barrier(0);                   // the resident arm unrolls 16 / W of these k loops: keep them apart, or their loads pile up in registers
  }
};
template <typename T> struct GcComposeEgress {           // shared-routing egress of the variant-stacked F ((K + 1) N rows, the last N unconditional):
  GcEgress<T> eg; int K; const float* a; const float* m;      // D_k = sx x + sf F[k N + n], formed as GcEgress forms its pair; eg.half = N per
  using Cur = typename GcEgress<T>::Cur;
  template <int W> DEVI Cur seek(long e) const { return eg.template seek<W>(e); }
  DEVI void advance(Cur& k) const { eg.advance(k); }
  DEVI void rewind(Cur& k) const { eg.rewind(k); }
  template <int W> DEVI void load(float* dc, float* du, long n, long per, long e, const Cur& k) const {
#pragma clang fp contract(off)
    const T* f = eg.F + ((long)n * eg.HW + k.p) * eg.C + k.c;
    const float sf = eg.sf[n], s = eg.sx[n];
    const float* an = a + n * K;
    const float* mn = m ? m + n * K * (long)eg.HW : nullptr;
    float c0[W], t[W];
    gc_coef0<W>(c0, an, mn, K, eg.HW, k.p);
    ldw<float, W>(t, eg.x + n * per + e);
#pragma unroll
    for (int j = 0; j < W; ++j) {
      t[j] = s * t[j];
      du[j] = t[j] + sf * to_f(f[(long)K * eg.half + (long)j * eg.C]);
      dc[j] = c0[j] * du[j];
    }
#pragma nounroll
    for (int v = 0; v < K; ++v) {
      float c[W];
      gc_coef<W>(c, an[v], mn ? mn + (long)v * eg.HW : nullptr, k.p);
#pragma unroll
      for (int j = 0; j < W; ++j) dc[j] = dc[j] + c[j] * (t[j] + sf * to_f(f[(long)v * eg.half + (long)j * eg.C]));
    }
    __builtin_amdgcn_sched_barrier(0);                   // as in GcCompose
  }
};
template <typename L, typename TO, int W, bool RES, bool MOM>
__global__ __launch_bounds__(GC_TPB) void guide_combine_kernel(L ld, TO* out, float* mom, GcPar q, long per) {
#pragma clang fp contract(off)
  constexpr int K = RES ? GC_R / W : 1, NW = GC_TPB / 64;
  __shared__ double sm[5][NW];
  const long n = blockIdx.x, step = (long)GC_TPB * W, e0 = (long)threadIdx.x * W;
  float dc[K][W], m[K][W];
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  auto form = [&](float* dcv, float* mv, long e, const typename L::Cur& cur) {      // step 1 (fp32) of elements e ... e + W - 1
    float du[W];
    ld.template load<W>(dcv, du, n, per, e, cur);
    if constexpr (MOM) {
      float mp[W];
      gc_ldf<W>(mp, mom + n * per + e);
#pragma unroll
      for (int j = 0; j < W; ++j) mv[j] = (dcv[j] - du[j]) + q.beta * mp[j];
    } else {
#pragma unroll
      for (int j = 0; j < W; ++j) mv[j] = dcv[j] - du[j];
    }
  };
  auto sums = [&](const float* dcv, const float* mv) {    // step 2: the products of two fp32 values are exact in fp64
#pragma unroll
    for (int j = 0; j < W; ++j) {
      const double a = (double)mv[j], b = (double)dcv[j];
      s[0] = __builtin_fma(a, a, s[0]); s[1] = __builtin_fma(a, b, s[1]); s[2] = __builtin_fma(b, b, s[2]);
      s[3] += b; s[4] += a;
    }
  };
  typename L::Cur cur = ld.template seek<W>(e0);
  if constexpr (RES) {
#pragma unroll
    for (int k = 0; k < K; ++k) {                         // no branch: a vector past the end reads element 0 and counts as zeros
      const unsigned e = (unsigned)e0 + k * (unsigned)step;          // resident: offsets of 32 bits
      const bool ok = e < (unsigned)per;
      typename L::Cur at = cur;
      if (!ok) ld.rewind(at);
      form(dc[k], m[k], ok ? e : 0u, at);
#pragma unroll
      for (int j = 0; j < W; ++j) { dc[k][j] = ok ? dc[k][j] : 0.f; m[k][j] = ok ? m[k][j] : 0.f; }
      sums(dc[k], m[k]);
      ld.advance(cur);
    }
  } else {
    for (long e = e0; e < per; e += step) { form(dc[0], m[0], e, cur); sums(dc[0], m[0]); ld.advance(cur); }
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {                          // one branch after all five: a branch per sum lets the compiler sink the other
#pragma unroll                                            // sums' accumulation below it, with every element held as a double meanwhile
    for (int i = 0; i < 5; ++i) sm[i][threadIdx.x >> 6] = s[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 5; ++i) {                          // a butterfly over the NW slots: a + b == b + a, so every lane holds the same bits
    s[i] = sm[i][threadIdx.x & (NW - 1)];
#pragma unroll
    for (int o = NW / 2; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o, 64);
  }
  // steps 3 - 5 (fp64)
  const double S1 = s[0], S2 = s[1], S3 = s[2], T1 = s[3], T2 = s[4], cnt = (double)per;
  const double w1 = (double)(q.g_rows ? q.g_rows[n] : q.g) - 1.0, r = (double)q.r, phi = (double)q.phi;
  const double nrm = sqrt(S1), sc = nrm > r ? r / nrm : 1.0;
  const double c = S3 == 0.0 ? 0.0 : S2 / S3;
  const double b = w1 * sc, a = 1.0 - b * (1.0 - (double)q.eta) * c;
  const double so = a * T1 + b * T2, so2 = a * a * S3 + 2.0 * a * b * S2 + b * b * S1;
  const double varc = S3 - T1 * T1 / cnt, varo = so2 - so * so / cnt;
  const double rho = (varc <= 0.0 || varo <= 0.0) ? 1.0 : sqrt(varc / varo);
  const double f = phi * rho + (1.0 - phi);
  const float fa = (float)(f * a), fb = (float)(f * b);
  auto emit = [&](const float* dcv, const float* mv, long e) {      // step 6 (fp32), out rounded once
    float o[W];
#pragma unroll
    for (int j = 0; j < W; ++j) o[j] = fa * dcv[j] + fb * mv[j];
    if constexpr (MOM) gc_stf<W>(mom + n * per + e, mv);
    stw<TO, W>(out + n * per + e, o);
  };
  if constexpr (RES) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned e = (unsigned)e0 + k * (unsigned)step;
      if (e < (unsigned)per) emit(dc[k], m[k], e);
    }
  } else {
    cur = ld.template seek<W>(e0);
    for (long e = e0; e < per; e += step) { form(dc[0], m[0], e, cur); emit(dc[0], m[0], e); ld.advance(cur); }
  }
}

// ---------------------------------------------------------------- patch <-> image relayout (Vit_expert, model_components.py:698-704)
// tok[b][(hp,wp)][f] <-> img[b][hp*p+i][wp*p+j][c];  order 0: f = (i*p+j)*C + c ;  order 1 (PixelShuffle): f = c*p*p + i*p + j
template <typename T, bool TO_IMG>
__global__ void patch_relayout_kernel(T* out, const T* in, int H, int W, int C, int p, int hp, int wp, int order, long n, const int* rows) {
  // iterates over image elements of the *padded-free* image (H x W); tokens cover hp*p x wp*p
  long i0;
  row_window(rows, (long)H * W * C, i0, n);
  GRID_STRIDE(j, n) {
    const long i = i0 + j;
    long t = i; const int c = (int)(t % C); t /= C;
    const int x = (int)(t % W); t /= W;
    const int y = (int)(t % H); const long b = t / H;
    const int ph = y / p, ii = y % p, pw = x / p, jj = x % p;
    const int f = order ? c * p * p + ii * p + jj : (ii * p + jj) * C + c;
    const long tk = ((b * hp + ph) * wp + pw) * ((long)C * p * p) + f;
    if (TO_IMG) out[i] = in[tk];
    else out[tk] = in[i];
  }
}

// 16-byte version (C % (16 / sizeof(T)) == 0): one thread per 8- (bf16) / 4-channel (fp32) vector of an image pixel; the index
// arithmetic (five divisions by run-time values) is paid once per vector instead of once per element.  order 0: the token side is
// a 16-byte vector too; order 1 (PixelShuffle): the vector's channels sit p*p elements apart in the token.
template <typename T, bool TO_IMG>
__global__ void patch_relayout_vec_kernel(T* out, const T* in, int H, int W, int C, int p, int hp, int wp, int order, long nv, const int* rows) {
  constexpr int VW = VT<T>::W;
  const int CV = C / VW;
  long i0;
  row_window(rows, (long)H * W * CV, i0, nv);
  GRID_STRIDE(j, nv) {
    const long i = i0 + j;
    long t = i; const int c0 = (int)(t % CV) * VW; t /= CV;
    const int x = (int)(t % W); t /= W;
    const int y = (int)(t % H); const long b = t / H;
    const int ph = y / p, ii = y - ph * p, pw = x / p, jj = x - pw * p;
    const long tb = ((b * hp + ph) * wp + pw) * ((long)C * p * p);
    T* img = (TO_IMG ? out : const_cast<T*>(in)) + i * VW;
    if (order == 0) {
      T* tk = (TO_IMG ? const_cast<T*>(in) : out) + tb + (long)(ii * p + jj) * C + c0;
      if (TO_IMG) *reinterpret_cast<uint4*>(img) = *reinterpret_cast<const uint4*>(tk);
      else *reinterpret_cast<uint4*>(tk) = *reinterpret_cast<const uint4*>(img);
    } else {
      const int pp = p * p;
      T* tk = (TO_IMG ? const_cast<T*>(in) : out) + tb + (long)c0 * pp + ii * p + jj;
      alignas(16) T v[VW];
      if (TO_IMG) {
#pragma unroll
        for (int k = 0; k < VW; ++k) v[k] = tk[(long)k * pp];
        *reinterpret_cast<uint4*>(img) = *reinterpret_cast<const uint4*>(v);
      } else {
        *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(img);
#pragma unroll
        for (int k = 0; k < VW; ++k) tk[(long)k * pp] = v[k];
      }
    }
  }
}

// image -> tokens in PixelShuffle order (f = c*p*p + i*p + j) with the 16-byte vector on the TOKEN side: a thread owns VW consecutive j
// of one (token, c, i) and gathers them from VW neighbouring pixels (the image-side-vector form above scatters 2-byte stores p*p
// elements apart: 75 us for 67 MB; this form writes whole vectors).  Needs p % VW == 0.
template <typename T>
__global__ void patch_to_tokens_o1_vec_kernel(T* tok, const T* img, int H, int W, int C, int p, int hp, int wp, long nv, const int* rows) {
  constexpr int VW = VT<T>::W;
  const int jv = p / VW;                                     // vectors per (c, i) row of a token
  long v0;
  row_window(rows, (long)hp * wp * C * p * jv, v0, nv);
  GRID_STRIDE(j, nv) {
    const long v = v0 + j;
    long t = v;
    const int j0 = (int)(t % jv) * VW; t /= jv;
    const int ii = (int)(t % p); t /= p;
    const int c = (int)(t % C); t /= C;
    const int pw = (int)(t % wp); t /= wp;
    const int ph = (int)(t % hp); const long b = t / hp;
    const int y = ph * p + ii, x0 = pw * p + j0;
    alignas(16) T vals[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) vals[k] = (y < H && x0 + k < W) ? img[((b * H + y) * W + x0 + k) * C + c] : from_f<T>(0.f);
    *reinterpret_cast<uint4*>(tok + v * VW) = *reinterpret_cast<const uint4*>(vals);
  }
}

// ---------------------------------------------------------------- small vector-path kernels
__global__ void fourier_kernel(float* out, const float* x, const float* freqs, const float* phases, int F, long n) {
  GRID_STRIDE(i, n) {                                                  // model_internals.py:171-174
    const long b = i / F; const int f = (int)(i - b * F);
    out[i] = cosf(x[b] * freqs[f] + phases[f]) * 1.41421356237309515f;
  }
}
// EDM preconditioning coefficients (model_config2.py:431-438): coef[0..3][B] = c_skip, c_out, c_in, c_noise
__global__ void edm_coeffs_kernel(float* coef, const float* sigma, int nsig, float sd, int B) {
  GRID_STRIDE(b, B) {
    const float s = sigma[nsig == 1 ? 0 : b];
    const float q = s * s + sd * sd;
    coef[b] = sd * sd / q;
    coef[B + b] = s * sd / sqrtf(q);
    coef[2 * B + b] = 1.f / sqrtf(q);
    coef[3 * B + b] = logf(s) * 0.25f;
  }
}
// closed-form path scaling (model_config2.py:244-249): out[0][B]=s_vit, out[1][B]=s_unet, pair[B][2]
__global__ void sigmoid_scaling_kernel(float* sv, float* su, float* pair, const float* c_noise, float tp, float soft, int B) {
  GRID_STRIDE(b, B) {
    const float w = 1.f / (1.f + expf(-((c_noise[b] * 4.f - tp) / soft)));
    const float v = (w + 1e-2f) * 2.f, u = ((1.f - w) + 1e-2f) * 2.f;
    sv[b] = v; su[b] = u; pair[2 * b] = v; pair[2 * b + 1] = u;
  }
}



// ---------------------------------------------------------------- kernels with a 16-byte form only, or whose 16-byte form is another algorithm
// dx = gx + dy * silu'(x): the gradient of a tensor that feeds mp_silu AND a second consumer (residual / skip), in one pass
template <typename T>
__global__ void mp_silu_bwd_add_vec_kernel(T* dx, const T* dy, const T* x, const T* gx, float sx, long nv) {
  constexpr int W = VT<T>::W;
  GRID_STRIDE(v, nv) {
    float f[W], g[W], r[W];
    vload<T>(f, x + v * W); vload<T>(g, dy + v * W); vload<T>(r, gx + v * W);
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] = sx * r[j] + g[j] * mp_silu_grad_f(f[j]);
    vstore<T>(dx + v * W, f);
  }
}
// film_silu backward, 16-byte form: block = (pixel chunk, sample); a thread's vectors all carry the same channel chunk (256 % (C/W) == 0): register partials
template <typename T>
__global__ __launch_bounds__(256) void film_silu_bwd_vec_kernel(T* du, float* de, const T* da, const T* u, const float* e, long HW, int C, int chunk,
                                                               uint32_t seed_lo, uint32_t seed_hi, const unsigned long long* seed_dev, float p,
                                                               const unsigned char* mask = nullptr) {
  constexpr int W = VT<T>::W;
  extern __shared__ float sm[];
  if (p > 0.f) mix_seed(seed_lo, seed_hi, seed_dev);
  const float inv = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const int s = blockIdx.y, cv = C / W;
  for (int c = threadIdx.x; c < C; c += blockDim.x) sm[c] = 0.f;
  __syncthreads();
  const long p0 = (long)blockIdx.x * chunk;
  const long p1 = (p0 + chunk < HW) ? p0 + chunk : HW;
  const long base = (long)s * HW * C;
  const int c0 = (threadIdx.x % cv) * W;
  float ev[W], acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) { ev[j] = e[(long)s * C + c0 + j]; acc[j] = 0.f; }
  for (long v = p0 * cv + threadIdx.x; v < p1 * cv; v += 256) {
    float uv[W], g[W];
    vload<T>(uv, u + base + v * W); vload<T>(g, da + base + v * W);
    if (W == 8 && p > 0.f && mask) {                           // the forward saved its keep decisions (bit j of the vector's byte): no second draw
      const unsigned m = mask[(base + v * W) >> 3];
#pragma unroll
      for (int j = 0; j < W; ++j) g[j] = (m >> j) & 1u ? g[j] * inv : 0.f;
    } else if (p > 0.f) {
      uint32_t r4[W];
#pragma unroll
      for (int q = 0; q < W / 4; ++q) { const long qi = (base + v * W) / 4 + q; philox((uint32_t)qi, (uint32_t)(qi >> 32), seed_lo, seed_hi, r4 + 4 * q); }
#pragma unroll
      for (int j = 0; j < W; ++j) g[j] = u01(r4[j]) >= p ? g[j] * inv : 0.f;
    }
#pragma unroll
    for (int j = 0; j < W; ++j) {
      g[j] *= mp_silu_grad_f(uv[j] * ev[j]);
      acc[j] += g[j] * uv[j];
      g[j] *= ev[j];
    }
    vstore<T>(du + base + v * W, g);
  }
#pragma unroll
  for (int j = 0; j < W; ++j) atomicAdd(&sm[c0 + j], acc[j]);
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += blockDim.x) atomicAdd(&de[(long)s * C + c], sm[c]);
}
// mp_cat + mp_silu of the result in one pass (decoder blocks: the concatenation feeds mp_silu and the skip / residual path), and the
// matching backward: d(cat) = g_cat + g_h * silu'(cat), split and weighted
template <typename T>
__global__ void cat2_silu_fwd_vec_kernel(T* out, T* out_h, const T* a, const T* b, float wa, float wb, int Ca, int Cb, long rows) {
  constexpr int W = VT<T>::W;
  const int cva = Ca / W, cv = (Ca + Cb) / W;
  GRID_STRIDE(v, rows * cv) {
    const long r = v / cv; const int c = (int)(v - r * cv);
    float f[W];
    const bool first = c < cva;
    vload<T>(f, first ? a + (r * cva + c) * W : b + (r * (cv - cva) + c - cva) * W);
    const float wgt = first ? wa : wb;
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] *= wgt;
    vstore<T>(out + v * W, f);
    T tmp[W];
#pragma unroll
    for (int j = 0; j < W; ++j) tmp[j] = from_f<T>(f[j]);         // mp_silu sees the stored (rounded) value, like the two-kernel form
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] = mp_silu_f(to_f(tmp[j]));
    vstore<T>(out_h + v * W, f);
  }
}
template <typename T>
__global__ void cat2_silu_bwd_vec_kernel(T* da, T* db, const T* gcat, const T* gh, const T* xcat, float wa, float wb, int Ca, int Cb, long rows) {
  constexpr int W = VT<T>::W;
  const int cva = Ca / W, cv = (Ca + Cb) / W;
  GRID_STRIDE(v, rows * cv) {
    const long r = v / cv; const int c = (int)(v - r * cv);
    float f[W], g[W], x[W];
    vload<T>(g, gh + v * W); vload<T>(x, xcat + v * W);
    if (gcat) vload<T>(f, gcat + v * W);
    else {
#pragma unroll
      for (int j = 0; j < W; ++j) f[j] = 0.f;
    }
    const bool first = c < cva;
    const float wgt = first ? wa : wb;
#pragma unroll
    for (int j = 0; j < W; ++j) f[j] = (f[j] + g[j] * mp_silu_grad_f(x[j])) * wgt;
    vstore<T>(first ? da + (r * cva + c) * W : db + (r * (cv - cva) + c - cva) * W, f);
  }
}
// seq_reduce is deterministic (no atomics: the router's average pool feeds the top-k, and run-to-run float-add order would make the
// logits -- and through bf16 rounding every downstream tensor -- differ between identical calls).
// (a) one block per sample; thread (r, c) = (tid / cv, tid % cv) walks rows r, r + R, ... of its 16-byte channel chunk, then a
//     fixed-order tree over the R = 256 / cv row lanes.
template <typename T>
__global__ __launch_bounds__(256) void seq_reduce_det_vec_kernel(float* out, const T* x, long S, int C, float scale) {
  constexpr int W = VT<T>::W;
  extern __shared__ float sm[];                                // [R][C]
  const int n = blockIdx.x, cv = C / W, R = 256 / cv;
  const int r = threadIdx.x / cv, c0 = (threadIdx.x % cv) * W;
  const T* xs = x + (long)n * S * C;
  float acc[W];
#pragma unroll
  for (int j = 0; j < W; ++j) acc[j] = 0.f;
  for (long s0 = r; s0 < S; s0 += R) {
    float f[W];
    vload<T>(f, xs + s0 * C + c0);
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] += f[j];
  }
#pragma unroll
  for (int j = 0; j < W; ++j) sm[r * C + c0 + j] = acc[j];
  __syncthreads();
  for (int st = R >> 1; st >= 1; st >>= 1) {
    if (r < st) {
#pragma unroll
      for (int j = 0; j < W; ++j) sm[r * C + c0 + j] += sm[(r + st) * C + c0 + j];
    }
    __syncthreads();
  }
  if (r == 0) {
#pragma unroll
    for (int j = 0; j < W; ++j) out[(long)n * C + c0 + j] += scale * sm[c0 + j];
  }
}
// (b) any C: one thread per (sample, channel), four interleaved partial sums combined in a fixed order
template <typename T>
__global__ void seq_reduce_det_kernel(float* out, const T* x, long S, int C, float scale) {
  const int n = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const T* xs = x + (long)n * S * C + c;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  long s0 = 0;
  for (; s0 + 4 <= S; s0 += 4) {
    a0 += to_f(xs[s0 * C]); a1 += to_f(xs[(s0 + 1) * C]); a2 += to_f(xs[(s0 + 2) * C]); a3 += to_f(xs[(s0 + 3) * C]);
  }
  for (; s0 < S; ++s0) a0 += to_f(xs[s0 * C]);
  out[(long)n * C + c] += scale * ((a0 + a1) + (a2 + a3));
}
template <typename T> static inline bool chunk_fixed_ok(int C) {
  const int W = VT<T>::W;
  return C % W == 0 && C / W <= 256 && 256 % (C / W) == 0;
}

// ---------------------------------------------------------------- adaLN (Router, model_components.py:148-151): x*(1+gamma)+beta, cond = [gamma | beta]
__global__ void adaln_fwd_kernel(float* out, const float* x, const float* cond, int F, long n) {
  GRID_STRIDE(i, n) {
    const long b = i / F; const int f = (int)(i - b * F);
    out[i] = x[i] * (1.f + cond[b * 2 * F + f]) + cond[b * 2 * F + F + f];
  }
}
__global__ void adaln_bwd_kernel(float* dx, float* dcond, const float* g, const float* x, const float* cond, int F, long n) {
  GRID_STRIDE(i, n) {
    const long b = i / F; const int f = (int)(i - b * F);
    dx[i] = g[i] * (1.f + cond[b * 2 * F + f]);
    dcond[b * 2 * F + f] = g[i] * x[i];
    dcond[b * 2 * F + F + f] = g[i];
  }
}
// positive part of one column of the sparse gate matrix: out[b] = w[b][e] > 0 ? w[b][e] : 0   (NaN -> 0, as `mask = w > 0`)
__global__ void take_col_pos_fwd_kernel(float* out, const float* w, int E, int e, long B) {
  GRID_STRIDE(b, B) { const float v = w[b * E + e]; out[b] = v > 0.f ? v : 0.f; }
}
__global__ void take_col_pos_bwd_kernel(float* dw, const float* g, const float* w, int E, int e, long B) {
  GRID_STRIDE(b, B) { if (w[b * E + e] > 0.f) dw[b * E + e] = g[b]; }
}

// F.dropout(p): keep with prob 1-p, scale 1/(1-p); the mask is regenerated from (seed, element index) in bwd
template <typename T>
__global__ void dropout_kernel(T* out, const T* x, uint32_t seed_lo, uint32_t seed_hi, const unsigned long long* seed_dev, float p, long n) {
  mix_seed(seed_lo, seed_hi, seed_dev);
  const float inv = 1.f / (1.f - p);
  GRID_STRIDE(q, (n + 3) / 4) {
    uint32_t r[4];
    philox((uint32_t)q, (uint32_t)(q >> 32), seed_lo, seed_hi, r);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long i = q * 4 + j;
      if (i < n) out[i] = from_f<T>(u01(r[j]) >= p ? to_f(x[i]) * inv : 0.f);
    }
  }
}
__global__ void randn_kernel(float* out, uint32_t seed_lo, uint32_t seed_hi, const unsigned long long* seed_dev, float scale, long n) {
  mix_seed(seed_lo, seed_hi, seed_dev);
  GRID_STRIDE(q, (n + 3) / 4) {
    float v[4];
    randn4(q, seed_lo, seed_hi, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) if (q * 4 + j < n) out[q * 4 + j] = scale * v[j];
  }
}
// the same draws with the scale read from device memory: a captured launch follows a scale that changes between replays (the trainer's zeta)
__global__ void randn_ds_kernel(float* out, uint32_t seed_lo, uint32_t seed_hi, const unsigned long long* seed_dev, const float* scale, long n) {
  mix_seed(seed_lo, seed_hi, seed_dev);
  const float sc = *scale;
  GRID_STRIDE(q, (n + 3) / 4) {
    float v[4];
    randn4(q, seed_lo, seed_hi, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) if (q * 4 + j < n) out[q * 4 + j] = sc * v[j];
  }
}

// out = sum of up to 16 same-shaped tensors: the backward of a fan-out (a tensor consumed by n layers) in ONE pass -- autograd's own
// accumulation is n - 1 separate add launches over the same data
struct SumSrcs { const void* p[16]; float sc[16]; };
template <typename T>
__global__ void sum_n_kernel(T* out, SumSrcs s, int n, long nv, long nelem) {
  constexpr int W = VT<T>::W;
  GRID_STRIDE(v, nv) {
    if ((v + 1) * W <= nelem) {
      float f[W], g[W];
      vload<T>(f, (const T*)s.p[0] + v * W);
#pragma unroll
      for (int j = 0; j < W; ++j) f[j] *= s.sc[0];
      for (int k = 1; k < n; ++k) {
        vload<T>(g, (const T*)s.p[k] + v * W);
#pragma unroll
        for (int j = 0; j < W; ++j) f[j] += s.sc[k] * g[j];
      }
      vstore<T>(out + v * W, f);
    } else {
      for (long e = v * W; e < nelem; ++e) {
        float f = 0.f;
        for (int k = 0; k < n; ++k) f += s.sc[k] * to_f(((const T*)s.p[k])[e]);
        out[e] = from_f<T>(f);
      }
    }
  }
}

}  // namespace

// an entry point that ends in one dtype switch: the launch, then its status
#define DT_LAUNCH(dtype, ...) DT_SWITCH(dtype, __VA_ARGS__) return hdmoe_launch_status();

#define L1D(kernel, n, ...) hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(TPB), 0, stream, __VA_ARGS__)
// the two arms of a kernel<T, W> over n elements: 16-byte vectors when `vec_ok` (the count divides by VT<T>::W, the pointers are aligned), else W = 1
#define L1D_W(vec_ok, kernel, n, ...)                                   \
  if (vec_ok) L1D((kernel<T, VT<T>::W>), (n) / VT<T>::W, __VA_ARGS__);  \
  else L1D((kernel<T, 1>), n, __VA_ARGS__)

// Measurement aid (bench.py "attention", tools/exp_rate.py): issue rate of v_exp_f32, the instruction that bounds the attention kernels.
// Every thread runs 8 independent chains a = exp2(-a) (the negation is a source modifier: one v_exp_f32 per link), `iters` links each.
__global__ __launch_bounds__(256) void exp_rate_kernel(float* out, int iters) {
  float a[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] = 0.25f + 0.001f * (float)((threadIdx.x + k) & 63);
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = __builtin_amdgcn_exp2f(-a[k]);
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += a[k];
  out[(long)blockIdx.x * 256 + threadIdx.x] = s;
}

extern "C" {

int hdmoe_axpby(void* out, const void* x, const void* y, float a, float b, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, L1D_W(n % VT<T>::W == 0 && al16(out) && al16(x) && al16(y), axpby_kernel, n, (T*)out, (const T*)x, (const T*)y, a, b, n))
}
/* EDM sampler stage pieces (fp32 latents; t: device float64 schedule of N + 1 values, idx: device stage index) */
int hdmoe_sched_pick(float* sigma, const double* t, const int* idx, int off, hipStream_t stream) {
  if (!sigma || !t || !idx) return HDMOE_EINVAL;
  hipLaunchKernelGGL(sched_pick_kernel, dim3(1), dim3(64), 0, stream, sigma, t, idx, off);
  return hdmoe_launch_status();
}
int hdmoe_idx_advance(int* idx, hipStream_t stream) {
  if (!idx) return HDMOE_EINVAL;
  hipLaunchKernelGGL(idx_advance_kernel, dim3(1), dim3(64), 0, stream, idx);
  return hdmoe_launch_status();
}
// known-region operand block (x0, noise, mask): all NULL (no blend) or all set; the 16-byte path when every pointer allows it
static inline int known_block(const float* x0, const float* noise, const float* mask) {
  return (x0 == nullptr && noise == nullptr && mask == nullptr) ? 0 : (x0 && noise && mask) ? 1 : -1;
}
static int heun_euler_launch(float* xn, const float* xh, const float* den, const double* t, const int* idx, const double* t_hat, long n,
                             const float* x0, const float* noise, const float* mask, hipStream_t stream) {
  if (!xn || !xh || !den || !t || !idx || n < 0 || known_block(x0, noise, mask) < 0) return HDMOE_EINVAL;
  if (n % 4 == 0 && al16(xn) && al16(xh) && al16(den) && al16(x0) && al16(noise) && al16(mask))
    L1D(heun_euler_kernel<4>, n / 4, xn, xh, den, t, idx, t_hat, n / 4, x0, noise, mask);
  else
    L1D(heun_euler_kernel<1>, n, xn, xh, den, t, idx, t_hat, n, x0, noise, mask);
  return hdmoe_launch_status();
}
static int heun_correct_launch(float* out, const float* xh, const float* den, const float* xn, const float* den2, const double* t, const int* idx,
                               const double* t_hat, long n, const float* x0, const float* noise, const float* mask, hipStream_t stream) {
  if (!out || !xh || !den || !xn || !den2 || !t || !idx || n < 0 || known_block(x0, noise, mask) < 0) return HDMOE_EINVAL;
  if (n % 4 == 0 && al16(out) && al16(xh) && al16(den) && al16(xn) && al16(den2) && al16(x0) && al16(noise) && al16(mask))
    L1D(heun_correct_kernel<4>, n / 4, out, xh, den, xn, den2, t, idx, t_hat, n / 4, x0, noise, mask);
  else
    L1D(heun_correct_kernel<1>, n, out, xh, den, xn, den2, t, idx, t_hat, n, x0, noise, mask);
  return hdmoe_launch_status();
}
int hdmoe_heun_euler(float* xn, const float* xh, const float* den, const double* t, const int* idx, long n,
                     const float* x0, const float* noise, const float* mask, hipStream_t stream) {
  return heun_euler_launch(xn, xh, den, t, idx, nullptr, n, x0, noise, mask, stream);
}
int hdmoe_heun_correct(float* out, const float* xh, const float* den, const float* xn, const float* den2, const double* t, const int* idx, long n,
                       const float* x0, const float* noise, const float* mask, hipStream_t stream) {
  return heun_correct_launch(out, xh, den, xn, den2, t, idx, nullptr, n, x0, noise, mask, stream);
}
int hdmoe_heun_euler_hat(float* xn, const float* xh, const float* den, const double* t, const int* idx, const double* t_hat, long n,
                         const float* x0, const float* noise, const float* mask, hipStream_t stream) {
  if (!t_hat) return HDMOE_EINVAL;
  return heun_euler_launch(xn, xh, den, t, idx, t_hat, n, x0, noise, mask, stream);
}
int hdmoe_heun_correct_hat(float* out, const float* xh, const float* den, const float* xn, const float* den2, const double* t, const int* idx,
                           const double* t_hat, long n, const float* x0, const float* noise, const float* mask, hipStream_t stream) {
  if (!t_hat) return HDMOE_EINVAL;
  return heun_correct_launch(out, xh, den, xn, den2, t, idx, t_hat, n, x0, noise, mask, stream);
}
// finite and >= 0 (false for NaN)
static inline bool nonneg_finite(double v) { return v >= 0.0 && v <= 1.79769313486231570815e308; }
int hdmoe_heun_churn(float* x_hat, const float* x, float* sigma, double* t_hat, const double* t, const int* idx, const unsigned long long* seed,
                     double gamma_cap, double s_min, double s_max, double s_noise, long n, hipStream_t stream) {
  if (!x_hat || !x || !sigma || !t_hat || !t || !idx || !seed || n < 0) return HDMOE_EINVAL;
  if (!nonneg_finite(gamma_cap) || !nonneg_finite(s_noise) || s_min != s_min || s_max != s_max) return HDMOE_EINVAL;
  if (n % 4 == 0 && al16(x_hat) && al16(x))
    L1D(heun_churn_kernel<4>, n / 4, x_hat, x, sigma, t_hat, t, idx, seed, gamma_cap, s_min, s_max, s_noise, n / 4);
  else
    L1D(heun_churn_kernel<1>, n, x_hat, x, sigma, t_hat, t, idx, seed, gamma_cap, s_min, s_max, s_noise, n);
  return hdmoe_launch_status();
}
// do the n-float ranges at p and q share an element
static inline bool overlap(const float* p, const float* q, long n) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q, bytes = (uintptr_t)n * sizeof(float);
  return n > 0 && a < b + bytes && b < a + bytes;
}
static int dpm2m_launch(bool sde, float* x_out, const float* x, const float* den, float* den_prev, const double* t, const int* idx, const int* i0, long n,
                        const float* x0, const float* noise, const float* mask, float eta, float s_noise, const unsigned long long* seed,
                        hipStream_t stream) {
  if (!x_out || !x || !den || !den_prev || !t || !idx || !i0 || n < 0 || known_block(x0, noise, mask) < 0) return HDMOE_EINVAL;
  if (overlap(den_prev, den, n) || overlap(den_prev, x, n) || overlap(den_prev, x_out, n)) return HDMOE_EINVAL;
#define DPM2M(W, SDE, nv) L1D((dpm2m_step_kernel<W, SDE>), nv, x_out, x, den, den_prev, t, idx, i0, nv, x0, noise, mask, eta, s_noise, seed)
  if (n % 4 == 0 && al16(x_out) && al16(x) && al16(den) && al16(den_prev) && al16(x0) && al16(noise) && al16(mask)) {
    if (sde) DPM2M(4, true, n / 4); else DPM2M(4, false, n / 4);
  } else {
    if (sde) DPM2M(1, true, n); else DPM2M(1, false, n);
  }
#undef DPM2M
  return hdmoe_launch_status();
}
int hdmoe_dpm2m_step(float* x_out, const float* x, const float* den, float* den_prev, const double* t, const int* idx, const int* i0, long n,
                     const float* x0, const float* noise, const float* mask, hipStream_t stream) {
  return dpm2m_launch(false, x_out, x, den, den_prev, t, idx, i0, n, x0, noise, mask, 0.f, 0.f, nullptr, stream);
}
int hdmoe_dpm2m_sde_step(float* x_out, const float* x, const float* den, float* den_prev, const double* t, const int* idx, const int* i0, long n,
                         const float* x0, const float* noise, const float* mask, float eta, float s_noise, const unsigned long long* seed,
                         hipStream_t stream) {
  if (!seed || !nonneg_finite(eta) || !nonneg_finite(s_noise)) return HDMOE_EINVAL;
  return dpm2m_launch(true, x_out, x, den, den_prev, t, idx, i0, n, x0, noise, mask, eta, s_noise, seed, stream);
}
int hdmoe_known_blend(void* x, const void* x0, const void* noise, const float* mask, float s, long n, int dtype, hipStream_t stream) {
  if (!x || !x0 || !noise || !mask || n < 0) return HDMOE_EINVAL;
  if (dtype == HDMOE_F32 && n % 4 == 0 && al16(x) && al16(x0) && al16(noise) && al16(mask)) {
    L1D((known_blend_kernel<float, 4>), n / 4, (float*)x, (const float*)x0, (const float*)noise, mask, s, n);
    return hdmoe_launch_status();
  }
  DT_LAUNCH(dtype, L1D((known_blend_kernel<T, 1>), n, (T*)x, (const T*)x0, (const T*)noise, mask, s, n))
}
int hdmoe_exp_rate(float* out, int blocks, int iters, hipStream_t stream) {
  if (!out || blocks < 1 || iters < 1) return HDMOE_EINVAL;
  hipLaunchKernelGGL(exp_rate_kernel, dim3(blocks), dim3(256), 0, stream, out, iters);
  return hdmoe_launch_status();
}
int hdmoe_sum_n(void* out, const void* const* srcs, const float* src_scale, int n, long nelem, int dtype, hipStream_t stream) {
  if (!out || !srcs || n < 1 || n > 16) return HDMOE_EINVAL;
  SumSrcs s;
  bool al = al16(out);
  for (int k = 0; k < 16; ++k) { s.p[k] = srcs[k < n ? k : 0]; s.sc[k] = (src_scale && k < n) ? src_scale[k] : 1.f; al = al && al16(s.p[k]); }
  if (!al) return HDMOE_EINVAL;
  DT_LAUNCH(dtype, L1D(sum_n_kernel<T>, (nelem + VT<T>::W - 1) / VT<T>::W, (T*)out, s, n, (nelem + VT<T>::W - 1) / VT<T>::W, nelem))
}
int hdmoe_affine(void* out, const void* x, float a, float c, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, L1D(affine_kernel<T>, n, (T*)out, (const T*)x, a, c, n))
}
int hdmoe_mul(void* out, const void* x, const void* y, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, L1D(mul_kernel<T>, n, (T*)out, (const T*)x, (const T*)y, n))
}
int hdmoe_cast(void* out, const void* x, long n, int dt_in, int dt_out, hipStream_t stream) {
  if (dt_in == HDMOE_F32 && dt_out == HDMOE_BF16) L1D((cast_kernel<float, bf16>), n, (bf16*)out, (const float*)x, n);
  else if (dt_in == HDMOE_BF16 && dt_out == HDMOE_F32) L1D((cast_kernel<bf16, float>), n, (float*)out, (const bf16*)x, n);
  else if (dt_in == HDMOE_F32 && dt_out == HDMOE_F32) L1D((cast_kernel<float, float>), n, (float*)out, (const float*)x, n);
  else if (dt_in == HDMOE_BF16 && dt_out == HDMOE_BF16) L1D((cast_kernel<bf16, bf16>), n, (bf16*)out, (const bf16*)x, n);
  else if (dt_in == HDMOE_F16 && dt_out == HDMOE_F32) L1D(cast_h2f_kernel, n, (float*)out, (const _Float16*)x, n);
  else if (dt_in == HDMOE_F32 && dt_out == HDMOE_F16) L1D(cast_f2h_kernel, n, (_Float16*)out, (const float*)x, n);
  else return HDMOE_EDTYPE;
  return hdmoe_launch_status();
}
/* up == 0: y (N, Ho, Wo, C) = scale * stride-2 depthwise correlation of x (N, H, W, C) with outer(k, k), padding `pad`;
 * up == 1: the transposed operation (x is the small tensor).  taps: L <= 8 host floats (already normalised by the caller). */
int hdmoe_fir_resample(void* y, const void* x, const float* taps, int L, int pad, float scale, int up, int N, int H, int W, int Ho, int Wo, int C,
                       int dtype, hipStream_t stream) {
  if (!y || !x || !taps || L < 1 || L > 8 || pad < 0 || N < 0) return HDMOE_EINVAL;
  FirTaps f;
  for (int i = 0; i < 8; ++i) f.k[i] = i < L ? taps[i] : 0.f;
  const long total = (long)N * Ho * Wo * C;
  if (total == 0) return HDMOE_OK;
  DT_LAUNCH(dtype, if (up) L1D(fir_up_kernel<T>, total, (T*)y, (const T*)x, f, L, pad, scale, H, W, Ho, Wo, C, total);
                   else L1D(fir_down_kernel<T>, total, (T*)y, (const T*)x, f, L, pad, scale, H, W, Ho, Wo, C, total))
}
int hdmoe_mp_silu_fwd(void* out, const void* x, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, L1D_W(n % VT<T>::W == 0 && al16(out) && al16(x), mp_silu_fwd_kernel, n, (T*)out, (const T*)x, n))
}
int hdmoe_mp_silu_bwd(void* dx, const void* dy, const void* x, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, L1D_W(n % VT<T>::W == 0 && al16(dx) && al16(dy) && al16(x), mp_silu_bwd_kernel, n, (T*)dx, (const T*)dy, (const T*)x, n))
}
/* dx = sx * gx + dy * mp_silu'(x); 16-byte aligned, n % (16 / esz) == 0 */
int hdmoe_mp_silu_bwd_add(void* dx, const void* dy, const void* x, const void* gx, float sx, long n, int dtype, hipStream_t stream) {
  if (!dx || !dy || !x || !gx || !(al16(dx) && al16(dy) && al16(x) && al16(gx))) return HDMOE_EINVAL;
  DT_LAUNCH(dtype, if (n % VT<T>::W == 0) L1D(mp_silu_bwd_add_vec_kernel<T>, n / VT<T>::W, (T*)dx, (const T*)dy, (const T*)x, (const T*)gx, sx, n / VT<T>::W);
                   else return HDMOE_EINVAL)
}
/* out = mp_cat(a, b) (weights wa, wb), out_h = mp_silu(out); Ca, Cb multiples of 16 / esz */
int hdmoe_cat2_silu_fwd(void* out, void* out_h, const void* a, const void* b, float wa, float wb, int Ca, int Cb, long rows, int dtype,
                        hipStream_t stream) {
  if (!(al16(out) && al16(out_h) && al16(a) && al16(b)) || !out || !out_h) return HDMOE_EINVAL;
  DT_LAUNCH(dtype, if (Ca % VT<T>::W == 0 && Cb % VT<T>::W == 0)
                     L1D(cat2_silu_fwd_vec_kernel<T>, rows * (Ca + Cb) / VT<T>::W, (T*)out, (T*)out_h, (const T*)a, (const T*)b, wa, wb, Ca, Cb, rows);
                   else return HDMOE_EINVAL)
}
/* (da, db) = split((gcat + gh * mp_silu'(xcat)) * (wa | wb)); gcat may be NULL */
int hdmoe_cat2_silu_bwd(void* da, void* db, const void* gcat, const void* gh, const void* xcat, float wa, float wb, int Ca, int Cb,
                        long rows, int dtype, hipStream_t stream) {
  if (!(al16(da) && al16(db) && al16(gcat) && al16(gh) && al16(xcat)) || !gh || !xcat) return HDMOE_EINVAL;
  DT_LAUNCH(dtype, if (Ca % VT<T>::W == 0 && Cb % VT<T>::W == 0)
                     L1D(cat2_silu_bwd_vec_kernel<T>, rows * (Ca + Cb) / VT<T>::W, (T*)da, (T*)db, (const T*)gcat, (const T*)gh, (const T*)xcat, wa, wb, Ca, Cb, rows);
                   else return HDMOE_EINVAL)
}
int hdmoe_sigmoid_fwd(void* out, const void* x, float a, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, L1D(sigmoid_fwd_kernel<T>, n, (T*)out, (const T*)x, a, n))
}
int hdmoe_sigmoid_bwd(void* dx, const void* dy, const void* y, float a, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, L1D(sigmoid_bwd_kernel<T>, n, (T*)dx, (const T*)dy, (const T*)y, a, n))
}
int hdmoe_film_silu_fwd(void* out, const void* u, const float* e, int N, long HW, int C, int dtype, hipStream_t stream) {
  const long n = (long)N * HW * C;
  DT_LAUNCH(dtype, L1D_W(C % VT<T>::W == 0 && al16(out) && al16(u), film_silu_fwd_kernel, n, (T*)out, (const T*)u, e, HW, C, n, 0u, 0u, nullptr, 0.f))
}
// FiLM + mp_silu + F.dropout in one pass (vectorised layouts only: C % (16/sizeof(T)) == 0)
int hdmoe_film_silu_drop_fwd(void* out, const void* u, const float* e, int N, long HW, int C, unsigned long long seed,
                             const unsigned long long* seed_dev, float p, int dtype, hipStream_t stream) {
  const long n = (long)N * HW * C;
  if (p < 0.f || p >= 1.f) return HDMOE_EINVAL;
  DT_LAUNCH(dtype, if (C % VT<T>::W == 0 && al16(out) && al16(u)) L1D((film_silu_fwd_kernel<T, VT<T>::W>), n / VT<T>::W, (T*)out, (const T*)u, e, HW, C, n,
                                                                     (uint32_t)seed, (uint32_t)(seed >> 32), seed_dev, p);
                   else return HDMOE_EINVAL)
}
int hdmoe_film_silu_drop_bwd(void* du, float* de, const void* da, const void* u, const float* e, int N, long HW, int C,
                             unsigned long long seed, const unsigned long long* seed_dev, float p, int dtype, hipStream_t stream) {
  if (N > 65535 || p < 0.f || p >= 1.f) return HDMOE_EINVAL;
  const int chunk = 256;
  dim3 grid(cdiv(HW, chunk), N);
  DT_LAUNCH(dtype, if (chunk_fixed_ok<T>(C) && al16(du) && al16(da) && al16(u))
                     hipLaunchKernelGGL(film_silu_bwd_vec_kernel<T>, grid, dim3(TPB), C * sizeof(float), stream, (T*)du, de, (const T*)da, (const T*)u, e, HW, C, chunk,
                                        (uint32_t)seed, (uint32_t)(seed >> 32), seed_dev, p);
                   else return HDMOE_EINVAL)
}
/* hdmoe_film_silu_drop_fwd that also saves the keep decisions (bf16 only): mask [N][HW][C/8] bytes, bit j of a byte = element j of the
 * 16-byte vector is kept.  `out` is bit-identical to hdmoe_film_silu_drop_fwd's. */
int hdmoe_film_silu_drop_fwd_mask(void* out, unsigned char* mask, const void* u, const float* e, int N, long HW, int C, unsigned long long seed,
                                  const unsigned long long* seed_dev, float p, int dtype, hipStream_t stream) {
  const long n = (long)N * HW * C;
  if (p <= 0.f || p >= 1.f || dtype != HDMOE_BF16 || !mask || C % 8 || !al16(out) || !al16(u)) return HDMOE_EINVAL;
  L1D((film_silu_fwd_kernel<bf16, 8>), n / 8, (bf16*)out, (const bf16*)u, e, HW, C, n, (uint32_t)seed, (uint32_t)(seed >> 32), seed_dev, p, mask);
  return hdmoe_launch_status();
}
/* hdmoe_film_silu_drop_bwd from the saved mask instead of a second Philox draw (bf16 only; de accumulates).  du is bit-identical. */
int hdmoe_film_silu_mask_bwd(void* du, float* de, const void* da, const void* u, const float* e, const unsigned char* mask, int N, long HW, int C,
                             float p, int dtype, hipStream_t stream) {
  if (N > 65535 || p <= 0.f || p >= 1.f || dtype != HDMOE_BF16 || !mask) return HDMOE_EINVAL;
  const int chunk = 256;
  dim3 grid(cdiv(HW, chunk), N);
  if (!(chunk_fixed_ok<bf16>(C) && al16(du) && al16(da) && al16(u))) return HDMOE_EINVAL;
  hipLaunchKernelGGL(film_silu_bwd_vec_kernel<bf16>, grid, dim3(TPB), C * sizeof(float), stream, (bf16*)du, de, (const bf16*)da, (const bf16*)u, e, HW, C, chunk,
                     0u, 0u, nullptr, p, mask);
  return hdmoe_launch_status();
}
int hdmoe_film_silu_bwd(void* du, float* de, const void* da, const void* u, const float* e, int N, long HW, int C,
                        int dtype, hipStream_t stream) {
  if (N > 65535) return HDMOE_EINVAL;
  const int chunk = 256;
  dim3 grid(cdiv(HW, chunk), N);
  DT_LAUNCH(dtype, if (chunk_fixed_ok<T>(C) && al16(du) && al16(da) && al16(u))
                     hipLaunchKernelGGL(film_silu_bwd_vec_kernel<T>, grid, dim3(TPB), C * sizeof(float), stream, (T*)du, de, (const T*)da, (const T*)u, e, HW, C, chunk, 0u, 0u, nullptr, 0.f);
                   else hipLaunchKernelGGL(film_silu_bwd_kernel<T>, grid, dim3(TPB), C * sizeof(float), stream, (T*)du, de,
                                      (const T*)da, (const T*)u, e, HW, C, chunk))
}
int hdmoe_scale_rows_fwd(void* out, const void* x, const float* s, long rows, long L, int dtype, hipStream_t stream) {
  const long n = rows * L;
  DT_LAUNCH(dtype, L1D_W(L % VT<T>::W == 0 && al16(out) && al16(x), scale_rows_fwd_kernel, n, (T*)out, (const T*)x, s, L, n))
}
int hdmoe_scale_rows_bwd(void* dx, float* ds, const void* dy, const void* x, const float* s, long rows, long L,
                         int dtype, hipStream_t stream) {
  if (rows > 65535) return HDMOE_EINVAL;
  // W-wide items per workgroup: 2048 16-byte vectors (8 per thread) or 8192 elements
  DT_LAUNCH(dtype, if (L % VT<T>::W == 0 && al16(dx) && al16(dy) && al16(x))
                     hipLaunchKernelGGL((scale_rows_bwd_kernel<T, VT<T>::W>), dim3(cdiv(L / VT<T>::W, 2048), (unsigned)rows), dim3(TPB), 0, stream, (T*)dx, ds,
                                        (const T*)dy, (const T*)x, s, L, 2048);
                   else hipLaunchKernelGGL((scale_rows_bwd_kernel<T, 1>), dim3(cdiv(L, 8192), (unsigned)rows), dim3(TPB), 0, stream, (T*)dx, ds, (const T*)dy,
                                      (const T*)x, s, L, 8192))
}
int hdmoe_cat2_fwd(void* out, const void* a, const void* b, float wa, float wb, int Ca, int Cb, long rows, int dtype,
                   hipStream_t stream) {
  DT_LAUNCH(dtype, L1D_W(Ca % VT<T>::W == 0 && Cb % VT<T>::W == 0 && al16(out) && al16(a) && al16(b), cat2_fwd_kernel, rows * (Ca + Cb),
                         (T*)out, (const T*)a, (const T*)b, wa, wb, Ca, Cb, rows))
}
int hdmoe_cat2_bwd(void* da, void* db, const void* dout, float wa, float wb, int Ca, int Cb, long rows, int dtype,
                   hipStream_t stream) {
  DT_LAUNCH(dtype, L1D_W(Ca % VT<T>::W == 0 && Cb % VT<T>::W == 0 && al16(da) && al16(db) && al16(dout), cat2_bwd_kernel, rows * (Ca + Cb),
                         (T*)da, (T*)db, (const T*)dout, wa, wb, Ca, Cb, rows))
}
int hdmoe_pool2(void* out, const void* x, int N, int Ho, int Wo, int C, float scale, int dtype, hipStream_t stream) {
  const long n = (long)N * Ho * Wo * C;
  DT_LAUNCH(dtype, L1D_W(C % VT<T>::W == 0 && al16(out) && al16(x), pool2_kernel, n, (T*)out, (const T*)x, Ho, Wo, C, scale, n))
}
int hdmoe_upsample2(void* out, const void* x, int N, int Ho, int Wo, int C, float scale, int dtype, hipStream_t stream) {
  if ((Ho | Wo) & 1) return HDMOE_EINVAL;
  const long n = (long)N * Ho * Wo * C;
  DT_LAUNCH(dtype, L1D_W(C % VT<T>::W == 0 && al16(out) && al16(x), upsample2_kernel, n, (T*)out, (const T*)x, Ho, Wo, C, scale, n))
}
int hdmoe_seq_reduce(float* out, const void* x, int N, long S, int C, float scale, int dtype, hipStream_t stream) {
  if (N > 65535 || C > 8192) return HDMOE_EINVAL;
  // accumulates into `out` (callers pass zeros or a running sum); deterministic: no atomics, fixed summation order
  DT_LAUNCH(dtype, if (chunk_fixed_ok<T>(C) && al16(x)) hipLaunchKernelGGL(seq_reduce_det_vec_kernel<T>, dim3(N), dim3(256),
                                                                           (size_t)(256 / (C / VT<T>::W)) * C * sizeof(float), stream,
                                                                           out, (const T*)x, S, C, scale);
                   else hipLaunchKernelGGL(seq_reduce_det_kernel<T>, dim3(cdiv(C, TPB), N), dim3(TPB), 0, stream, out, (const T*)x, S, C, scale))
}
int hdmoe_seq_bcast_add(void* out, const void* x, const float* t, int N, long S, int C, float scale, int dtype,
                        hipStream_t stream) {
  const long n = (long)N * S * C;
  DT_LAUNCH(dtype, L1D(seq_bcast_add_kernel<T>, n, (T*)out, (const T*)x, t, S, C, scale, n))
}
int hdmoe_bias_add(void* out, const void* x, const float* bias, long rows, long L, int dtype, hipStream_t stream) {
  const long n = rows * L;
  DT_LAUNCH(dtype, L1D(bias_add_kernel<T>, n, (T*)out, (const T*)x, bias, L, n, nullptr, 0))
}
int hdmoe_colsum(float* out, const void* dy, long rows, long L, int dtype, hipStream_t stream) {
  const int rchunk = 64;
  if (cdiv(rows, rchunk) > 65535) return HDMOE_EINVAL;
  dim3 grid(cdiv(L, TPB), cdiv(rows, rchunk));
  DT_LAUNCH(dtype, hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(TPB), 0, stream, out, (const T*)dy, rows, L, rchunk, nullptr, 0))
}
/* The two above over the leading rows [rows[0], rows[1]) of an [N][S][L] tensor only (rows: DEVICE pointer to two ints, read by the
 * kernel; the grid is the all-rows one, nothing outside the window is read or written, an empty window does nothing). */
int hdmoe_bias_add_rows(void* out, const void* x, const float* bias, const int* rows, int N, long S, long L, int dtype, hipStream_t stream) {
  if (!out || !x || !bias || !rows || N < 0 || S < 1 || L < 1) return HDMOE_EINVAL;
  const long n = (long)N * S * L;
  if (n == 0) return HDMOE_OK;
  hdmoe_count_selection(HDMOE_SEL_ROW_WINDOW);
  DT_LAUNCH(dtype, L1D(bias_add_kernel<T>, n, (T*)out, (const T*)x, bias, L, n, rows, S * L))
}
int hdmoe_colsum_rows(float* out, const void* dy, const int* rows, int N, long S, long L, int dtype, hipStream_t stream) {
  if (!out || !dy || !rows || N < 0 || S < 1 || L < 1) return HDMOE_EINVAL;
  const int rchunk = 64;
  const long mrows = (long)N * S;
  if (mrows == 0) return HDMOE_OK;
  if (cdiv(mrows, rchunk) > 65535) return HDMOE_EINVAL;
  dim3 grid(cdiv(L, TPB), cdiv(mrows, rchunk));
  hdmoe_count_selection(HDMOE_SEL_ROW_WINDOW);
  DT_LAUNCH(dtype, hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(TPB), 0, stream, out, (const T*)dy, mrows, L, rchunk, rows, S))
}
int hdmoe_lerp_param_fwd(void* out, const void* a, const void* b, const float* alpha, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, L1D(lerp_param_fwd_kernel<T>, n, (T*)out, (const T*)a, (const T*)b, alpha, n))
}
int hdmoe_lerp_param_bwd(void* da, void* db, float* dalpha, const void* g, const void* a, const void* b,
                         const float* alpha, long n, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, if (n % VT<T>::W == 0 && al16(da) && al16(db) && al16(g) && al16(a) && al16(b)) {
                     long blocks = (n / VT<T>::W + TPB - 1) / TPB; if (blocks > 1024) blocks = 1024;   // (one atomic per block)
                     hipLaunchKernelGGL((lerp_param_bwd_kernel<T, VT<T>::W>), dim3((unsigned)blocks), dim3(TPB), 0, stream, (T*)da, (T*)db, dalpha, (const T*)g,
                                        (const T*)a, (const T*)b, alpha, n);
                   } else L1D((lerp_param_bwd_kernel<T, 1>), n, (T*)da, (T*)db, dalpha, (const T*)g, (const T*)a, (const T*)b, alpha, n))
}
int hdmoe_gate_mix_fwd(void* out, float* gate, const void* logits, const void* U, const void* A, long rows, int C,
                       int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, {
    const int lpr = C / VT<T>::W;
    if (C % VT<T>::W == 0 && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0 && al16(out) && al16(U) && al16(A))
      L1D(gate_mix_fwd_vec_kernel<T>, rows * lpr, (T*)out, gate, (const T*)logits, (const T*)U, (const T*)A, lpr, rows * lpr);
    else L1D(gate_mix_fwd_kernel<T>, rows * C, (T*)out, gate, (const T*)logits, (const T*)U, (const T*)A, C, rows);
  })
}
int hdmoe_gate_mix_bwd(void* dU, void* dA, void* dlogits, const void* dout, const float* dgate, const float* gate,
                       const void* U, const void* A, long rows, int C, int dtype, hipStream_t stream) {
  DT_LAUNCH(dtype, {
    const int lpr = C / VT<T>::W;
    if (C % VT<T>::W == 0 && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0 && al16(dU) && al16(dA) && al16(dout) && al16(U) && al16(A))
      L1D(gate_mix_bwd_vec_kernel<T>, (rows * lpr + 63) / 64 * 64, (T*)dU, (T*)dA, (T*)dlogits, (const T*)dout, dgate, gate, (const T*)U,
          (const T*)A, lpr, rows * lpr, (rows * lpr + 63) / 64 * 64);
    else L1D(gate_mix_bwd_kernel<T>, rows, (T*)dU, (T*)dA, (T*)dlogits, (const T*)dout, dgate, gate, (const T*)U, (const T*)A, C, rows);
  })
}
int hdmoe_softmax_rows_fwd(float* out, const float* x, long rows, int C, float scale, hipStream_t stream) {
  L1D(softmax_rows_fwd_kernel, rows, out, x, C, scale, rows);
  return hdmoe_launch_status();
}
int hdmoe_softmax_rows_bwd(float* dx, const float* dy, const float* y, long rows, int C, float scale, hipStream_t stream) {
  L1D(softmax_rows_bwd_kernel, rows, dx, dy, y, C, scale, rows);
  return hdmoe_launch_status();
}
int hdmoe_nchw_to_nhwc(void* out, const float* x, const float* s, int N, int C, long HW, int dtype, hipStream_t stream) {
  const long n = (long)N * C * HW;
  DT_LAUNCH(dtype, L1D(nchw_to_nhwc_kernel<T>, n, (T*)out, x, s, C, HW, n))
}
int hdmoe_nhwc_to_nchw(float* out, const void* F, const float* sf, const float* x, const float* sx, int N, int C, long HW,
                       int dtype, hipStream_t stream) {
  const long n = (long)N * C * HW;
  DT_LAUNCH(dtype, L1D(nhwc_to_nchw_kernel<T>, n, out, (const T*)F, sf, x, sx, C, HW, n))
}
int hdmoe_nhwc_to_nchw_guided(float* out, const void* F, const float* sf, const float* x, const float* sx, float g, int N, int C, long HW,
                              int dtype, hipStream_t stream) {
  if (!out || !F || N < 1 || C < 1 || HW < 1 || !(g == g) || g - g != 0.f) return HDMOE_EINVAL;
  const long n = (long)N * C * HW;
  DT_LAUNCH(dtype, L1D(nhwc_to_nchw_guided_kernel<T>, n, out, (const T*)F, sf, x, sx, g, C, HW, n))
}
int hdmoe_nhwc_to_nchw_guided_rows(float* out, const void* F, const float* sf, const float* x, const float* sx, const float* g, int N, int C,
                                   long HW, int dtype, hipStream_t stream) {
  if (!out || !F || !g || N < 1 || C < 1 || HW < 1) return HDMOE_EINVAL;
  const long n = (long)N * C * HW;
  DT_LAUNCH(dtype, L1D(nhwc_to_nchw_guided_rows_kernel<T>, n, out, (const T*)F, sf, x, sx, g, C, HW, n))
}
int hdmoe_lerp_rows(void* out, const void* ref, const void* d, const float* g, long rows, long per, int dtype, hipStream_t stream) {
  if (!out || !ref || !d || !g || rows < 1 || per < 1) return HDMOE_EINVAL;
  const long n = rows * per;
  DT_LAUNCH(dtype, L1D_W(per % VT<T>::W == 0 && al16(out) && al16(ref) && al16(d), lerp_rows_kernel, n, (T*)out, (const T*)ref, (const T*)d, g, per, n))
}
// the arms of guide_combine_kernel: W = VW when `vec_ok` else 1, resident when the sample fits GC_TPB * GC_R elements, with or without momentum
#define GC_ARM(L, TO, W_, RES_, ld, out, mom, q, rows, per)                                                                                  \
  if (mom) hipLaunchKernelGGL((guide_combine_kernel<L, TO, W_, RES_, true>), dim3(rows), dim3(GC_TPB), 0, stream, ld, out, mom, q, per);    \
  else hipLaunchKernelGGL((guide_combine_kernel<L, TO, W_, RES_, false>), dim3(rows), dim3(GC_TPB), 0, stream, ld, out, mom, q, per)
#define GC_LAUNCH(vec_ok, VW, L, TO, ld, out, mom, q, rows, per)                                       \
  if (vec_ok) {                                                                                        \
    if ((per) <= GC_TPB * GC_R) { GC_ARM(L, TO, VW, true, ld, out, mom, q, rows, per); }               \
    else { GC_ARM(L, TO, VW, false, ld, out, mom, q, rows, per); }                                     \
  } else {                                                                                             \
    if ((per) <= GC_TPB * GC_R) { GC_ARM(L, TO, 1, true, ld, out, mom, q, rows, per); }                \
    else { GC_ARM(L, TO, 1, false, ld, out, mom, q, rows, per); }                                      \
  }
// eta, r, beta, phi are the caller's to range-check; a NaN among them (or in g) is refused, r = inf is the "no clamp" value
static bool gc_args_ok(float g, const float* g_rows, float eta, float r, float beta, float phi, const float* momentum) {
  const bool fin = (g_rows || g - g == 0.f) && eta - eta == 0.f && beta - beta == 0.f && phi - phi == 0.f;
  return fin && r > 0.f && (beta == 0.f || momentum);
}
int hdmoe_guide_combine(void* out, const void* ref, const void* d, float g, const float* g_rows, float eta, float r, float beta, float phi,
                        float* momentum, long rows, long per, int dtype, hipStream_t stream) {
  if (!out || !ref || !d || rows < 1 || rows > 0x7fffffffL || per < 1 || !gc_args_ok(g, g_rows, eta, r, beta, phi, momentum)) return HDMOE_EINVAL;
  const GcPar q{g, g_rows, eta, r, beta, phi};
  float* mom = beta != 0.f ? momentum : nullptr;
  DT_LAUNCH(dtype, {
    const GcPair<T> ld{(const T*)ref, (const T*)d};
    GC_LAUNCH(per % VT<T>::W == 0 && al16(out) && al16(ref) && al16(d) && al16(mom), VT<T>::W, GcPair<T>, T, ld, (T*)out, mom, q, (unsigned)rows, per);
  })
}
int hdmoe_nhwc_to_nchw_guide_combine(float* out, const void* F, const float* sf, const float* x, const float* sx, float g, const float* g_rows,
                                     float eta, float r, float beta, float phi, float* momentum, int N, int C, long HW, int dtype,
                                     hipStream_t stream) {
  if (!out || !F || !sf || !x || !sx || N < 1 || C < 1 || HW < 1 || (long)C * HW > 0x7fffffffL || !gc_args_ok(g, g_rows, eta, r, beta, phi, momentum))
    return HDMOE_EINVAL;
  const GcPar q{g, g_rows, eta, r, beta, phi};
  float* mom = beta != 0.f ? momentum : nullptr;
  const long per = (long)C * HW;
  DT_LAUNCH(dtype, {
    const GcEgress<T> ld{(const T*)F, sf, x, sx, C, (unsigned)HW, (long)N * per};
    GC_LAUNCH(HW % 4 == 0 && al16(out) && al16(x) && al16(mom), 4, GcEgress<T>, float, ld, out, mom, q, (unsigned)N, per);
  })
}
// composed guidance: what both entry points refuse about K, the weights and the masks (masks: HW positions per plane, per = C HW)
static bool gc_compose_ok(int K, const float* a, const float* m, long HW, long per) {
  if (K < 1 || K > HDMOE_COMPOSE_MAX || !a) return false;
  return !m || (HW >= 1 && HW <= 0x7fffffffL && per % HW == 0);
}
int hdmoe_guide_compose(void* out, const void* ref, const void* const* d_ptrs, int K, const float* a, const float* m, long HW, float g,
                        const float* g_rows, float eta, float r, float beta, float phi, float* momentum, long rows, long per, int dtype,
                        hipStream_t stream) {
  if (!out || !ref || !d_ptrs || rows < 1 || rows > 0x7fffffffL || per < 1 || !gc_compose_ok(K, a, m, HW, per) ||
      !gc_args_ok(g, g_rows, eta, r, beta, phi, momentum))
    return HDMOE_EINVAL;
  bool al = al16(out) && al16(ref);
  for (int k = 0; k < K; ++k) {
    if (!d_ptrs[k]) return HDMOE_EINVAL;
    al = al && al16(d_ptrs[k]);
  }
  const GcPar q{g, g_rows, eta, r, beta, phi};
  float* mom = beta != 0.f ? momentum : nullptr;
  DT_LAUNCH(dtype, {
    GcCompose<T> ld{{}, (const T*)ref, a, m, K, m ? (unsigned)HW : 1u};
    for (int k = 0; k < K; ++k) ld.d[k] = (const T*)d_ptrs[k];
    // The element arm always re-reads: its resident form (16 unrolled vectors, each with the two k loops) does not fit the 128 registers
    // of a 1024-thread workgroup and would spill.  It is the fall-back for odd sizes and unaligned pointers, served from L2.
    if (per % VT<T>::W == 0 && al && al16(mom) && (!m || (HW % VT<T>::W == 0 && al16(m)))) {
      if (per <= GC_TPB * GC_R) { GC_ARM(GcCompose<T>, T, VT<T>::W, true, ld, (T*)out, mom, q, (unsigned)rows, per); }
      else { GC_ARM(GcCompose<T>, T, VT<T>::W, false, ld, (T*)out, mom, q, (unsigned)rows, per); }
    } else {
      GC_ARM(GcCompose<T>, T, 1, false, ld, (T*)out, mom, q, (unsigned)rows, per);
    }
  })
}
int hdmoe_nhwc_to_nchw_compose(float* out, const void* F, const float* sf, const float* x, const float* sx, int K, const float* a, const float* m,
                               float g, const float* g_rows, float eta, float r, float beta, float phi, float* momentum, int N, int C, long HW,
                               int dtype, hipStream_t stream) {
  if (!out || !F || !sf || !x || !sx || N < 1 || C < 1 || HW < 1 || (long)C * HW > 0x7fffffffL || !gc_compose_ok(K, a, m, HW, (long)C * HW) ||
      !gc_args_ok(g, g_rows, eta, r, beta, phi, momentum))
    return HDMOE_EINVAL;
  const GcPar q{g, g_rows, eta, r, beta, phi};
  float* mom = beta != 0.f ? momentum : nullptr;
  const long per = (long)C * HW;
  DT_LAUNCH(dtype, {
    const GcComposeEgress<T> ld{{(const T*)F, sf, x, sx, C, (unsigned)HW, (long)N * per}, K, a, m};
    GC_LAUNCH(HW % 4 == 0 && al16(out) && al16(x) && al16(mom) && al16(m), 4, GcComposeEgress<T>, float, ld, out, mom, q, (unsigned)N, per);
  })
}
static int relayout_entry(void* out, const void* in, const int* rows, int N, int H, int W, int C, int p, int hp, int wp, int order,
                          int to_img, int dtype, hipStream_t stream) {
  if (hp * p < H || wp * p < W) return HDMOE_EINVAL;
  const long n = (long)N * H * W * C;
  if (rows) hdmoe_count_selection(HDMOE_SEL_ROW_WINDOW);
  if (!to_img && order == 1 && al16(out) && (dtype == HDMOE_BF16 || dtype == HDMOE_F32) && p % (dtype == HDMOE_BF16 ? 8 : 4) == 0) {
    const long nv = (long)N * hp * wp * C * p * p / (dtype == HDMOE_BF16 ? 8 : 4);      // covers the padded tokens too (zeros)
    DT_LAUNCH(dtype, L1D(patch_to_tokens_o1_vec_kernel<T>, nv, (T*)out, (const T*)in, H, W, C, p, hp, wp, nv, rows))
  }
  if (al16(out) && al16(in) && C % (dtype == HDMOE_BF16 ? 8 : 4) == 0 && (dtype == HDMOE_BF16 || dtype == HDMOE_F32)) {
    const long nv = n / (dtype == HDMOE_BF16 ? 8 : 4);
    if (to_img) { DT_LAUNCH(dtype, L1D((patch_relayout_vec_kernel<T, true>), nv, (T*)out, (const T*)in, H, W, C, p, hp, wp, order, nv, rows)) }
    else { DT_LAUNCH(dtype, L1D((patch_relayout_vec_kernel<T, false>), nv, (T*)out, (const T*)in, H, W, C, p, hp, wp, order, nv, rows)) }
  }
  if (to_img) { DT_LAUNCH(dtype, L1D((patch_relayout_kernel<T, true>), n, (T*)out, (const T*)in, H, W, C, p, hp, wp, order, n, rows)) }
  else { DT_LAUNCH(dtype, L1D((patch_relayout_kernel<T, false>), n, (T*)out, (const T*)in, H, W, C, p, hp, wp, order, n, rows)) }
}
int hdmoe_patch_relayout(void* out, const void* in, int N, int H, int W, int C, int p, int hp, int wp, int order,
                         int to_img, int dtype, hipStream_t stream) {
  return relayout_entry(out, in, nullptr, N, H, W, C, p, hp, wp, order, to_img, dtype, stream);
}
/* hdmoe_patch_relayout over the image rows [rows[0], rows[1]) only (rows: DEVICE pointer to two ints, read by the kernel): same kernels,
 * same grid; rows outside the window are neither read nor written. */
int hdmoe_patch_relayout_rows(void* out, const void* in, const int* rows, int N, int H, int W, int C, int p, int hp, int wp, int order,
                              int to_img, int dtype, hipStream_t stream) {
  if (!rows || !out || !in || N < 0) return HDMOE_EINVAL;
  if (N == 0) return HDMOE_OK;
  return relayout_entry(out, in, rows, N, H, W, C, p, hp, wp, order, to_img, dtype, stream);
}
int hdmoe_fourier(float* out, const float* x, const float* freqs, const float* phases, int B, int F, hipStream_t stream) {
  const long n = (long)B * F;
  L1D(fourier_kernel, n, out, x, freqs, phases, F, n);
  return hdmoe_launch_status();
}
int hdmoe_edm_coeffs(float* coef, const float* sigma, int nsig, float sigma_data, int B, hipStream_t stream) {
  if (nsig != 1 && nsig != B) return HDMOE_EINVAL;
  L1D(edm_coeffs_kernel, B, coef, sigma, nsig, sigma_data, B);
  return hdmoe_launch_status();
}
int hdmoe_sigmoid_scaling(float* sv, float* su, float* pair, const float* c_noise, float tp, float soft, int B,
                          hipStream_t stream) {
  L1D(sigmoid_scaling_kernel, B, sv, su, pair, c_noise, tp, soft, B);
  return hdmoe_launch_status();
}
int hdmoe_adaln_fwd(float* out, const float* x, const float* cond, long B, int F, hipStream_t stream) {
  L1D(adaln_fwd_kernel, B * F, out, x, cond, F, B * F);
  return hdmoe_launch_status();
}
int hdmoe_adaln_bwd(float* dx, float* dcond, const float* g, const float* x, const float* cond, long B, int F, hipStream_t stream) {
  L1D(adaln_bwd_kernel, B * F, dx, dcond, g, x, cond, F, B * F);
  return hdmoe_launch_status();
}
int hdmoe_take_col_pos_fwd(float* out, const float* w, long B, int E, int e, hipStream_t stream) {
  if (e < 0 || e >= E) return HDMOE_EINVAL;
  L1D(take_col_pos_fwd_kernel, B, out, w, E, e, B);
  return hdmoe_launch_status();
}
int hdmoe_take_col_pos_bwd(float* dw, const float* g, const float* w, long B, int E, int e, hipStream_t stream) {
  if (e < 0 || e >= E) return HDMOE_EINVAL;
  L1D(take_col_pos_bwd_kernel, B, dw, g, w, E, e, B);
  return hdmoe_launch_status();
}
int hdmoe_dropout(void* out, const void* x, unsigned long long seed, const unsigned long long* seed_dev, float p, long n, int dtype,
                  hipStream_t stream) {
  if (p < 0.f || p >= 1.f) return HDMOE_EINVAL;
  DT_LAUNCH(dtype, L1D(dropout_kernel<T>, (n + 3) / 4, (T*)out, (const T*)x, (uint32_t)seed, (uint32_t)(seed >> 32), seed_dev, p, n))
}
int hdmoe_randn(float* out, unsigned long long seed, const unsigned long long* seed_dev, float scale, long n, hipStream_t stream) {
  L1D(randn_kernel, (n + 3) / 4, out, (uint32_t)seed, (uint32_t)(seed >> 32), seed_dev, scale, n);
  return hdmoe_launch_status();
}
int hdmoe_randn_ds(float* out, unsigned long long seed, const unsigned long long* seed_dev, const float* scale, long n, hipStream_t stream) {
  if (!out || !scale || n < 0) return HDMOE_EINVAL;
  L1D(randn_ds_kernel, (n + 3) / 4, out, (uint32_t)seed, (uint32_t)(seed >> 32), seed_dev, scale, n);
  return hdmoe_launch_status();
}
int hdmoe_seed_advance(unsigned long long* seed_dev, hipStream_t stream) {
  hipLaunchKernelGGL(seed_advance_kernel, dim3(1), dim3(1), 0, stream, seed_dev);
  return hdmoe_launch_status();
}

}  // extern "C"
