// Exponential moving average of the weights (EDM2 power-function profiles or a constant beta), up to 4 profiles at once, and the in-place
// exchange parameters <-> one profile.  One launch walks every tracked tensor through a (tensor, chunk) table shaped like the optimizer's
// (optim.hip): 4096-element chunks, 256 threads.  Pure streaming: p is read once, every e_k is read and written once, (1 + 2K) * 4 bytes
// per parameter.  Nothing is reduced and nothing is atomic, so the result is bit-identical from run to run and across data-parallel ranks.
// Below them: the post-hoc combination of saved averages into averages of other profiles (hdmoe_mt_combine).
#include "common.h"
#include "hdmoe.h"

namespace {

constexpr int EMA_MAX_PROFILES = 4;
struct __attribute__((aligned(8))) EmaDesc {   // mirrored by hdmoe_hip/ema.py
  unsigned long long p;                       // device address of the parameter (fp32)
  unsigned long long e[EMA_MAX_PROFILES];     // device addresses of its averages; entries >= nprofiles are ignored
  long numel;
};
constexpr int EMA_CHUNK = 4096;
constexpr int EMA_VEC_PER_THREAD = EMA_CHUNK / 4 / 256;    // float4 per thread of a full chunk

// The step count lives in device memory (int64: exact for ever, unlike a float counter) and is advanced in front of the update, so a
// captured graph replays with the right decay for every step.
// `ok` (hdmoe_mt_ema_ok; NULL = unguarded): a device verdict of hdmoe_mt_stats.  0 leaves the counter and every profile as they are.
__global__ void mt_ema_step_kernel(long long* step, const int* ok) {
  if (ok && !*ok) return;
  *step += 1;
}

// a = 1 - beta(t).  Power profile: beta(t) = (1 - 1/t)^(gamma + 1); 1 - beta through expm1 / log1p keeps full precision when beta -> 1.
DEVI float ema_weight(double coef, long long t, int mode) {
  if (mode == HDMOE_EMA_CONSTANT) return (float)(1.0 - coef);
  if (t <= 1) return 1.f;
  return (float)(-expm1((coef + 1.0) * log1p(-1.0 / (double)t)));
}
// lerp form with one fma; a == 1 stores p itself (e + (p - e) would round twice)
DEVI float ema_lerp(float p, float e, float a) { return a == 1.f ? p : fmaf(a, p - e, e); }

template <int K>
__global__ __launch_bounds__(256) void mt_ema_kernel(const EmaDesc* descs, const int2* chunks, const long long* step, const double* coefs,
                                                     int mode, const int* ok) {
  if (ok && !*ok) return;                          // (block-uniform: in front of the barrier below)
  __shared__ float sa[EMA_MAX_PROFILES];
  if (threadIdx.x < K) sa[threadIdx.x] = ema_weight(coefs[threadIdx.x], *step, mode);       // fp64, once per block
  __syncthreads();
  float a[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = sa[k];
  const int2 c = chunks[blockIdx.x];
  const EmaDesc d = descs[c.x];
  const long i0 = (long)c.y * EMA_CHUNK;
  const long i1 = i0 + EMA_CHUNK < d.numel ? i0 + EMA_CHUNK : d.numel;
  if (i0 >= i1) return;
  const float* p = (const float*)d.p;
  unsigned long long al = d.p;                     // a chunk starts 16 KiB into its tensor: it is aligned when the tensor is
#pragma unroll
  for (int k = 0; k < K; ++k) al |= d.e[k];
  long is = i0;                                    // first element left to the scalar loop
  if ((al & 15) == 0) {
    const int n4 = (int)((i1 - i0) >> 2);
    const float4* p4 = (const float4*)(p + i0);
    float4 pv[EMA_VEC_PER_THREAD];
#pragma unroll
    for (int u = 0; u < EMA_VEC_PER_THREAD; ++u) {
      const int j = threadIdx.x + 256 * u;
      if (j < n4) pv[u] = p4[j];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float4* e4 = (float4*)((float*)d.e[k] + i0);
      float4 ev[EMA_VEC_PER_THREAD];
#pragma unroll
      for (int u = 0; u < EMA_VEC_PER_THREAD; ++u) {
        const int j = threadIdx.x + 256 * u;
        if (j < n4) ev[u] = e4[j];
      }
#pragma unroll
      for (int u = 0; u < EMA_VEC_PER_THREAD; ++u) {
        const int j = threadIdx.x + 256 * u;
        if (j < n4)
          e4[j] = make_float4(ema_lerp(pv[u].x, ev[u].x, a[k]), ema_lerp(pv[u].y, ev[u].y, a[k]), ema_lerp(pv[u].z, ev[u].z, a[k]),
                              ema_lerp(pv[u].w, ev[u].w, a[k]));
      }
    }
    is = i0 + 4L * n4;                             // up to 3 tail elements of the tensor's last chunk
  }
  for (long i = is + threadIdx.x; i < i1; i += 256) {
    const float pi = p[i];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float* e = (float*)d.e[k];
      e[i] = ema_lerp(pi, e[i], a[k]);
    }
  }
}

// p <-> e[profile]: every element is read into registers before either side is written, and no two threads share an element
__global__ __launch_bounds__(256) void mt_swap_kernel(const EmaDesc* descs, const int2* chunks, int profile) {
  const int2 c = chunks[blockIdx.x];
  const EmaDesc* d = descs + c.x;                  // (fields read one by one: indexing a register copy by `profile` would go through scratch)
  const unsigned long long pa = d->p, ea = d->e[profile];
  const long numel = d->numel;
  const long i0 = (long)c.y * EMA_CHUNK;
  const long i1 = i0 + EMA_CHUNK < numel ? i0 + EMA_CHUNK : numel;
  if (i0 >= i1 || !ea) return;                     // !ea: the table holds fewer profiles than `profile`
  float* p = (float*)pa;
  float* e = (float*)ea;
  long is = i0;
  if (((pa | ea) & 15) == 0) {
    const int n4 = (int)((i1 - i0) >> 2);
    float4* p4 = (float4*)(p + i0);
    float4* e4 = (float4*)(e + i0);
    float4 pv[EMA_VEC_PER_THREAD], ev[EMA_VEC_PER_THREAD];
#pragma unroll
    for (int u = 0; u < EMA_VEC_PER_THREAD; ++u) {
      const int j = threadIdx.x + 256 * u;
      pv[u] = ev[u] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (j < n4) { pv[u] = p4[j]; ev[u] = e4[j]; }
    }
#pragma unroll
    for (int u = 0; u < EMA_VEC_PER_THREAD; ++u) {
      const int j = threadIdx.x + 256 * u;
      if (j < n4) { p4[j] = ev[u]; e4[j] = pv[u]; }
    }
    is = i0 + 4L * n4;
  }
  for (long i = is + threadIdx.x; i < i1; i += 256) {
    const float pi = p[i], ei = e[i];
    p[i] = ei; e[i] = pi;
  }
}

// Post-hoc reconstruction: dst_t = sum_s w[s][t] src_s over nsrc saved averages, K targets per launch.  A block owns 1024 consecutive
// elements (one float4 per lane) and walks the sources once for all K targets: (nsrc + K) * 4 bytes per element.  Every lane keeps its own
// fp64 fma chains in source order, so the result depends neither on the launch geometry nor on K nor on the access width.  The weights and
// the table are read-only and indexed by the loop counter alone: uniform (scalar-unit) loads, no per-lane traffic.
constexpr int CMB_MAX_DST = 8;
constexpr int CMB_MAX_SRC = 4096;
constexpr int CMB_BLOCK = 1024;                    // elements per block
constexpr int CMB_UNROLL = 4;                      // sources whose loads are issued before the first fma consumes one

template <int K, int W>                            // W floats per access: 4 (float4) or 1
DEVI void combine_span(const unsigned long long* __restrict__ src, const unsigned long long* da, int nsrc, const double* __restrict__ w,
                       long off) {
  typedef float vecW __attribute__((ext_vector_type(W)));
  typedef __attribute__((address_space(1))) vecW gvecW;                        // global, not flat: the table holds plain integers
  typedef __attribute__((address_space(1))) float gfloat;
  double acc[K][W];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int c = 0; c < W; ++c) acc[k][c] = 0.0;
  int s = 0;
  for (; s + CMB_UNROLL <= nsrc; s += CMB_UNROLL) {
    vecW x[CMB_UNROLL];
#pragma unroll
    for (int u = 0; u < CMB_UNROLL; ++u) x[u] = *(const gvecW*)((const gfloat*)src[s + u] + off);
#pragma unroll
    for (int u = 0; u < CMB_UNROLL; ++u)
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const double wk = w[(long)(s + u) * K + k];
#pragma unroll
        for (int c = 0; c < W; ++c) acc[k][c] = fma(wk, (double)x[u][c], acc[k][c]);
      }
  }
  for (; s < nsrc; ++s) {
    const vecW x = *(const gvecW*)((const gfloat*)src[s] + off);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double wk = w[(long)s * K + k];
#pragma unroll
      for (int c = 0; c < W; ++c) acc[k][c] = fma(wk, (double)x[c], acc[k][c]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    vecW y;
#pragma unroll
    for (int c = 0; c < W; ++c) y[c] = (float)acc[k][c];
    *(gvecW*)((gfloat*)da[k] + off) = y;
  }
}

template <int K>
__global__ __launch_bounds__(256) void mt_combine_kernel(const unsigned long long* __restrict__ src, const unsigned long long* __restrict__ dst,
                                                         int nsrc, long numel, const double* __restrict__ w) {
  unsigned long long al = 0;                       // every block looks at the whole table: nsrc * 8 bytes from L2 next to nsrc * 4 KiB of data
  for (int s = threadIdx.x; s < nsrc; s += 256) al |= src[s];
  unsigned long long da[K];
#pragma unroll
  for (int k = 0; k < K; ++k) { da[k] = dst[k]; al |= da[k]; }
  const bool vec = !__syncthreads_or((int)(al & 15));
  const long i0 = (long)blockIdx.x * CMB_BLOCK;
  const long i1 = i0 + CMB_BLOCK < numel ? i0 + CMB_BLOCK : numel;
  long is = i0;                                    // first element left to the scalar loop
  if (vec) {
    const int n4 = (int)((i1 - i0) >> 2);
    if ((int)threadIdx.x < n4) combine_span<K, 4>(src, da, nsrc, w, i0 + 4L * threadIdx.x);
    is = i0 + 4L * n4;                             // up to 3 tail elements of the last block
  }
  for (long i = is + threadIdx.x; i < i1; i += 256) combine_span<K, 1>(src, da, nsrc, w, i);
}

template <int K>
void launch_combine(const void* src, const void* dst, int nsrc, long numel, const double* w, hipStream_t stream) {
  const long blocks = (numel + CMB_BLOCK - 1) / CMB_BLOCK;
  hipLaunchKernelGGL(mt_combine_kernel<K>, dim3((unsigned)blocks), dim3(256), 0, stream, (const unsigned long long*)src,
                     (const unsigned long long*)dst, nsrc, numel, w);
}

}  // namespace

extern "C" {

int hdmoe_mt_combine(const void* src_table, const void* dst_table, int nsrc, int ndst, long numel, const double* weights,
                     hipStream_t stream) {
  if (nsrc < 1 || nsrc > CMB_MAX_SRC || ndst < 1 || ndst > CMB_MAX_DST || numel < 0) return HDMOE_EINVAL;
  if (numel > (long)CMB_BLOCK * 0x7fffffffL) return HDMOE_EINVAL;              // the grid's x dimension
  if (numel == 0) return HDMOE_OK;
  if (!src_table || !dst_table || !weights) return HDMOE_EINVAL;
  switch (ndst) {
    case 1: launch_combine<1>(src_table, dst_table, nsrc, numel, weights, stream); break;
    case 2: launch_combine<2>(src_table, dst_table, nsrc, numel, weights, stream); break;
    case 3: launch_combine<3>(src_table, dst_table, nsrc, numel, weights, stream); break;
    case 4: launch_combine<4>(src_table, dst_table, nsrc, numel, weights, stream); break;
    case 5: launch_combine<5>(src_table, dst_table, nsrc, numel, weights, stream); break;
    case 6: launch_combine<6>(src_table, dst_table, nsrc, numel, weights, stream); break;
    case 7: launch_combine<7>(src_table, dst_table, nsrc, numel, weights, stream); break;
    default: launch_combine<8>(src_table, dst_table, nsrc, numel, weights, stream); break;
  }
  return hdmoe_launch_status();
}

int hdmoe_ema_desc_bytes(void) { return (int)sizeof(EmaDesc); }

int hdmoe_mt_ema_ok(const void* descs, const int* chunks, int nchunks, int nprofiles, long long* step_counter, const double* gammas_or_betas,
                    int mode, const int* ok, hipStream_t stream) {
  if (nprofiles < 1 || nprofiles > EMA_MAX_PROFILES || nchunks < 0) return HDMOE_EINVAL;
  if (mode != HDMOE_EMA_POWER && mode != HDMOE_EMA_CONSTANT) return HDMOE_EINVAL;
  if (nchunks == 0) return HDMOE_OK;
  if (!descs || !chunks || !step_counter || !gammas_or_betas) return HDMOE_EINVAL;
  const EmaDesc* d = (const EmaDesc*)descs;
  const int2* c = (const int2*)chunks;
  hipLaunchKernelGGL(mt_ema_step_kernel, dim3(1), dim3(1), 0, stream, step_counter, ok);
  switch (nprofiles) {
    case 1: hipLaunchKernelGGL(mt_ema_kernel<1>, dim3(nchunks), dim3(256), 0, stream, d, c, step_counter, gammas_or_betas, mode, ok); break;
    case 2: hipLaunchKernelGGL(mt_ema_kernel<2>, dim3(nchunks), dim3(256), 0, stream, d, c, step_counter, gammas_or_betas, mode, ok); break;
    case 3: hipLaunchKernelGGL(mt_ema_kernel<3>, dim3(nchunks), dim3(256), 0, stream, d, c, step_counter, gammas_or_betas, mode, ok); break;
    default: hipLaunchKernelGGL(mt_ema_kernel<4>, dim3(nchunks), dim3(256), 0, stream, d, c, step_counter, gammas_or_betas, mode, ok); break;
  }
  return hdmoe_launch_status();
}

int hdmoe_mt_ema(const void* descs, const int* chunks, int nchunks, int nprofiles, long long* step_counter, const double* gammas_or_betas,
                 int mode, hipStream_t stream) {
  return hdmoe_mt_ema_ok(descs, chunks, nchunks, nprofiles, step_counter, gammas_or_betas, mode, nullptr, stream);
}

int hdmoe_mt_swap(const void* descs, const int* chunks, int nchunks, int profile, hipStream_t stream) {
  if (profile < 0 || profile >= EMA_MAX_PROFILES || nchunks < 0) return HDMOE_EINVAL;
  if (nchunks == 0) return HDMOE_OK;
  if (!descs || !chunks) return HDMOE_EINVAL;
  hipLaunchKernelGGL(mt_swap_kernel, dim3(nchunks), dim3(256), 0, stream, (const EmaDesc*)descs, (const int2*)chunks, profile);
  return hdmoe_launch_status();
}

}  // extern "C"
