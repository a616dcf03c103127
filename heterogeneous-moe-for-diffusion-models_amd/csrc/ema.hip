// Exponential moving average of the weights (EDM2 power-function profiles or a constant beta), up to 4 profiles at once, and the in-place
// exchange parameters <-> one profile.  One launch walks every tracked tensor through a (tensor, chunk) table shaped like the optimizer's
// (optim.hip): 4096-element chunks, 256 threads.  Pure streaming: p is read once, every e_k is read and written once, (1 + 2K) * 4 bytes
// per parameter.  Nothing is reduced and nothing is atomic, so the result is bit-identical from run to run and across data-parallel ranks.
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
__global__ void mt_ema_step_kernel(long long* step) { *step += 1; }

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
                                                     int mode) {
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

}  // namespace

extern "C" {

int hdmoe_ema_desc_bytes(void) { return (int)sizeof(EmaDesc); }

int hdmoe_mt_ema(const void* descs, const int* chunks, int nchunks, int nprofiles, long long* step_counter, const double* gammas_or_betas,
                 int mode, hipStream_t stream) {
  if (nprofiles < 1 || nprofiles > EMA_MAX_PROFILES || nchunks < 0) return HDMOE_EINVAL;
  if (mode != HDMOE_EMA_POWER && mode != HDMOE_EMA_CONSTANT) return HDMOE_EINVAL;
  if (nchunks == 0) return HDMOE_OK;
  if (!descs || !chunks || !step_counter || !gammas_or_betas) return HDMOE_EINVAL;
  const EmaDesc* d = (const EmaDesc*)descs;
  const int2* c = (const int2*)chunks;
  hipLaunchKernelGGL(mt_ema_step_kernel, dim3(1), dim3(1), 0, stream, step_counter);
  switch (nprofiles) {
    case 1: hipLaunchKernelGGL(mt_ema_kernel<1>, dim3(nchunks), dim3(256), 0, stream, d, c, step_counter, gammas_or_betas, mode); break;
    case 2: hipLaunchKernelGGL(mt_ema_kernel<2>, dim3(nchunks), dim3(256), 0, stream, d, c, step_counter, gammas_or_betas, mode); break;
    case 3: hipLaunchKernelGGL(mt_ema_kernel<3>, dim3(nchunks), dim3(256), 0, stream, d, c, step_counter, gammas_or_betas, mode); break;
    default: hipLaunchKernelGGL(mt_ema_kernel<4>, dim3(nchunks), dim3(256), 0, stream, d, c, step_counter, gammas_or_betas, mode); break;
  }
  return hdmoe_launch_status();
}

int hdmoe_mt_swap(const void* descs, const int* chunks, int nchunks, int profile, hipStream_t stream) {
  if (profile < 0 || profile >= EMA_MAX_PROFILES || nchunks < 0) return HDMOE_EINVAL;
  if (nchunks == 0) return HDMOE_OK;
  if (!descs || !chunks) return HDMOE_EINVAL;
  hipLaunchKernelGGL(mt_swap_kernel, dim3(nchunks), dim3(256), 0, stream, (const EmaDesc*)descs, (const int2*)chunks, profile);
  return hdmoe_launch_status();
}

}  // extern "C"
