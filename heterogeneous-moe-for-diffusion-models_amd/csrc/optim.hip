// Row N3 (the step right after the path): fused multi-tensor gradient-norm clip + AdamW (reference Utils/training.py:55-65,195-197:
// torch.optim.AdamW with 4 LR groups, torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)).
// One launch walks every parameter tensor through a (tensor, chunk) table; the clip coefficient is read from device memory, so
// norm -> clip -> update needs no host sync.
#include "common.h"
#include "hdmoe.h"

namespace {

struct __attribute__((aligned(8))) OptDesc {   // mirrored by hdmoe_hip/optim.py
  unsigned long long p, g, m, v;              // device addresses (m, v may be 0 for norm/scale-only tables)
  unsigned long long step;                    // float: this tensor's own AdamW step count (torch.optim.AdamW keeps one per tensor), or 0
  unsigned long long use;                     // float: > 0 when the tensor received a gradient this step (rows routed to its expert), or 0 = always
  long numel;
  int group, pad0;
};
constexpr int OPT_CHUNK = 4096;

// acc + v^2, the one expression both norm passes (mt_sumsq_kernel, mt_stats_kernel) accumulate with: whatever the compiler makes of it
// (one fma), it makes the same of it in both
DEVI float sq_add(float acc, float v) { return acc + v * v; }

// Two deterministic passes (no float atomics): the clip coefficient multiplies every update, so a run-to-run difference in the last bit of
// the norm would let data-parallel replicas drift apart bit by bit.
__global__ __launch_bounds__(256) void mt_sumsq_kernel(float* partial, const OptDesc* descs, const int2* chunks) {
  __shared__ float sm[16];
  const int2 c = chunks[blockIdx.x];
  const OptDesc d = descs[c.x];
  const float* g = (const float*)d.g;
  const long i0 = (long)c.y * OPT_CHUNK;
  const long i1 = i0 + OPT_CHUNK < d.numel ? i0 + OPT_CHUNK : d.numel;
  float acc = 0.f;
  for (long i = i0 + threadIdx.x; i < i1; i += 256) acc = sq_add(acc, g[i]);
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(1024) void mt_sumsq_final_kernel(float* out, const float* partial, int n) {
  __shared__ float sm[16];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 1024) acc += partial[i];       // fixed order per thread, fixed tree below
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) out[0] = acc;
}

// ---- gradient / parameter health: the norm pass above with {sum, min, max, non-finite count} beside the sum of squares and one row per
// statistics group.  Same two-pass shape and the same summation order for the sum of squares (a non-finite element adds an exact 0), so a
// table without one gives hdmoe_mt_sumsq's total bit for bit.
constexpr int STATS_WS = HDMOE_STATS_WS_PER_CHUNK;    // ws arrays of nchunks each: sumsq | sum | min | max | (elements << 16 | non-finite) | group
constexpr int STATS_MAX_GROUPS = 64;
static_assert(STATS_WS == 6, "mt_stats_kernel / mt_stats_final_kernel lay ws out as six arrays");

DEVI float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
template <typename T> DEVI T wave_add(T v) {       // integer counts: any order gives the same sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// One thread's record {sum of squares, sum, min, max, NC integer counts} reduced over the block in ONE exchange through LDS: every wave-level
// chain is issued before the barrier, so they overlap.  The two float sums follow block_sum's arithmetic to the bit -- wave_sum, then the
// wave values added in wave order to 0.f -- which is what ties the total sum of squares to hdmoe_mt_sumsq's.  Called once per kernel (no
// barrier in front of the LDS writes); the result is valid in thread 0 only.
template <typename C, int NC>
DEVI void block_stats(float& sq, float& s, float& mn, float& mx, C (&cnt)[NC], float (*smf)[16], C (*smc)[16]) {
  sq = wave_sum(sq); s = wave_sum(s); mn = wave_min(mn); mx = wave_max(mx);
#pragma unroll
  for (int k = 0; k < NC; ++k) cnt[k] = wave_add(cnt[k]);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  if (lane == 0) {
    smf[0][w] = sq; smf[1][w] = s; smf[2][w] = mn; smf[3][w] = mx;
#pragma unroll
    for (int k = 0; k < NC; ++k) smc[k][w] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  sq = 0.f; s = 0.f; mn = INFINITY; mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < NC; ++k) cnt[k] = 0;
  for (int i = 0; i < nw; ++i) {
    sq += smf[0][i]; s += smf[1][i]; mn = fminf(mn, smf[2][i]); mx = fmaxf(mx, smf[3][i]);
#pragma unroll
    for (int k = 0; k < NC; ++k) cnt[k] += smc[k][i];
  }
}

// one element into a thread's record; a non-finite one adds an exact 0 to both sums and 1 to `bad`
DEVI void stats_add(float v, float& sq, float& s, float& mn, float& mx, int& bad) {
  const bool fin = fabsf(v) < INFINITY;                       // false for NaN and +-Inf
  const float f = fin ? v : 0.f;
  sq = sq_add(sq, f);
  s += f;
  mn = fminf(mn, fin ? v : INFINITY);
  mx = fmaxf(mx, fin ? v : -INFINITY);
  bad += fin ? 0 : 1;
}

template <int WHICH>
__global__ __launch_bounds__(256) void mt_stats_kernel(float* ws, const OptDesc* descs, const int2* chunks, int nchunks) {
  __shared__ float smf[4][16];
  __shared__ int smc[1][16];
  const int2 c = chunks[blockIdx.x];
  const OptDesc d = descs[c.x];
  const float* x = (const float*)(WHICH == HDMOE_STATS_PARAM ? d.p : d.g);
  const long i0 = (long)c.y * OPT_CHUNK;
  const long i1 = i0 + OPT_CHUNK < d.numel ? i0 + OPT_CHUNK : d.numel;
  float sq = 0.f, s = 0.f, mn = INFINITY, mx = -INFINITY;
  int bad[1] = {0};
  // mt_sumsq_kernel's element-to-thread map and order: thread t takes t, t + 256, ...  A full chunk issues its 16 loads before the first
  // one is consumed (same order of additions, the memory round trips overlap); the last chunk of a tensor walks the rolled loop
  if (i1 - i0 == OPT_CHUNK) {
    float v[OPT_CHUNK / 256];
#pragma unroll
    for (int u = 0; u < OPT_CHUNK / 256; ++u) v[u] = x[i0 + threadIdx.x + 256 * u];
#pragma unroll
    for (int u = 0; u < OPT_CHUNK / 256; ++u) stats_add(v[u], sq, s, mn, mx, bad[0]);
  } else {
    for (long i = i0 + threadIdx.x; i < i1; i += 256) stats_add(x[i], sq, s, mn, mx, bad[0]);
  }
  block_stats<int, 1>(sq, s, mn, mx, bad, smf, smc);
  if (threadIdx.x == 0) {
    const long n = i1 > i0 ? i1 - i0 : 0;
    const long b = blockIdx.x;
    ws[b] = sq;
    ws[nchunks + b] = s;
    ws[2L * nchunks + b] = mn;
    ws[3L * nchunks + b] = mx;
    ((int*)ws)[4L * nchunks + b] = (int)(n << 16) | bad[0];     // both <= 4096
    ((int*)ws)[5L * nchunks + b] = d.group;
  }
}
// Block g < ngroups reduces the chunks of group g, block ngroups every chunk: thread t takes the partials t, t + 1024, ... in order (a chunk
// outside the row adds an exact 0), then the block tree -- for the total row's sum of squares that is mt_sumsq_final_kernel's sum.
// The total block also gives the verdict and advances the counters.
__global__ __launch_bounds__(1024) void mt_stats_final_kernel(float* stats, long long* counts, int* ok, long long* counters, const float* ws,
                                                              int nchunks, int ngroups, long long step) {
  __shared__ float smf[4][16];
  __shared__ long long smc[2][16];
  const int g = blockIdx.x;
  const bool total = g == ngroups;
  const int* packed = (const int*)ws + 4L * nchunks;
  const int* group = (const int*)ws + 5L * nchunks;
  float sq = 0.f, s = 0.f, mn = INFINITY, mx = -INFINITY;
  long long cnt[2] = {0, 0};                                  // non-finite elements, elements
  for (int i = threadIdx.x; i < nchunks; i += 1024) {
    const float a = ws[i], b = ws[nchunks + i], lo = ws[2L * nchunks + i], hi = ws[3L * nchunks + i];   // (all six loads in flight at once)
    const int pk = packed[i];
    const bool in = total || group[i] == g;
    sq += in ? a : 0.f;
    s += in ? b : 0.f;
    mn = fminf(mn, in ? lo : INFINITY);
    mx = fmaxf(mx, in ? hi : -INFINITY);
    cnt[0] += in ? pk & 0xffff : 0;
    cnt[1] += in ? pk >> 16 : 0;
  }
  block_stats<long long, 2>(sq, s, mn, mx, cnt, smf, smc);
  if (threadIdx.x != 0) return;
  const long long nbad = cnt[0], n = cnt[1];
  stats[4 * g + 0] = s; stats[4 * g + 1] = sq; stats[4 * g + 2] = mn; stats[4 * g + 3] = mx;
  counts[2 * g + 0] = nbad; counts[2 * g + 1] = n;
  if (!total) return;
  const int good = nbad == 0 && fabsf(sq) < INFINITY;
  if (ok) ok[0] = good;
  if (counters) {
    counters[0] += 1;
    if (good) counters[2] = 0;
    else { counters[1] += 1; counters[2] += 1; counters[3] = step; }
  }
}

// coef = min(1, max_norm / (sqrt(sumsq) + 1e-6))  (torch.nn.utils.clip_grad_norm_)
DEVI float clip_coef(const float* sumsq, float max_norm) {
  if (!sumsq) return 1.f;
  return fminf(1.f, max_norm / (sqrtf(*sumsq) + 1e-6f));
}
__global__ __launch_bounds__(256) void mt_scale_kernel(const OptDesc* descs, const int2* chunks, const float* sumsq, float max_norm) {
  const float coef = clip_coef(sumsq, max_norm);
  const int2 c = chunks[blockIdx.x];
  const OptDesc d = descs[c.x];
  float* g = (float*)d.g;
  const long i0 = (long)c.y * OPT_CHUNK;
  const long i1 = i0 + OPT_CHUNK < d.numel ? i0 + OPT_CHUNK : d.numel;
  for (long i = i0 + threadIdx.x; i < i1; i += 256) g[i] *= coef;
}
struct AdamArgs { float lr[8], wd[8]; float beta1, beta2, eps, max_norm; };
// A tensor whose expert received no sample this step is skipped altogether -- the reference leaves its .grad None and torch.optim.AdamW
// then applies neither weight decay nor moment decay nor a step-count increment (reference model_config1.py:26-29 + Utils/training.py:195-197).
// `ok` (hdmoe_mt_adamw_ok; NULL = unguarded): a device verdict of hdmoe_mt_stats.  0 leaves the whole launch without a single store.
__global__ __launch_bounds__(256) void mt_step_kernel(const OptDesc* descs, int ntensors, const int* ok) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ntensors) return;
  if (ok && !*ok) return;
  const OptDesc d = descs[t];
  if (!d.step) return;
  if (d.use && !(*(const float*)d.use > 0.f)) return;
  *(float*)d.step += 1.f;
}
__global__ __launch_bounds__(256) void mt_adamw_kernel(const OptDesc* descs, const int2* chunks, const float* sumsq, AdamArgs a, const int* ok) {
  if (ok && !*ok) return;
  const int2 c = chunks[blockIdx.x];
  const OptDesc d = descs[c.x];
  if (d.use && !(*(const float*)d.use > 0.f)) return;
  const float coef = clip_coef(sumsq, a.max_norm);
  float* p = (float*)d.p; const float* g = (const float*)d.g; float* m = (float*)d.m; float* v = (float*)d.v;
  const float lr = a.lr[d.group], wd = a.wd[d.group];
  const float step = *(const float*)d.step;                  // already advanced by mt_step_kernel
  const float bc1 = 1.f - powf(a.beta1, step), bc2_sqrt = sqrtf(1.f - powf(a.beta2, step));
  const float step_size = lr / bc1;
  const long i0 = (long)c.y * OPT_CHUNK;
  const long i1 = i0 + OPT_CHUNK < d.numel ? i0 + OPT_CHUNK : d.numel;
  for (long i = i0 + threadIdx.x; i < i1; i += 256) {
    const float gi = g[i] * coef;
    float pi = p[i] * (1.f - lr * wd);                       // decoupled weight decay
    const float mi = a.beta1 * m[i] + (1.f - a.beta1) * gi;
    const float vi = a.beta2 * v[i] + (1.f - a.beta2) * gi * gi;
    m[i] = mi; v[i] = vi;
    pi -= step_size * mi / (sqrtf(vi) / bc2_sqrt + a.eps);
    p[i] = pi;
  }
}

}  // namespace

extern "C" {

int hdmoe_opt_desc_bytes(void) { return (int)sizeof(OptDesc); }
// sumsq (1 float) = sum over all tensors of g^2; ws: nchunks floats of scratch
int hdmoe_mt_sumsq(float* sumsq, const void* descs, const int* chunks, int nchunks, float* ws, hipStream_t stream) {
  if (!sumsq || (nchunks > 0 && !ws)) return HDMOE_EINVAL;
  if (nchunks > 0) hipLaunchKernelGGL(mt_sumsq_kernel, dim3(nchunks), dim3(256), 0, stream, ws, (const OptDesc*)descs, (const int2*)chunks);
  hipLaunchKernelGGL(mt_sumsq_final_kernel, dim3(1), dim3(1024), 0, stream, sumsq, ws, nchunks > 0 ? nchunks : 0);
  return hdmoe_launch_status();
}
int hdmoe_mt_clip_scale(const void* descs, const int* chunks, int nchunks, const float* sumsq, float max_norm, hipStream_t stream) {
  if (nchunks > 0) hipLaunchKernelGGL(mt_scale_kernel, dim3(nchunks), dim3(256), 0, stream, (const OptDesc*)descs, (const int2*)chunks, sumsq, max_norm);
  return hdmoe_launch_status();
}
// lr / wd: host arrays of ngroups (<= 8) floats; sumsq may be NULL (no clipping).  Every descriptor carries its tensor's step counter (device
// float, advanced here) and optionally a "used this step" flag; bias corrections are computed on the device from the per-tensor count.
int hdmoe_mt_adamw_ok(const void* descs, const int* chunks, int nchunks, int ntensors, const float* sumsq, float max_norm, const float* group_lr,
                      const float* group_wd, int ngroups, float beta1, float beta2, float eps, const int* ok, hipStream_t stream) {
  if (ngroups < 1 || ngroups > 8 || ntensors < 0) return HDMOE_EINVAL;
  AdamArgs a;
  for (int i = 0; i < 8; ++i) { a.lr[i] = group_lr[i < ngroups ? i : 0]; a.wd[i] = group_wd[i < ngroups ? i : 0]; }
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.max_norm = max_norm;
  if (ntensors > 0) hipLaunchKernelGGL(mt_step_kernel, dim3(cdiv(ntensors, 256)), dim3(256), 0, stream, (const OptDesc*)descs, ntensors, ok);
  if (nchunks > 0)
    hipLaunchKernelGGL(mt_adamw_kernel, dim3(nchunks), dim3(256), 0, stream, (const OptDesc*)descs, (const int2*)chunks, sumsq, a, ok);
  return hdmoe_launch_status();
}
int hdmoe_mt_adamw(const void* descs, const int* chunks, int nchunks, int ntensors, const float* sumsq, float max_norm, const float* group_lr,
                   const float* group_wd, int ngroups, float beta1, float beta2, float eps, hipStream_t stream) {
  return hdmoe_mt_adamw_ok(descs, chunks, nchunks, ntensors, sumsq, max_norm, group_lr, group_wd, ngroups, beta1, beta2, eps, nullptr, stream);
}
// stats (ngroups + 1, 4), counts (ngroups + 1, 2); ws: HDMOE_STATS_WS_PER_CHUNK * nchunks floats.  Contract: include/hdmoe.h
int hdmoe_mt_stats(float* stats, long long* counts, int* ok, long long* counters, const void* descs, const int* chunks, int nchunks,
                   int ngroups, int which, long long step, float* ws, hipStream_t stream) {
  if (!stats || !counts || ngroups < 1 || ngroups > STATS_MAX_GROUPS || nchunks < 0) return HDMOE_EINVAL;
  if (which != HDMOE_STATS_GRAD && which != HDMOE_STATS_PARAM) return HDMOE_EINVAL;
  if (nchunks > 0 && (!descs || !chunks || !ws)) return HDMOE_EINVAL;
  if (nchunks > 0) {
    if (which == HDMOE_STATS_PARAM)
      hipLaunchKernelGGL(mt_stats_kernel<HDMOE_STATS_PARAM>, dim3(nchunks), dim3(256), 0, stream, ws, (const OptDesc*)descs, (const int2*)chunks, nchunks);
    else
      hipLaunchKernelGGL(mt_stats_kernel<HDMOE_STATS_GRAD>, dim3(nchunks), dim3(256), 0, stream, ws, (const OptDesc*)descs, (const int2*)chunks, nchunks);
  }
  hipLaunchKernelGGL(mt_stats_final_kernel, dim3(ngroups + 1), dim3(1024), 0, stream, stats, counts, ok, counters, ws, nchunks, ngroups, step);
  return hdmoe_launch_status();
}

}  // extern "C"
