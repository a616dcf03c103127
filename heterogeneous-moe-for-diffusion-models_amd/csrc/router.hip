// K1 / K2: noisy-top-k router head and the sync-free sample dispatch.
//   head     : Router.forward tail, reference models/model_components.py:155-168
//   dispatch : router_to_unet_experts, reference models/model_config1.py:11-39 -- the reference gathers x[mask]
//              per expert behind a host sync (mask.any()); here a single-workgroup plan kernel builds the
//              expert-contiguous permutation on the device (LDS histogram + wavefront ballot scan), so the
//              whole step stays capturable in a hipGraph.
#include "common.h"
#include "hdmoe.h"

namespace {

constexpr int TPB = 256;

// ---------------------------------------------------------------- router head (one thread per row; E <= 64)
__global__ void router_head_fwd_kernel(float* sparse, float* probs, float* xout, int* idx, const float* logits, const float* noise,
                                       const float* mask, int E, int k, long B) {
  GRID_STRIDE(b, B) {
    const float* lg = logits + b * E;
    float* xo = xout + b * E;
    float mx = -INFINITY;
    for (int e = 0; e < E; ++e) {
      float v = lg[e];
      if (noise) v += noise[b * E + e];
      if (mask && mask[b * E + e] == 0.f) v = -INFINITY;
      xo[e] = v;
      mx = fmaxf(mx, v);
    }
    float sum = 0.f;
    for (int e = 0; e < E; ++e) sum += expf(xo[e] - mx);
    for (int e = 0; e < E; ++e) { probs[b * E + e] = expf(xo[e] - mx) / sum; sparse[b * E + e] = 0.f; }
    // top-k by repeated argmax; ties -> lowest index (torch.topk's tie order is implementation-defined)
    unsigned long long taken = 0ull;
    float top = 0.f;
    for (int j = 0; j < k; ++j) {
      int bi = -1; float bv = 0.f;
      for (int e = 0; e < E; ++e) {
        if ((taken >> e) & 1ull) continue;
        if (bi < 0 || xo[e] > bv) { bi = e; bv = xo[e]; }
      }
      taken |= 1ull << bi;
      idx[b * k + j] = bi;
      if (j == 0) top = bv;
    }
    float ws = 0.f;
    for (int j = 0; j < k; ++j) ws += expf(xo[idx[b * k + j]] - top);
    for (int j = 0; j < k; ++j) sparse[b * E + idx[b * k + j]] = expf(xo[idx[b * k + j]] - top) / ws;
  }
}

__global__ void router_head_bwd_kernel(float* dlogits, const float* dsparse, const float* dprobs, const float* dxout, const float* sparse,
                                       const float* probs, const int* idx, const float* mask, int E, int k, long B) {
  GRID_STRIDE(b, B) {
    float* dl = dlogits + b * E;
    float dot = 0.f;
    if (dprobs) for (int e = 0; e < E; ++e) dot += probs[b * E + e] * dprobs[b * E + e];
    for (int e = 0; e < E; ++e) {
      float g = dxout ? dxout[b * E + e] : 0.f;
      if (dprobs) g += probs[b * E + e] * (dprobs[b * E + e] - dot);
      dl[e] = g;
    }
    if (dsparse) {
      float dw = 0.f;
      for (int j = 0; j < k; ++j) { const int e = idx[b * k + j]; dw += sparse[b * E + e] * dsparse[b * E + e]; }
      for (int j = 0; j < k; ++j) { const int e = idx[b * k + j]; dl[e] += sparse[b * E + e] * (dsparse[b * E + e] - dw); }
    }
    if (mask) for (int e = 0; e < E; ++e) if (mask[b * E + e] == 0.f) dl[e] = 0.f;
  }
}

// ---------------------------------------------------------------- router head with a selection bias (loss-free load balancing)
// The head above with one change: the top-k runs over xout[e] + sel_bias[e].  probs, xout and the k gate weights -- the softmax of the RAW
// xout over the selected experts -- never see the bias, so it has no gradient and router_head_bwd_kernel serves both heads.  The first pick
// is no longer the largest raw value: the softmax is stabilised by the maximum of xout over the selected set.
// load / target (both or neither): integer accumulators of the step.  load[e] counts the rows that selected e among the experts their mask
// allows (a row with fewer allowed experts than k fills its top-k with masked ones at weight 0: the dispatch routes nothing there, and
// nothing is counted); target[e] gains every allowing row's fair share round(2^20 min(k, a_b) / a_b), a_b = the row's allowed experts.
// Integer sums do not depend on the order of the atomics.  Each wavefront reduces its 64 rows per expert in registers (a ballot for the
// load, a 32-bit butterfly for the shares: 64 * 2^20 fits), one lane adds the result to the workgroup's LDS copy, and the workgroup ends
// with E global atomics -- 256 lanes adding to the same few LDS words one by one cost more than the head itself.
constexpr int BAL_SHIFT = 20;
__global__ __launch_bounds__(TPB) void router_head_bias_fwd_kernel(float* sparse, float* probs, float* xout, int* idx, const float* logits,
                                                                   const float* noise, const float* mask, const float* sel_bias,
                                                                   unsigned long long* load, unsigned long long* target, int E, int k,
                                                                   long B) {
  __shared__ unsigned long long s_load[64], s_tgt[64];
  const bool acc = load != nullptr;                             // kernel-uniform: the barriers below are reached by all threads or by none
  if (acc) {
    if ((int)threadIdx.x < 64) { s_load[threadIdx.x] = 0ull; s_tgt[threadIdx.x] = 0ull; }
    __syncthreads();
  }
  // workgroup-uniform trip count: the wavefront reductions below need every lane, also those past the last row
  for (long base = (long)blockIdx.x * blockDim.x; base < B; base += (long)gridDim.x * blockDim.x) {
    const long b = base + threadIdx.x;
    unsigned long long taken = 0ull, allow = 0ull;              // bit e: picked / allowed by the row's mask
    unsigned share = 0u;
    if (b < B) {
      const float* lg = logits + b * E;
      float* xo = xout + b * E;
      float mx = -INFINITY;
      int allowed = 0;
      for (int e = 0; e < E; ++e) {
        float v = lg[e];
        if (noise) v += noise[b * E + e];
        if (mask && mask[b * E + e] == 0.f) v = -INFINITY; else { ++allowed; allow |= 1ull << e; }
        xo[e] = v;
        mx = fmaxf(mx, v);
      }
      float sum = 0.f;
      for (int e = 0; e < E; ++e) sum += expf(xo[e] - mx);
      for (int e = 0; e < E; ++e) { probs[b * E + e] = expf(xo[e] - mx) / sum; sparse[b * E + e] = 0.f; }
      // top-k of the biased scores by repeated argmax; ties -> lowest index.  -inf + bias stays -inf: a masked entry is picked last.
      float top = -INFINITY;
      for (int j = 0; j < k; ++j) {
        int bi = -1; float bv = 0.f;
        for (int e = 0; e < E; ++e) {
          if ((taken >> e) & 1ull) continue;
          const float s = xo[e] + sel_bias[e];
          if (bi < 0 || s > bv) { bi = e; bv = s; }
        }
        taken |= 1ull << bi;
        idx[b * k + j] = bi;
        top = fmaxf(top, xo[bi]);
      }
      float ws = 0.f;
      for (int j = 0; j < k; ++j) ws += expf(xo[idx[b * k + j]] - top);
      for (int j = 0; j < k; ++j) sparse[b * E + idx[b * k + j]] = expf(xo[idx[b * k + j]] - top) / ws;
      if (allowed > 0) {
        const unsigned q = (unsigned)(k < allowed ? k : allowed);
        share = ((q << BAL_SHIFT) + (unsigned)(allowed >> 1)) / (unsigned)allowed;       // <= 2^20
      }
    }
    if (acc) {
      const unsigned long long routed = taken & allow;
      for (int e = 0; e < E; ++e) {
        const unsigned long long picked = __ballot((routed >> e) & 1ull);
        unsigned t = ((allow >> e) & 1ull) ? share : 0u;
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);
        if ((threadIdx.x & 63) == 0) {
          if (picked) atomicAdd(&s_load[e], (unsigned long long)__popcll(picked));
          if (t) atomicAdd(&s_tgt[e], (unsigned long long)t);
        }
      }
    }
  }
  if (acc) {
    __syncthreads();
    if ((int)threadIdx.x < E) {
      if (s_load[threadIdx.x]) atomicAdd(&load[threadIdx.x], s_load[threadIdx.x]);
      if (s_tgt[threadIdx.x]) atomicAdd(&target[threadIdx.x], s_tgt[threadIdx.x]);
    }
  }
}

// One wavefront, behind the optimizer.  `ok` (NULL = unguarded): the device verdict of hdmoe_mt_stats; 0 leaves the bias as it is.
//   bias[e] += rate * sign(target[e] - 2^20 load[e])   (integers; a tie gives 0), then minus the mean, then clamped to +-bias_max;
//   last_* = the accumulators; the accumulators = 0 -- both always: a skipped step's counts must not reach the next step's decision.
// Every lane sums the E values in index order, so the mean does not depend on a reduction tree.
__global__ __launch_bounds__(64) void balance_bias_update_kernel(float* bias, long long* load, long long* target, long long* last_load,
                                                                 long long* last_target, const int* ok, float rate, float bias_max, int E) {
  __shared__ float sb[64];
  const int e = threadIdx.x;
  const bool apply = !ok || *ok != 0;                          // workgroup-uniform
  const long long l = e < E ? load[e] : 0ll, t = e < E ? target[e] : 0ll;
  if (apply) {
    float v = 0.f;
    if (e < E) {
      const long long d = t - l * (1ll << BAL_SHIFT);
      v = bias[e] + rate * (d > 0 ? 1.f : (d < 0 ? -1.f : 0.f));
      sb[e] = v;
    }
    __syncthreads();
    if (e < E) {
      float s = 0.f;
      for (int i = 0; i < E; ++i) s += sb[i];
      v -= s / (float)E;
      bias[e] = fminf(fmaxf(v, -bias_max), bias_max);
    }
  }
  if (e < E) {
    last_load[e] = l; last_target[e] = t;
    load[e] = 0ll; target[e] = 0ll;
  }
}

// ---------------------------------------------------------------- dispatch plan (single workgroup)
// routed pair (b, e) <=> sparse[b][e] > 0 (NaN > 0 is false: an all-masked sample is routed nowhere, as in the reference).
// Output order: expert-major, sample-minor (stable) == the order x[mask] produces per expert.
__global__ __launch_bounds__(1024) void dispatch_plan_kernel(int* perm, int* row_expert, float* row_w, int* inv, int* seg,
                                                            const float* sparse, int B, int E, int kcap) {
  __shared__ int cnt[64 + 1];
  __shared__ int wtot[16];
  __shared__ int base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
  const int R = B * kcap;
  for (int r = tid; r < R; r += blockDim.x) { perm[r] = -1; row_expert[r] = -1; row_w[r] = 0.f; inv[r] = -1; }
  if (tid <= E) cnt[tid] = 0;
  __syncthreads();
  for (int b = tid; b < B; b += blockDim.x)
    for (int e = 0; e < E; ++e)
      if (sparse[(long)b * E + e] > 0.f) atomicAdd(&cnt[e], 1);
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int e = 0; e <= E; ++e) { const int c = e < E ? cnt[e] : 0; cnt[e] = run; seg[e] = run < R ? run : R; run += c; }
  }
  __syncthreads();
  for (int e = 0; e < E; ++e) {
    if (tid == 0) base = cnt[e];
    __syncthreads();
    for (int b0 = 0; b0 < B; b0 += blockDim.x) {
      const int b = b0 + tid;
      const float w = b < B ? sparse[(long)b * E + e] : 0.f;
      const bool f = w > 0.f;
      const unsigned long long bal = __ballot(f);
      const int pre = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wtot[wv] = __popcll(bal);
      __syncthreads();
      int off = 0, tot = 0;
      for (int i = 0; i < nw; ++i) { if (i < wv) off += wtot[i]; tot += wtot[i]; }
      if (f) {
        const int pos = base + off + pre;
        int slot = 0;
        for (int e2 = 0; e2 < e; ++e2) slot += sparse[(long)b * E + e2] > 0.f ? 1 : 0;
        if (pos < R) {
          perm[pos] = b; row_expert[pos] = e; row_w[pos] = w;
          if (slot < kcap) inv[b * kcap + slot] = pos;
        }
      }
      __syncthreads();
      if (tid == 0) base += tot;
      __syncthreads();
    }
  }
}

// dst[r][:] = src[perm[r]][:]  (zeros for unused rows); 16-byte units
__global__ void gather_rows_kernel(uint4* dst, const uint4* src, const int* perm, long Lv, long n) {
  GRID_STRIDE(i, n) {
    const long r = i / Lv, c = i - r * Lv;
    const int s = perm[r];
    dst[i] = s >= 0 ? src[(long)s * Lv + c] : make_uint4(0, 0, 0, 0);
  }
}
template <typename T>
__global__ void gather_rows_scalar_kernel(T* dst, const T* src, const int* perm, long L, long n) {
  GRID_STRIDE(i, n) {
    const long r = i / L, c = i - r * L;
    const int s = perm[r];
    dst[i] = s >= 0 ? src[(long)s * L + c] : from_f<T>(0.f);
  }
}
// dst[r][:] = src[perm[r] % Bsrc][:]: the plan was built over a stack of copies of the Bsrc source rows (the guided evaluation's
// [conditional ; unconditional] halves share the stem features and the time embedding), the source is stored once
__global__ void gather_rows_paired_kernel(uint4* dst, const uint4* src, const int* perm, int Bsrc, long Lv, long n) {
  GRID_STRIDE(i, n) {
    const long r = i / Lv, c = i - r * Lv;
    const int s = perm[r];
    dst[i] = s >= 0 ? src[(long)(s % Bsrc) * Lv + c] : make_uint4(0, 0, 0, 0);
  }
}
template <typename T>
__global__ void gather_rows_paired_scalar_kernel(T* dst, const T* src, const int* perm, int Bsrc, long L, long n) {
  GRID_STRIDE(i, n) {
    const long r = i / L, c = i - r * L;
    const int s = perm[r];
    dst[i] = s >= 0 ? src[(long)(s % Bsrc) * L + c] : from_f<T>(0.f);
  }
}
// out[b][:] = sum_j w[r_j] * ys[r_j][:], r_j = inv[b][j]  (weights optional)
template <typename T>
__global__ void combine_rows_fwd_kernel(T* out, const T* ys, const int* inv, const float* row_w, int kcap, long L, long n) {
  GRID_STRIDE(i, n) {
    const long b = i / L, c = i - b * L;
    float acc = 0.f;
    for (int j = 0; j < kcap; ++j) {
      const int r = inv[b * kcap + j];
      if (r >= 0) {
        const float w = row_w ? row_w[r] : 1.f;
        if (w > 0.f) acc += w * to_f(ys[(long)r * L + c]);
      }
    }
    out[i] = from_f<T>(acc);
  }
}
// dys[r][:] = w[r] * dout[perm[r]][:] ;  dsparse[perm[r]][row_expert[r]] += <dout[perm[r]], ys[r]>
template <typename T>
__global__ void combine_rows_bwd_kernel(T* dys, float* dsparse, const T* dout, const T* ys, const int* perm, const int* row_expert,
                                        const float* row_w, int E, long L, int chunk) {
  __shared__ float sm[16];
  const long nck = (L + chunk - 1) / chunk;
  const long r = blockIdx.x / nck;                              // 1-D grid: (row, chunk) pairs, no 65535-row limit
  const int b = perm[r];
  const long p0 = (long)(blockIdx.x - r * nck) * chunk;
  const long p1 = (p0 + chunk < L) ? p0 + chunk : L;
  const float w = b >= 0 ? (row_w ? row_w[r] : 1.f) : 0.f;
  float acc = 0.f;
  for (long i = p0 + threadIdx.x; i < p1; i += blockDim.x) {
    const float g = b >= 0 ? to_f(dout[(long)b * L + i]) : 0.f;
    dys[(long)r * L + i] = from_f<T>(w * g);
    if (dsparse && b >= 0) acc += g * to_f(ys[(long)r * L + i]);
  }
  if (dsparse) {
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0 && b >= 0) atomicAdd(&dsparse[(long)b * E + row_expert[r]], acc);
  }
}

// counts ACCUMULATE: several forwards may share one optimizer step (gradient accumulation); FusedAdamW.step clears them behind the update
__global__ void seg_counts_kernel(float* counts, const int* seg, int E) {
  if ((int)threadIdx.x < E) counts[threadIdx.x] += (float)(seg[threadIdx.x + 1] - seg[threadIdx.x]);
}
// the same from the sparse gate weights (B, E) when no dispatch plan exists (experts evaluated on the whole batch): rows with weight > 0
__global__ void route_counts_kernel(float* counts, const float* sparse, int B, int E) {
  const int e = blockIdx.x;
  float c = 0.f;
  for (int b = threadIdx.x; b < B; b += blockDim.x) c += sparse[(long)b * E + e] > 0.f ? 1.f : 0.f;
  __shared__ float sm[16];
  c = block_sum(c, sm);
  if (threadIdx.x == 0) counts[e] += c;
}

}  // namespace

extern "C" {

int hdmoe_router_head_fwd(float* sparse, float* probs, float* xout, int* idx, const float* logits, const float* noise,
                          const float* mask, long B, int E, int k, hipStream_t stream) {
  if (E < 1 || E > 64 || k < 1 || k > E) return HDMOE_EINVAL;
  hipLaunchKernelGGL(router_head_fwd_kernel, dim3(grid_for(B)), dim3(TPB), 0, stream, sparse, probs, xout, idx, logits, noise, mask, E, k, B);
  return hdmoe_launch_status();
}
int hdmoe_router_head_bwd(float* dlogits, const float* dsparse, const float* dprobs, const float* dxout, const float* sparse,
                          const float* probs, const int* idx, const float* mask, long B, int E, int k, hipStream_t stream) {
  if (E < 1 || E > 64 || k < 1 || k > E) return HDMOE_EINVAL;
  hipLaunchKernelGGL(router_head_bwd_kernel, dim3(grid_for(B)), dim3(TPB), 0, stream, dlogits, dsparse, dprobs, dxout, sparse, probs, idx, mask, E, k, B);
  return hdmoe_launch_status();
}
int hdmoe_router_head_bias_fwd(float* sparse, float* probs, float* xout, int* idx, const float* logits, const float* noise,
                               const float* mask, const float* sel_bias, long long* load, long long* target, long B, int E, int k,
                               hipStream_t stream) {
  if (E < 1 || E > 64 || k < 1 || k > E || B < 0 || !sel_bias || (load == nullptr) != (target == nullptr)) return HDMOE_EINVAL;
  if (!sparse || !probs || !xout || !idx || !logits) return HDMOE_EINVAL;
  if (B == 0) return HDMOE_OK;
  hipLaunchKernelGGL(router_head_bias_fwd_kernel, dim3(grid_for(B)), dim3(TPB), 0, stream, sparse, probs, xout, idx, logits, noise, mask,
                     sel_bias, (unsigned long long*)load, (unsigned long long*)target, E, k, B);
  return hdmoe_launch_status();
}
int hdmoe_balance_bias_update(float* bias, long long* load, long long* target, long long* last_load, long long* last_target, const int* ok,
                              float rate, float bias_max, int E, hipStream_t stream) {
  if (!bias || !load || !target || !last_load || !last_target || E < 1 || E > 64) return HDMOE_EINVAL;
  if (!(rate >= 0.f) || !(bias_max >= 0.f)) return HDMOE_EINVAL;          // (NaN fails both)
  hipLaunchKernelGGL(balance_bias_update_kernel, dim3(1), dim3(64), 0, stream, bias, load, target, last_load, last_target, ok, rate, bias_max, E);
  return hdmoe_launch_status();
}
int hdmoe_dispatch_plan(int* perm, int* row_expert, float* row_w, int* inv, int* seg, const float* sparse, int B, int E, int kcap,
                        hipStream_t stream) {
  if (B < 1 || E < 1 || E > 64 || kcap < 1 || kcap > E) return HDMOE_EINVAL;
  hipLaunchKernelGGL(dispatch_plan_kernel, dim3(1), dim3(1024), 0, stream, perm, row_expert, row_w, inv, seg, sparse, B, E, kcap);
  return hdmoe_launch_status();
}
// counts[e] = rows routed to expert e in this step (float): the optimizer skips the tensors of an expert without rows, like the reference,
// whose `if not mask.any(): continue` leaves such an expert's gradients None (models/model_config1.py:26-29)
int hdmoe_seg_counts(float* counts, const int* seg, int E, hipStream_t stream) {
  if (!counts || !seg || E < 1 || E > 64) return HDMOE_EINVAL;
  hipLaunchKernelGGL(seg_counts_kernel, dim3(1), dim3(64), 0, stream, counts, seg, E);
  return hdmoe_launch_status();
}
int hdmoe_route_counts(float* counts, const float* sparse, int B, int E, hipStream_t stream) {
  if (!counts || !sparse || B < 1 || E < 1 || E > 64) return HDMOE_EINVAL;
  hipLaunchKernelGGL(route_counts_kernel, dim3(E), dim3(256), 0, stream, counts, sparse, B, E);
  return hdmoe_launch_status();
}
int hdmoe_gather_rows(void* dst, const void* src, const int* perm, long R, long L, int dtype, hipStream_t stream) {
  const long esz = dtype == HDMOE_F32 ? 4 : 2;
  if (dtype != HDMOE_F32 && dtype != HDMOE_BF16) return HDMOE_EDTYPE;
  if ((L * esz) % 16 == 0 && (uintptr_t)dst % 16 == 0 && (uintptr_t)src % 16 == 0) {
    const long Lv = L * esz / 16, n = R * Lv;
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(n)), dim3(TPB), 0, stream, (uint4*)dst, (const uint4*)src, perm, Lv, n);
  } else if (dtype == HDMOE_F32) {
    hipLaunchKernelGGL(gather_rows_scalar_kernel<float>, dim3(grid_for(R * L)), dim3(TPB), 0, stream, (float*)dst, (const float*)src, perm, L, R * L);
  } else {
    hipLaunchKernelGGL(gather_rows_scalar_kernel<bf16>, dim3(grid_for(R * L)), dim3(TPB), 0, stream, (bf16*)dst, (const bf16*)src, perm, L, R * L);
  }
  return hdmoe_launch_status();
}
int hdmoe_gather_rows_paired(void* dst, const void* src, const int* perm, long R, long L, int Bsrc, int dtype, hipStream_t stream) {
  const long esz = dtype == HDMOE_F32 ? 4 : 2;
  if (dtype != HDMOE_F32 && dtype != HDMOE_BF16) return HDMOE_EDTYPE;
  if (!dst || !src || !perm || R < 0 || L < 1 || Bsrc < 1) return HDMOE_EINVAL;
  if (R == 0) return HDMOE_OK;
  if ((L * esz) % 16 == 0 && (uintptr_t)dst % 16 == 0 && (uintptr_t)src % 16 == 0) {
    const long Lv = L * esz / 16, n = R * Lv;
    hipLaunchKernelGGL(gather_rows_paired_kernel, dim3(grid_for(n)), dim3(TPB), 0, stream, (uint4*)dst, (const uint4*)src, perm, Bsrc, Lv, n);
  } else if (dtype == HDMOE_F32) {
    hipLaunchKernelGGL(gather_rows_paired_scalar_kernel<float>, dim3(grid_for(R * L)), dim3(TPB), 0, stream, (float*)dst, (const float*)src, perm, Bsrc, L, R * L);
  } else {
    hipLaunchKernelGGL(gather_rows_paired_scalar_kernel<bf16>, dim3(grid_for(R * L)), dim3(TPB), 0, stream, (bf16*)dst, (const bf16*)src, perm, Bsrc, L, R * L);
  }
  return hdmoe_launch_status();
}
int hdmoe_combine_rows_fwd(void* out, const void* ys, const int* inv, const float* row_w, long B, int kcap, long L, int dtype,
                           hipStream_t stream) {
  const long n = B * L;
  if (dtype == HDMOE_F32) hipLaunchKernelGGL(combine_rows_fwd_kernel<float>, dim3(grid_for(n)), dim3(TPB), 0, stream, (float*)out, (const float*)ys, inv, row_w, kcap, L, n);
  else if (dtype == HDMOE_BF16) hipLaunchKernelGGL(combine_rows_fwd_kernel<bf16>, dim3(grid_for(n)), dim3(TPB), 0, stream, (bf16*)out, (const bf16*)ys, inv, row_w, kcap, L, n);
  else return HDMOE_EDTYPE;
  return hdmoe_launch_status();
}
int hdmoe_combine_rows_bwd(void* dys, float* dsparse, const void* dout, const void* ys, const int* perm, const int* row_expert,
                           const float* row_w, long R, int E, long L, int dtype, hipStream_t stream) {
  const int chunk = 8192;
  if (R < 0 || L < 1 || R * (long)cdiv(L, chunk) >= (1l << 31)) return HDMOE_EINVAL;
  if (R == 0) return HDMOE_OK;
  dim3 grid((unsigned)(R * (long)cdiv(L, chunk)));
  if (dtype == HDMOE_F32) hipLaunchKernelGGL(combine_rows_bwd_kernel<float>, grid, dim3(TPB), 0, stream, (float*)dys, dsparse, (const float*)dout, (const float*)ys, perm, row_expert, row_w, E, L, chunk);
  else if (dtype == HDMOE_BF16) hipLaunchKernelGGL(combine_rows_bwd_kernel<bf16>, grid, dim3(TPB), 0, stream, (bf16*)dys, dsparse, (const bf16*)dout, (const bf16*)ys, perm, row_expert, row_w, E, L, chunk);
  else return HDMOE_EDTYPE;
  return hdmoe_launch_status();
}
int hdmoe_version(void) { return 302; }

}  // extern "C"
