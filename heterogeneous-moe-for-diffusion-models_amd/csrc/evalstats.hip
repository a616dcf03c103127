// Held-out evaluation on the device (no counterpart in the reference, whose only quality signal is the training loss of the current
// batch; its graphs/plotter.py plot_expert_specialization_advanced probes the routers with a dummy input over a sigma grid).
//
// hdmoe_eval_inputs makes one evaluation batch from a LatentDataset-style table: fixed sigma levels, the posterior mean as the target and
// noise keyed by (seed, item, level) -- see the RNG contract in include/hdmoe.h -- so the batch of an (item, level) pair does not depend
// on the batch size, the position in the batch, the round or the rank.  One launch, an HBM-bound pass like gen_data_kernel.
//
// hdmoe_eval_accumulate adds the batch's statistics into a (K, 6 + 4E) table of doubles, per noise level: the denoising error and the
// gate probabilities of both routers.  Two launches, no atomics and no memset node.  The first writes one fp32 partial sum of squares
// per (sample, EVAL_CHUNK elements); the second is ONE workgroup that sums them per level, in sample order, in double.  The order of
// every sum is fixed by (B, L) alone, so the same inputs give the same bits, eager or replayed.
#include "common.h"
#include "hdmoe.h"

namespace {

constexpr unsigned long long EVAL_SALT = 0x8EBC6AF09C88C6E3ull;      // the evaluation noise: keys (seed ^ EVAL_SALT) + (item K + level) golden
constexpr int EVAL_MAXB = 4096;
constexpr int EVAL_MAXE = 8;
constexpr int EVAL_MAXK = 64;
constexpr int EVAL_CHUNK = 4096;                                     // elements per partial sum: fixed, so the sums do not depend on B
constexpr int EVAL_TPB = 256;
constexpr int EVAL_F_MAX = 6 + 4 * EVAL_MAXE;
constexpr int EVAL_SLOTS = (EVAL_MAXK * EVAL_F_MAX + EVAL_TPB - 1) / EVAL_TPB;   // (level, field) sums per thread of the finish kernel

template <typename T, int W> DEVI void ld_row(float* f, const T* p) {
  if constexpr (W == 1) f[0] = to_f(*p);
  else if constexpr (sizeof(T) == 4) vload<float>(f, (const float*)p);
  else {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = (float)v[j];
  }
}

// x0[b] = scale mean[item[b]], x[b] = x0[b] + sigma[b] eps, eps element j of the row = element j of hdmoe_randn under the row's own key.
// W == 4 needs chw % 4 == 0: a vector then lies inside one row and starts at a multiple of 4 of it, i.e. is one Philox block.
template <typename T, int W>
__global__ __launch_bounds__(256) void eval_inputs_kernel(float* x, float* x0, float* sigma, int* level, int* item, const T* mean,
                                                          const float* levels, unsigned long long key0, long first, int round, int count,
                                                          long chw, long N, int K, float scale, long nv) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (long)gridDim.x * blockDim.x) {
    const long off = v * W, b = off / chw, j = off - b * chw;
    const long it = (first + b) % N;
    const int k = (int)((it + round) % K);
    const float sg = levels[k];
    if (j == 0) {
      item[b] = (int)it;
      level[b] = b < count ? k : -1;
      sigma[b] = sg;
    }
    const unsigned long long key = key0 + (unsigned long long)(it * K + k) * 0x9E3779B97F4A7C15ull;
    float m[W], e[W];
    ld_row<T, W>(m, mean + it * chw + j);
#pragma unroll
    for (int q = 0; q < W; ++q) m[q] = scale * m[q];
    stw<float, W>(x0 + off, m);
    eps_w<W>(e, j, (uint32_t)key, (uint32_t)(key >> 32));
#pragma unroll
    for (int q = 0; q < W; ++q) m[q] = fmaf(sg, e[q], m[q]);
    stw<float, W>(x + off, m);
  }
}

template <typename T>
void launch_eval_inputs(float* x, float* x0, float* sigma, int* level, int* item, const void* mean, const float* levels,
                        unsigned long long key0, long first, int round, int count, long B, long chw, long N, int K, float scale,
                        hipStream_t stream) {
  const long n = B * chw;
  const uintptr_t src_mask = 4 * sizeof(T) - 1;                // a 4-element vector of the storage type
  const bool vec = chw % 4 == 0 && al16(x) && al16(x0) && !((uintptr_t)mean & src_mask);
  const long nv = vec ? n / 4 : n, blocks = (nv + 255) / 256;
  const dim3 grid((unsigned)(blocks > 2048 ? 2048 : blocks));
  if (vec)
    hipLaunchKernelGGL((eval_inputs_kernel<T, 4>), grid, dim3(256), 0, stream, x, x0, sigma, level, item, (const T*)mean, levels, key0, first,
                       round, count, chw, N, K, scale, nv);
  else
    hipLaunchKernelGGL((eval_inputs_kernel<T, 1>), grid, dim3(256), 0, stream, x, x0, sigma, level, item, (const T*)mean, levels, key0, first,
                       round, count, chw, N, K, scale, nv);
}

// ws[b][c] = sum over chunk c of row b of (d - t)^2 in fp32: 16 terms per thread in index order, then block_sum's tree (6 butterfly
// steps inside a wave, the 4 wave sums one after the other) -- the longest chain of fp32 additions is 16 + 6 + 4 = 26 terms.
__global__ __launch_bounds__(EVAL_TPB) void eval_sse_kernel(float* ws, const float* d, const float* t, long L, int nchunks) {
  __shared__ float sm[16];
  const long b = blockIdx.y, p0 = (long)blockIdx.x * EVAL_CHUNK;
  const long p1 = p0 + EVAL_CHUNK < L ? p0 + EVAL_CHUNK : L;
  float acc = 0.f;
  for (long i = p0 + threadIdx.x; i < p1; i += EVAL_TPB) { const float e = d[b * L + i] - t[b * L + i]; acc += e * e; }
  acc = block_sum(acc, sm);
  if (threadIdx.x == 0) ws[b * nchunks + blockIdx.x] = acc;
}

// torch.clamp semantics: NaN propagates
DEVI float clamp_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// One workgroup.  Rows go through LDS in tiles of EVAL_TPB: thread r of a tile makes row b's five error terms in double and copies its
// gate probabilities; then thread o owns the sums (level, field) = o, o + EVAL_TPB, ... and walks the tile's rows in order, so every
// sum runs over its level's samples in sample order whatever K, E and B are.  A row whose level lies outside [0, K) matches no sum:
// it is skipped and never indexes acc.
__global__ __launch_bounds__(EVAL_TPB) void eval_finish_kernel(double* acc, const float* ws, const float* sigma, const int* level,
                                                               const float* log_var, const float* pU, const float* pV, int B, long L, int E,
                                                               int K, int nchunks, double sd2) {
  __shared__ double s_val[5][EVAL_TPB];                    // mse, mse^2, w mse, mse exp(-lv) + lv, lv
  __shared__ float s_p[EVAL_TPB][2 * EVAL_MAXE];           // pU | pV of the row
  __shared__ int s_lvl[EVAL_TPB];
  const int tid = threadIdx.x, F = 6 + 4 * E, nout = K * F;
  double sum[EVAL_SLOTS];
#pragma unroll
  for (int s = 0; s < EVAL_SLOTS; ++s) sum[s] = 0.0;
  for (int base = 0; base < B; base += EVAL_TPB) {
    const int rows = B - base < EVAL_TPB ? B - base : EVAL_TPB;
    __syncthreads();                                       // the previous tile has been read
    if (tid < rows) {
      const long b = base + tid;
      double sse = 0.0;
      for (int c = 0; c < nchunks; ++c) sse += (double)ws[b * nchunks + c];
      const double mse = sse / (double)L, sg = (double)sigma[b];
      const double lv = log_var ? (double)clamp_nan(log_var[b], -10.f, 10.f) : 0.0;
      s_val[0][tid] = mse;
      s_val[1][tid] = mse * mse;
      s_val[2][tid] = (sg * sg + sd2) / (sg * sg * sd2) * mse;
      s_val[3][tid] = mse * exp(-lv) + lv;
      s_val[4][tid] = lv;
      for (int e = 0; e < E; ++e) { s_p[tid][e] = pU[b * E + e]; s_p[tid][EVAL_MAXE + e] = pV[b * E + e]; }
      s_lvl[tid] = level[b];
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < EVAL_SLOTS; ++s) {
      const int o = tid + s * EVAL_TPB;
      if (o < nout) {
        const int k = o / F, f = o - k * F;
        const int g = f - 6, which = g >= 0 ? g / E : 0, e = g >= 0 ? g - which * E : 0;
        const int col = (which >> 1) * EVAL_MAXE + e;      // which: 0 sum pU, 1 count pU > 0, 2 sum pV, 3 count pV > 0
        double a = sum[s];
        // rows of other levels cost one broadcast LDS read and a compare.  (A branch-free walk that reads both sources for every row
        // and selects the term was no faster at B = 256, K = 16: 60 against 48 us for the two launches, on a box whose other figures were 12 % up.)
        for (int r = 0; r < rows; ++r) {
          if (s_lvl[r] != k) continue;
          if (f == 0) a += 1.0;
          else if (f < 6) a += s_val[f - 1][r];
          else if (which & 1) a += s_p[r][col] > 0.f ? 1.0 : 0.0;
          else a += (double)s_p[r][col];
        }
        sum[s] = a;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < EVAL_SLOTS; ++s) {
    const int o = tid + s * EVAL_TPB;
    if (o < nout) acc[o] += sum[s];
  }
}

}  // namespace

extern "C" {

int hdmoe_eval_chunk(void) { return EVAL_CHUNK; }

int hdmoe_eval_inputs(float* x, float* x0, float* sigma, int* level, int* item, const void* mean, int data_dtype, const float* levels,
                      unsigned long long seed, int round, long first, long count, long B, long chw, long N, int K, double scale,
                      hipStream_t stream) {
  if (!x || !x0 || !sigma || !level || !item || !mean || !levels || x == x0) return HDMOE_EINVAL;
  if (B < 1 || B > EVAL_MAXB || chw < 1 || N < 1 || N >= (1l << 31) || K < 1 || K > EVAL_MAXK) return HDMOE_EINVAL;
  if (count < 0 || count > B || first < 0 || first > (1l << 62) || round < 0 || !(scale == scale)) return HDMOE_EINVAL;
  if (data_dtype != HDMOE_F32 && data_dtype != HDMOE_BF16) return HDMOE_EDTYPE;
  const unsigned long long key0 = seed ^ EVAL_SALT;
  if (data_dtype == HDMOE_F32)
    launch_eval_inputs<float>(x, x0, sigma, level, item, mean, levels, key0, first, round, (int)count, B, chw, N, K, (float)scale, stream);
  else
    launch_eval_inputs<bf16>(x, x0, sigma, level, item, mean, levels, key0, first, round, (int)count, B, chw, N, K, (float)scale, stream);
  return hdmoe_launch_status();
}

int hdmoe_eval_accumulate(double* acc, float* ws, const float* denoised, const float* x0, const float* sigma, const int* level,
                          const float* log_var, const float* pU, const float* pV, int B, long L, int E, int K, double sigma_data,
                          hipStream_t stream) {
  if (!acc || !ws || !denoised || !x0 || !sigma || !level || !pU || !pV) return HDMOE_EINVAL;
  if (B < 1 || B > EVAL_MAXB || L < 1 || E < 1 || E > EVAL_MAXE || K < 1 || K > EVAL_MAXK) return HDMOE_EINVAL;
  const int nchunks = (int)((L + EVAL_CHUNK - 1) / EVAL_CHUNK);
  if ((L + EVAL_CHUNK - 1) / EVAL_CHUNK > 65535) return HDMOE_EINVAL;                  // grid.x; a row of 2^28 elements
  hipLaunchKernelGGL(eval_sse_kernel, dim3(nchunks, B), dim3(EVAL_TPB), 0, stream, ws, denoised, x0, L, nchunks);
  hipLaunchKernelGGL(eval_finish_kernel, dim3(1), dim3(EVAL_TPB), 0, stream, acc, ws, sigma, level, log_var, pU, pV, B, L, E, K, nchunks,
                     sigma_data * sigma_data);
  return hdmoe_launch_status();
}

}  // extern "C"
