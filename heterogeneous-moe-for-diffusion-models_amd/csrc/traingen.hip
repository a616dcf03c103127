// Training inputs of one step, generated on the device (reference Utils/utils.py:26-61 sample_sigma_hybrid, :228-330 MaskGenerator,
// training.py:125-135 the noising): sigma, the noised latents, both router masks and zeta go straight into the static buffers the
// captured step reads.  Keyed by (seed, step) alone -- see the RNG contract in include/hdmoe.h -- so a resumed run regenerates its inputs.
//
// Two launches.  The per-sample part (B <= 4096 values, a B x B ranking) is one workgroup: it needs all B shuffle keys at once, and in
// LDS the ranking is B broadcast reads per position.  The noising is a plain HBM-bound pass over B * chw elements on the whole device
// and reads the sigma the first kernel wrote; fusing the two would make every workgroup of the large pass repeat the ranking.
//
// hdmoe_text_dropout is the conditioning dropout of the same step (classifier-free guidance): the copy of the text embeddings into
// their static buffer with a per-sample substitution by the null row folded in.  Its decision is one Philox block per sample, which
// every workgroup draws again for the row segment it moves -- unlike the ranking, that is nothing beside the segment's tens of KB.
#include "common.h"
#include "hdmoe.h"

namespace {

constexpr int GEN_MAXB = 4096;
constexpr int GEN_MAXE = 8;
constexpr int GEN_TPB = 1024;

struct GenArgs {
  float* sigma; float* umask; float* vmask; float* zeta_out; int* src;
  const float* ucen; const float* vcen;
  uint32_t k1lo, k1hi, k2lo, k2hi, k3lo, k3hi;          // Philox keys of the streams r = 1, 2, 3
  int B, E, n_ln, min_active;
  float sigma_min, sigma_max, p_mean, p_std, ln_min, ln_span, inv_denom, ubw, vbw, zeta;
};

// mask row of one sample: band test + the min_active nearest experts (rank of dist_e among the E distances, ties to the lower index)
DEVI void mask_row(float* out, const float* cen, float pct, float bw, int E, int min_active) {
  float d[GEN_MAXE];
#pragma unroll
  for (int e = 0; e < GEN_MAXE; ++e) d[e] = e < E ? fabsf(pct - cen[e]) : 0.f;
#pragma unroll
  for (int e = 0; e < GEN_MAXE; ++e) {
    if (e < E) {
      int rank = 0;
#pragma unroll
      for (int f = 0; f < GEN_MAXE; ++f)
        if (f < E && (d[f] < d[e] || (d[f] == d[e] && f < e))) ++rank;
      out[e] = (d[e] <= bw || rank < min_active) ? 1.f : 0.f;
    }
  }
}

__global__ __launch_bounds__(GEN_TPB) void gen_small_kernel(GenArgs a) {
  __shared__ float s_val[GEN_MAXB];                       // pre-shuffle sigma values
  __shared__ __attribute__((aligned(16))) float s_key[GEN_MAXB];   // shuffle keys (padded with +inf to a multiple of 4)
  const int B = a.B, nq = (B + 3) >> 2;
  for (int q = threadIdx.x; q < nq; q += GEN_TPB) {
    float z[4];
    uint32_t ru[4], rk[4];
    randn4(q, a.k1lo, a.k1hi, z);
    philox((uint32_t)q, 0u, a.k2lo, a.k2hi, ru);
    philox((uint32_t)q, 0u, a.k3lo, a.k3hi, rk);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int s = 4 * q + j;
      const float v = s < a.n_ln ? expf(a.p_mean + a.p_std * z[j]) : expf(a.ln_min + a.ln_span * u01(ru[j]));
      s_val[s] = fminf(fmaxf(v, a.sigma_min), a.sigma_max);
      s_key[s] = s < B ? u01(rk[j]) : __builtin_inff();
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < B; i += GEN_TPB) {
    const float k = s_key[i];
    int rank = 0;
    for (int q = 0; q < nq; ++q) {                        // every lane reads the same 16 bytes: an LDS broadcast
      const float4 o = *reinterpret_cast<const float4*>(&s_key[4 * q]);
      const int j = 4 * q;
      rank += (o.x < k || (o.x == k && j < i)) ? 1 : 0;
      rank += (o.y < k || (o.y == k && j + 1 < i)) ? 1 : 0;
      rank += (o.z < k || (o.z == k && j + 2 < i)) ? 1 : 0;
      rank += (o.w < k || (o.w == k && j + 3 < i)) ? 1 : 0;
    }
    const float sg = s_val[rank];                         // rank < B: at most B - 1 of the B finite keys come before key i
    a.src[i] = rank;
    a.sigma[i] = sg;
    const float t = (logf(sg) - a.p_mean) * a.inv_denom;
    const float pct = fminf(fmaxf(0.5f * (1.f + erff(t)), 0.f), 1.f);
    mask_row(a.umask + (long)i * a.E, a.ucen, pct, a.ubw, a.E, a.min_active);
    mask_row(a.vmask + (long)i * a.E, a.vcen, pct, a.vbw, a.E, a.min_active);
  }
  if (threadIdx.x == 0) *a.zeta_out = a.zeta;
}

// x = x0 + sigma[b] * eps, W elements per thread (W == 4: chw % 4 == 0, so the four elements share their sample)
template <int W>
__global__ __launch_bounds__(256) void gen_noise_kernel(float* x, const float* x0, const float* sigma, uint32_t lo, uint32_t hi, long chw, long nv) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (long)gridDim.x * blockDim.x) {
    const long off = v * W;
    float p[W], e[W];
    ldw<W>(p, x0 + off);
    eps_w<W>(e, off, lo, hi);
    const float sg = sigma[off / chw];
#pragma unroll
    for (int j = 0; j < W; ++j) p[j] = fmaf(sg, e[j], p[j]);
    stw<W>(x + off, p);
  }
}

// Rows of row_n elements of T (uint4 on the 16-byte path), cut into `segs` equal segments of seg_len <= DROP_SEG elements; one segment
// per workgroup and trip.  The drop decision is uniform over the workgroup (draw d_i of include/hdmoe.h: word i % 4 of block (i / 4,
// c1 = 1) under the r = 3 key), so it is scalar work in front of the segment's loads: long segments, DROP_U independent loads per
// thread, keep that preamble small beside the traffic (measured at (256, 77 x 768) fp32: DROP_U = 4 / 8 / 16 -> 18.7 / 18.0 / 17.7 us).
constexpr int DROP_TPB = 256;
constexpr int DROP_U = 16;
constexpr int DROP_SEG = DROP_TPB * DROP_U;

template <typename T>
__global__ __launch_bounds__(DROP_TPB) void text_dropout_kernel(T* out, float* keep, const T* text, const T* null_row, uint32_t klo,
                                                                 uint32_t khi, long row_n, long seg_len, long segs, long units, float p) {
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long i = u / segs, s = u - i * segs;
    uint32_t r[4];
    philox((uint32_t)(i >> 2), 1u, klo, khi, r);
    const int lane = (int)(i & 3);
    const uint32_t w = lane == 0 ? r[0] : lane == 1 ? r[1] : lane == 2 ? r[2] : r[3];
    const bool drop = u01(w) < p;
    if (s == 0 && threadIdx.x == 0) keep[i] = drop ? 0.f : 1.f;
    const T* src = drop ? null_row : text + i * row_n;       // nullptr: a dropped row without a null row is zeros
    T* dst = out + i * row_n;
    const long e0 = s * seg_len + threadIdx.x;
    const long end = e0 - threadIdx.x + seg_len < row_n ? e0 - threadIdx.x + seg_len : row_n;
    T v[DROP_U];
#pragma unroll
    for (int j = 0; j < DROP_U; ++j) {
      const long e = e0 + (long)j * DROP_TPB;
      v[j] = T{};
      if (src && e < end) v[j] = src[e];
    }
#pragma unroll
    for (int j = 0; j < DROP_U; ++j) {
      const long e = e0 + (long)j * DROP_TPB;
      if (e < end) dst[e] = v[j];
    }
  }
}

template <typename T>
void launch_text_dropout(void* out, float* keep, const void* text, const void* null_row, uint32_t klo, uint32_t khi, long B, long row_n,
                         float p, hipStream_t stream) {
  const long segs = (row_n + DROP_SEG - 1) / DROP_SEG, seg_len = (row_n + segs - 1) / segs, units = B * segs;
  const long trips = (units + 2047) / 2048, grid = (units + trips - 1) / trips;      // <= 2048 workgroups, the same trips for all but the last
  hipLaunchKernelGGL(text_dropout_kernel<T>, dim3((unsigned)grid), dim3(DROP_TPB), 0, stream, (T*)out, keep, (const T*)text,
                     (const T*)null_row, klo, khi, row_n, seg_len, segs, units, p);
}

inline void stream_key(unsigned long long seed, unsigned long long ctr, uint32_t& lo, uint32_t& hi) {   // mix_seed on the host
  const unsigned long long k = seed + ctr * 0x9E3779B97F4A7C15ull;
  lo = (uint32_t)k; hi = (uint32_t)(k >> 32);
}

}  // namespace

extern "C" {

int hdmoe_train_inputs(float* x, float* sigma, float* unet_mask, float* vit_mask, float* zeta_out, int* src, const float* x0,
                       const float* unet_centers, const float* vit_centers, unsigned long long seed, unsigned long long step, long B, long chw,
                       int E, int min_active, double sigma_min, double sigma_max, double p_mean, double p_std, double extreme_prob,
                       double unet_bw, double vit_bw, float zeta, hipStream_t stream) {
  if (!x || !sigma || !unet_mask || !vit_mask || !zeta_out || !src || !x0 || !unet_centers || !vit_centers) return HDMOE_EINVAL;
  if (B < 1 || B > GEN_MAXB || chw < 1 || E < 1 || E > GEN_MAXE || min_active < 0 || min_active > E) return HDMOE_EINVAL;
  if (!(sigma_min > 0.0) || !(sigma_max >= sigma_min) || !(extreme_prob >= 0.0 && extreme_prob <= 1.0)) return HDMOE_EINVAL;
  GenArgs a;
  a.sigma = sigma; a.umask = unet_mask; a.vmask = vit_mask; a.zeta_out = zeta_out; a.src = src;
  a.ucen = unet_centers; a.vcen = vit_centers;
  stream_key(seed, 4ull * step + 1ull, a.k1lo, a.k1hi);
  stream_key(seed, 4ull * step + 2ull, a.k2lo, a.k2hi);
  stream_key(seed, 4ull * step + 3ull, a.k3lo, a.k3hi);
  a.B = (int)B; a.E = E; a.min_active = min_active;
  a.n_ln = (int)((double)B * (1.0 - extreme_prob));         // the reference's int(batch_size * (1 - extreme_prob)), in double as there
  a.sigma_min = (float)sigma_min; a.sigma_max = (float)sigma_max; a.p_mean = (float)p_mean; a.p_std = (float)p_std;
  a.ln_min = (float)log(sigma_min); a.ln_span = (float)(log(sigma_max) - log(sigma_min));
  a.inv_denom = 1.f / (float)(p_std * sqrt(2.0));
  a.ubw = (float)unet_bw; a.vbw = (float)vit_bw; a.zeta = zeta;
  hipLaunchKernelGGL(gen_small_kernel, dim3(1), dim3(GEN_TPB), 0, stream, a);
  uint32_t lo, hi;
  stream_key(seed, 4ull * step, lo, hi);
  const long n = B * chw;
  if (chw % 4 == 0 && al16(x) && al16(x0)) {
    const long nv = n / 4;
    const long blocks = (nv + 255) / 256;
    hipLaunchKernelGGL(gen_noise_kernel<4>, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, stream, x, x0, sigma, lo, hi, chw, nv);
  } else {
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(gen_noise_kernel<1>, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, stream, x, x0, sigma, lo, hi, chw, n);
  }
  return hdmoe_launch_status();
}

int hdmoe_text_dropout(void* out, float* keep, const void* text, const void* null_row, unsigned long long seed, unsigned long long step,
                       long B, long row, int elem_bytes, double p, hipStream_t stream) {
  if (!out || !keep || !text || out == text) return HDMOE_EINVAL;
  if (B < 1 || row < 1 || (elem_bytes != 2 && elem_bytes != 4) || !(p >= 0.0 && p <= 1.0)) return HDMOE_EINVAL;
  uint32_t lo, hi;
  stream_key(seed, 4ull * step + 3ull, lo, hi);
  const long bytes = row * elem_bytes;
  if (bytes % 16 == 0 && al16(out) && al16(text) && al16(null_row))
    launch_text_dropout<uint4>(out, keep, text, null_row, lo, hi, B, bytes / 16, (float)p, stream);
  else if (elem_bytes == 4)
    launch_text_dropout<uint32_t>(out, keep, text, null_row, lo, hi, B, row, (float)p, stream);
  else
    launch_text_dropout<uint16_t>(out, keep, text, null_row, lo, hi, B, row, (float)p, stream);
  return hdmoe_launch_status();
}

}  // extern "C"
