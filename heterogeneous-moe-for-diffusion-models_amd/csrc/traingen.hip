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
//
// hdmoe_dataset_inputs makes the data of the step on the device as well: the per-sample kernel also says which dataset items the batch
// holds (keyed_perm.h) and which of them are mirrored, and one pass gathers their rows, draws the VAE posterior, mirrors, scales and
// noises, writing x0 and x together.  hdmoe_text_gather_dropout is the text side: the dropout kernel with its rows taken through item.
#include "common.h"
#include "hdmoe.h"
#include "keyed_perm.h"

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
  // the dataset's batch (hdmoe_dataset_inputs; item == nullptr: none): item[i] = perm(first + i), flip[i] from the data stream r = 1
  int* item; float* flip;
  KeyedPerm perm;
  uint32_t first, kflo, kfhi;
  float p_flip;
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
  if (a.item) {
    for (int i = threadIdx.x; i < B; i += GEN_TPB) {
      a.item[i] = (int)keyed_perm_at(a.perm, a.first + (uint32_t)i);       // first + B <= N: the host checked it
      uint32_t r[4];
      philox((uint32_t)(i >> 2), 0u, a.kflo, a.kfhi, r);
      const int lane = i & 3;
      const uint32_t w = lane == 0 ? r[0] : lane == 1 ? r[1] : lane == 2 ? r[2] : r[3];
      a.flip[i] = u01(w) < a.p_flip ? 1.f : 0.f;
    }
  }
}

// x = x0 + sigma[b] * eps, W elements per thread (W == 4: chw % 4 == 0, so the four elements share their sample)
template <int W>
__global__ __launch_bounds__(256) void gen_noise_kernel(float* x, const float* x0, const float* sigma, uint32_t lo, uint32_t hi, long chw, long nv) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (long)gridDim.x * blockDim.x) {
    const long off = v * W;
    float p[W], e[W];
    ldw<float, W>(p, x0 + off);
    eps_w<W>(e, off, lo, hi);
    const float sg = sigma[off / chw];
#pragma unroll
    for (int j = 0; j < W; ++j) p[j] = fmaf(sg, e[j], p[j]);
    stw<float, W>(x + off, p);
  }
}

// W elements of a dataset row as fp32 (bf16 storage is converted here); p is W-element aligned when W == 4
template <typename T, int W> DEVI void ld_data(float* f, const T* p) {
  if constexpr (W == 1) f[0] = to_f(*p);
  else if constexpr (sizeof(T) == 4) vload<float>(f, (const float*)p);
  else {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) f[j] = (float)v[j];
  }
}

template <int W> DEVI void rev_w(float* f) {
#pragma unroll
  for (int j = 0; j < W / 2; ++j) { const float t = f[j]; f[j] = f[W - 1 - j]; f[W - 1 - j] = t; }
}

// The dataset's pass: x0[b,c,h,w] = scale (mean[item[b],c,h,w'] + std[...] eps_p), x = x0 + sigma[b] eps, w' = flip[b] ? Wd - 1 - w : w.
// W == 4 needs Wd % 4 == 0: a vector then lies inside one image row, and its mirror image is the aligned vector at Wd - 4 - w with the
// lanes reversed.  eps_p and eps are indexed by the OUTPUT element, so the mirrored read changes no draw.  Row offsets are 64-bit.
template <typename T, int W>
__global__ __launch_bounds__(256) void gen_data_kernel(float* x, float* x0, const float* sigma, const int* item, const float* flip, const T* mean,
                                                       const T* sd, uint32_t lo, uint32_t hi, uint32_t plo, uint32_t phi, long chw, int Wd,
                                                       float scale, long nv) {
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (long)gridDim.x * blockDim.x) {
    const long off = v * W, b = off / chw, rem = off - b * chw;
    const long row = rem / Wd;
    const int w = (int)(rem - row * Wd);
    const bool fl = flip[b] != 0.f;
    const long src = (long)item[b] * chw + row * Wd + (fl ? Wd - W - w : w);
    float m[W], p[W], e[W];
    ld_data<T, W>(m, mean + src);
    if (fl) rev_w<W>(m);
    if (sd) {
      float s[W], z[W];
      ld_data<T, W>(s, sd + src);
      if (fl) rev_w<W>(s);
      eps_w<W>(z, off, plo, phi);
#pragma unroll
      for (int j = 0; j < W; ++j) m[j] = fmaf(s[j], z[j], m[j]);
    }
#pragma unroll
    for (int j = 0; j < W; ++j) p[j] = scale * m[j];
    stw<float, W>(x0 + off, p);
    eps_w<W>(e, off, lo, hi);
    const float sg = sigma[b];
#pragma unroll
    for (int j = 0; j < W; ++j) p[j] = fmaf(sg, e[j], p[j]);
    stw<float, W>(x + off, p);
  }
}

template <typename T>
void launch_gen_data(float* x, float* x0, const float* sigma, const int* item, const float* flip, const void* mean, const void* sd, uint32_t lo,
                     uint32_t hi, uint32_t plo, uint32_t phi, long B, long chw, int Wd, float scale, hipStream_t stream) {
  const long n = B * chw;
  const uintptr_t src_mask = 4 * sizeof(T) - 1;                // a 4-element vector of the storage type
  const bool vec = Wd % 4 == 0 && al16(x) && al16(x0) && !((uintptr_t)mean & src_mask) && !((uintptr_t)sd & src_mask);
  const long nv = vec ? n / 4 : n, blocks = (nv + 255) / 256;
  const dim3 grid((unsigned)(blocks > 2048 ? 2048 : blocks));
  if (vec)
    hipLaunchKernelGGL((gen_data_kernel<T, 4>), grid, dim3(256), 0, stream, x, x0, sigma, item, flip, (const T*)mean, (const T*)sd, lo, hi, plo,
                       phi, chw, Wd, scale, nv);
  else
    hipLaunchKernelGGL((gen_data_kernel<T, 1>), grid, dim3(256), 0, stream, x, x0, sigma, item, flip, (const T*)mean, (const T*)sd, lo, hi, plo,
                       phi, chw, Wd, scale, nv);
}

// Rows of row_n elements of T (uint4 on the 16-byte path), cut into `segs` equal segments of seg_len <= DROP_SEG elements; one segment
// per workgroup and trip.  The drop decision is uniform over the workgroup (draw d_i of include/hdmoe.h: word i % 4 of block (i / 4,
// c1 = 1) under the r = 3 key), so it is scalar work in front of the segment's loads: long segments, DROP_U independent loads per
// thread, keep that preamble small beside the traffic (measured at (256, 77 x 768) fp32: DROP_U = 4 / 8 / 16 -> 18.7 / 18.0 / 17.7 us).
constexpr int DROP_TPB = 256;
constexpr int DROP_U = 16;
constexpr int DROP_SEG = DROP_TPB * DROP_U;

// Row indirection of hdmoe_text_gather_dropout (G): `text` is the dataset's table and row i comes from its row text_index[item[i]], 0
// (single: one fixed prompt) or item[i].  Without it (hdmoe_text_dropout) row i of `text` is read and `rows` is not looked at: that
// instantiation is the kernel as it was.
struct TextRows {
  const int* item; const int* text_index; int single;
};

template <typename T, bool G>
__global__ __launch_bounds__(DROP_TPB) void text_dropout_kernel(T* out, float* keep, const T* text, const T* null_row, TextRows rows, uint32_t klo,
                                                                 uint32_t khi, long row_n, long seg_len, long segs, long units, float p) {
  for (long u = blockIdx.x; u < units; u += gridDim.x) {
    const long i = u / segs, s = u - i * segs;
    uint32_t r[4];
    philox((uint32_t)(i >> 2), 1u, klo, khi, r);
    const int lane = (int)(i & 3);
    const uint32_t w = lane == 0 ? r[0] : lane == 1 ? r[1] : lane == 2 ? r[2] : r[3];
    const bool drop = u01(w) < p;
    if (s == 0 && threadIdx.x == 0) keep[i] = drop ? 0.f : 1.f;
    long t = i;
    if constexpr (G) {
      t = rows.item[i];
      if (rows.text_index) t = rows.text_index[t];
      else if (rows.single) t = 0;
    }
    const T* src = drop ? null_row : text + t * row_n;       // nullptr: a dropped row without a null row is zeros
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
void launch_text_dropout(void* out, float* keep, const void* text, const void* null_row, TextRows rows, uint32_t klo, uint32_t khi, long B,
                         long row_n, float p, hipStream_t stream) {
  const long segs = (row_n + DROP_SEG - 1) / DROP_SEG, seg_len = (row_n + segs - 1) / segs, units = B * segs;
  const long trips = (units + 2047) / 2048, grid = (units + trips - 1) / trips;      // <= 2048 workgroups, the same trips for all but the last
  if (rows.item)
    hipLaunchKernelGGL((text_dropout_kernel<T, true>), dim3((unsigned)grid), dim3(DROP_TPB), 0, stream, (T*)out, keep, (const T*)text,
                       (const T*)null_row, rows, klo, khi, row_n, seg_len, segs, units, p);
  else
    hipLaunchKernelGGL((text_dropout_kernel<T, false>), dim3((unsigned)grid), dim3(DROP_TPB), 0, stream, (T*)out, keep, (const T*)text,
                       (const T*)null_row, rows, klo, khi, row_n, seg_len, segs, units, p);
}

inline void stream_key(unsigned long long seed, unsigned long long ctr, uint32_t& lo, uint32_t& hi) {   // mix_seed on the host
  const unsigned long long k = seed + ctr * 0x9E3779B97F4A7C15ull;
  lo = (uint32_t)k; hi = (uint32_t)(k >> 32);
}

// both text entry points: the key, the access path and the launch
int text_rows(void* out, float* keep, const void* text, const void* null_row, TextRows rows, unsigned long long seed,
                     unsigned long long step, long B, long row, int elem_bytes, double p, hipStream_t stream) {
  uint32_t lo, hi;
  stream_key(seed, 4ull * step + 3ull, lo, hi);
  const long bytes = row * elem_bytes;
  if (bytes % 16 == 0 && al16(out) && al16(text) && al16(null_row))
    launch_text_dropout<uint4>(out, keep, text, null_row, rows, lo, hi, B, bytes / 16, (float)p, stream);
  else if (elem_bytes == 4)
    launch_text_dropout<uint32_t>(out, keep, text, null_row, rows, lo, hi, B, row, (float)p, stream);
  else
    launch_text_dropout<uint16_t>(out, keep, text, null_row, rows, lo, hi, B, row, (float)p, stream);
  return hdmoe_launch_status();
}

constexpr unsigned long long DATA_SALT = 0xE7037ED1A0B428DBull;      // the dataset's streams: keys (seed ^ DATA_SALT) + (4 step + r) golden

// validation and the per-sample kernel's arguments that hdmoe_train_inputs and hdmoe_dataset_inputs share; false: HDMOE_EINVAL
bool gen_args(GenArgs& a, float* sigma, float* unet_mask, float* vit_mask, float* zeta_out, int* src, const float* unet_centers,
              const float* vit_centers, unsigned long long seed, unsigned long long step, long B, long chw, int E, int min_active,
              double sigma_min, double sigma_max, double p_mean, double p_std, double extreme_prob, double unet_bw, double vit_bw, float zeta) {
  if (!sigma || !unet_mask || !vit_mask || !zeta_out || !src || !unet_centers || !vit_centers) return false;
  if (B < 1 || B > GEN_MAXB || chw < 1 || E < 1 || E > GEN_MAXE || min_active < 0 || min_active > E) return false;
  if (!(sigma_min > 0.0) || !(sigma_max >= sigma_min) || !(extreme_prob >= 0.0 && extreme_prob <= 1.0)) return false;
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
  a.item = nullptr; a.flip = nullptr; a.perm = KeyedPerm{}; a.first = 0u; a.kflo = a.kfhi = 0u; a.p_flip = 0.f;
  return true;
}

}  // namespace

extern "C" {

int hdmoe_train_inputs(float* x, float* sigma, float* unet_mask, float* vit_mask, float* zeta_out, int* src, const float* x0,
                       const float* unet_centers, const float* vit_centers, unsigned long long seed, unsigned long long step, long B, long chw,
                       int E, int min_active, double sigma_min, double sigma_max, double p_mean, double p_std, double extreme_prob,
                       double unet_bw, double vit_bw, float zeta, hipStream_t stream) {
  if (!x || !x0) return HDMOE_EINVAL;
  GenArgs a;
  if (!gen_args(a, sigma, unet_mask, vit_mask, zeta_out, src, unet_centers, vit_centers, seed, step, B, chw, E, min_active, sigma_min, sigma_max,
                p_mean, p_std, extreme_prob, unet_bw, vit_bw, zeta))
    return HDMOE_EINVAL;
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

int hdmoe_dataset_perm(int* out, unsigned long long seed, unsigned long long epoch, long N, long first, long count) {
  if (!out || N < 1 || N >= (1l << 31) || first < 0 || count < 0 || first > N || count > N - first) return HDMOE_EINVAL;
  const KeyedPerm p = keyed_perm_make(seed, epoch, (uint32_t)N);
  for (long i = 0; i < count; ++i) out[i] = (int)keyed_perm_at(p, (uint32_t)(first + i));
  return HDMOE_OK;
}

int hdmoe_dataset_inputs(float* x, float* x0, float* sigma, float* unet_mask, float* vit_mask, float* zeta_out, int* src, int* item, float* flip,
                         const void* mean, const void* std_dev, int data_dtype, const float* unet_centers, const float* vit_centers,
                         unsigned long long seed, unsigned long long data_seed, unsigned long long step, long B, long chw, long N, int H, int W,
                         int world, int rank, double scale, double p_flip, int E, int min_active, double sigma_min, double sigma_max,
                         double p_mean, double p_std, double extreme_prob, double unet_bw, double vit_bw, float zeta, hipStream_t stream) {
  if (!x || !x0 || !item || !flip || !mean || x == x0) return HDMOE_EINVAL;
  if (N < 1 || N >= (1l << 31) || H < 1 || W < 1 || chw < 1 || chw % ((long)H * W) != 0 || world < 1 || rank < 0 || rank >= world)
    return HDMOE_EINVAL;
  if (B < 1 || B > GEN_MAXB || B * (long)world > N || !(p_flip >= 0.0 && p_flip <= 1.0) || !(scale == scale)) return HDMOE_EINVAL;
  if (data_dtype != HDMOE_F32 && data_dtype != HDMOE_BF16) return HDMOE_EDTYPE;
  GenArgs a;
  if (!gen_args(a, sigma, unet_mask, vit_mask, zeta_out, src, unet_centers, vit_centers, seed, step, B, chw, E, min_active, sigma_min, sigma_max,
                p_mean, p_std, extreme_prob, unet_bw, vit_bw, zeta))
    return HDMOE_EINVAL;
  const unsigned long long per = (unsigned long long)(B * world), spe = (unsigned long long)N / per;      // steps per epoch: drop_last
  const unsigned long long dseed = seed ^ DATA_SALT;
  a.item = item; a.flip = flip; a.p_flip = (float)p_flip;
  a.perm = keyed_perm_make(data_seed, step / spe, (uint32_t)N);
  a.first = (uint32_t)((step % spe) * per + (unsigned long long)rank * (unsigned long long)B);              // first + B <= spe * per <= N
  stream_key(dseed, 4ull * step + 1ull, a.kflo, a.kfhi);
  hipLaunchKernelGGL(gen_small_kernel, dim3(1), dim3(GEN_TPB), 0, stream, a);
  uint32_t lo, hi, plo, phi;
  stream_key(seed, 4ull * step, lo, hi);
  stream_key(dseed, 4ull * step, plo, phi);
  if (data_dtype == HDMOE_F32)
    launch_gen_data<float>(x, x0, sigma, item, flip, mean, std_dev, lo, hi, plo, phi, B, chw, W, (float)scale, stream);
  else
    launch_gen_data<bf16>(x, x0, sigma, item, flip, mean, std_dev, lo, hi, plo, phi, B, chw, W, (float)scale, stream);
  return hdmoe_launch_status();
}

int hdmoe_text_dropout(void* out, float* keep, const void* text, const void* null_row, unsigned long long seed, unsigned long long step,
                       long B, long row, int elem_bytes, double p, hipStream_t stream) {
  if (!out || !keep || !text || out == text) return HDMOE_EINVAL;
  if (B < 1 || row < 1 || (elem_bytes != 2 && elem_bytes != 4) || !(p >= 0.0 && p <= 1.0)) return HDMOE_EINVAL;
  return text_rows(out, keep, text, null_row, TextRows{nullptr, nullptr, 0}, seed, step, B, row, elem_bytes, p, stream);
}

int hdmoe_text_gather_dropout(void* out, float* keep, const void* table, const int* text_index, const int* item, const void* null_row,
                              unsigned long long seed, unsigned long long step, long B, long K, long N, long row, int elem_bytes, double p,
                              hipStream_t stream) {
  if (!out || !keep || !table || !item || out == table) return HDMOE_EINVAL;
  if (B < 1 || K < 1 || N < 1 || row < 1 || (elem_bytes != 2 && elem_bytes != 4) || !(p >= 0.0 && p <= 1.0)) return HDMOE_EINVAL;
  if (!text_index && K != 1 && K != N) return HDMOE_EINVAL;
  return text_rows(out, keep, table, null_row, TextRows{item, text_index, !text_index && K == 1 ? 1 : 0}, seed, step, B, row, elem_bytes, p, stream);
}

}  // extern "C"
